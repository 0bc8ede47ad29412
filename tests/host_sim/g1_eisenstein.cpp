// TEST HARNESS (CPU): the base-8 Eisenstein recoder and the G1 scalar multiplication of g1.hpp compiled for the host with
// C12381_CHECK_BOUNDS, as a stand-alone program (tests/test_host_sim_g1_eisenstein.py).  Not a product path.
//   g1_eisenstein table            the class table, the chain deltas and whether FP_BETA_B is the square of FP_BETA_A
//   g1_eisenstein recode < pairs   one line "k0 k1" (hex, < 2^128) per pair -> ten hex dwords per line
//   g1_eisenstein digits < ks      one line "k" (hex, < 2^256) per scalar -> ten hex dwords per line (k mod r, split, recoded)
//   g1_eisenstein mul < batch      binary: n (8 bytes LE), n 96-byte points, n 32-byte scalars -> n records of 96 result bytes + 1 byte
//                                  (1 = the lane took g1_scalar_mul_complete), as sim_g1coz_mul_batch of g1_coz.cpp forms them
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"

using namespace c12381;

static bool hex_words(const char* s, uint32_t* w, int nw) {
    const size_t len = std::strlen(s);
    if (len == 0 || len > (size_t)8 * nw) return false;
    for (int i = 0; i < nw; ++i) w[i] = 0;
    for (size_t i = 0; i < len; ++i) {
        const char c = s[len - 1 - i];
        uint32_t v;
        if (c >= '0' && c <= '9') v = c - '0';
        else if (c >= 'a' && c <= 'f') v = c - 'a' + 10;
        else return false;
        w[i / 8] |= v << (4 * (i % 8));
    }
    return true;
}

static void print_digits(const uint32_t (&kd)[10]) {
    for (int i = 0; i < 10; ++i) std::printf("%08x%c", kd[i], i == 9 ? '\n' : ' ');
}

static int mul_batch() {
    uint64_t n = 0;
    if (std::fread(&n, 8, 1, stdin) != 1 || n > (1u << 20)) return 2;
    std::vector<uint8_t> pts(96 * n), sc(32 * n), out(97 * n);
    if (n && (std::fread(pts.data(), 96, n, stdin) != n || std::fread(sc.data(), 32, n, stdin) != n)) return 2;
    std::vector<int32_t> tabv(G1_TAB_DWORDS + 4);
    int32_t* tab = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(tabv.data()) + 15) & ~(uintptr_t)15);
    for (size_t i = 0; i < n; ++i) {
        uint32_t rp[24], rs[8], k[8];
        std::memcpy(rp, pts.data() + 96 * i, 96);
        std::memcpy(rs, sc.data() + 32 * i, 32);
        const bool inf = raw_all_zero(rp, 24);
        fp px, py;
        fp_from_raw48(px, rp); fp_from_raw48(py, rp + 12);
        scalar_from_raw32(k, rs);
        g1p acc;
        uint8_t* o = out.data() + 97 * i;
        o[96] = g1_scalar_mul_eis(acc, px, py, inf, k, tab) ? 1 : 0;
        if (scalar_below_x2(k) && !inf) {
            g1p base, nn;
            base.x = px; base.y = py; fp_one(base.z);
            g1_norm1(nn, acc);
            g1_glv_small_scalar_term(nn, base);
            acc = nn;
        }
        if (g1_is_inf(acc)) { std::memset(o, 0, 96); continue; }
        fp zn, zi, ax, ay;
        fp_norm1(zn, acc.z);
        fp_inv(zi, zn);
        g1_to_affine(ax, ay, acc, zi);
        uint32_t rx[12], ry[12];
        fp_to_raw48(rx, ax); fp_to_raw48(ry, ay);
        std::memcpy(o, rx, 48); std::memcpy(o + 48, ry, 48);
    }
    return std::fwrite(out.data(), 97, n, stdout) == n ? 0 : 2;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "table") {
        for (int c = 0; c < 64; ++c) std::printf("%x%c", (unsigned)EIS_CLASSES.v[c], c == 63 ? '\n' : ' ');
        std::printf("%x\n", EIS_CHAIN_DELTAS);
        fp b, b2, want;
        uint32_t r1[12], r2[12];
        fp_set_const(b, FP_BETA_A);
        fp_set_const(want, FP_BETA_B);
        fp_sqr(b2, b);
        fp_to_raw48(r1, b2); fp_to_raw48(r2, want);
        std::printf("%d\n", std::memcmp(r1, r2, 48) == 0 ? 1 : 0);
        return 0;
    }
    if (mode == "recode" || mode == "digits") {
        char s0[80], s1[80];
        uint32_t kd[10];
        if (mode == "recode") {
            while (std::scanf("%79s %79s", s0, s1) == 2) {
                uint32_t k0[4], k1[4];
                if (!hex_words(s0, k0, 4) || !hex_words(s1, k1, 4)) return 2;
                eis_recode(kd, k0, k1);
                print_digits(kd);
            }
        } else {
            while (std::scanf("%79s", s0) == 1) {
                uint32_t k[8];
                if (!hex_words(s0, k, 8)) return 2;
                eis_scalar_digits(kd, k);
                print_digits(kd);
            }
        }
        return 0;
    }
    if (mode == "mul") return mul_batch();
    std::fprintf(stderr, "usage: g1_eisenstein table | recode | digits | mul\n");
    return 2;
}
