// TEST HARNESS (CPU): g1_scalar_mul_eis of g1.hpp compiled for the host with C12381_CHECK_BOUNDS, as a stand-alone program
// (tests/test_host_sim_g1_eisenstein_seed.py): the product seeded from the top two digits.  Not a product path.
//   g1_eisenstein_seed codes         the digits the seed knows: top 1, top psi, low (-5,2), low (3,-5), seed (2,2), seed (2,3), in hex
//   g1_eisenstein_seed mul < batch   binary: n (8 bytes LE), n 96-byte points, n 32-byte scalars -> n records of 96 result bytes + 1 byte
//                                    (1 = the lane took g1_scalar_mul_complete), as the mul mode of g1_eisenstein.cpp forms them
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"

using namespace c12381;

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
    if (mode == "codes") {
        std::printf("%x %x %x %x %x %x\n", EIS_TOP_ONE, EIS_TOP_PSI, EIS_LOW_ONE, EIS_LOW_PSI, EIS_SEED_ONE, EIS_SEED_PSI);
        return 0;
    }
    if (mode == "mul") return mul_batch();
    std::fprintf(stderr, "usage: g1_eisenstein_seed codes | mul\n");
    return 2;
}
