// TEST HARNESS (CPU): the leaner forms of the single G1 product (g1.hpp) compiled for the host with C12381_CHECK_BOUNDS, as a stand-alone
// program (tests/test_host_sim_g1_lean.py): the nine-reduction mixed addition g1j_madd_eis under g1j_add_eis against g1j_madd under
// g1j_add_signed, the table with beta^2 x = -(x + beta x) against the table built with products, and the whole product.  Not a product path.
//   g1_lean add < lanes     binary: n (8 bytes LE), then n lanes of five operands X1 Y1 Z1 x2 y2 (14 int32 limbs, then the DECLARED bounds lb, vb as
//                           two doubles, each), acc_inf and the digit code (two uint32) -> per lane 86 int32: X Y Z of g1j_add_eis, its acc_inf,
//                           X Y Z of g1j_add_signed over g1j_madd, its acc_inf
//   g1_lean table < points  binary: n, n 96-byte points -> per lane 2 x 630 int32: the 11 x 4 fields (14 limbs each) and Z_T of g1e_table, then
//                           the same of the table as it was built before (every beta^2 x a product; a copy kept below)
//   g1_lean mul < batch     binary: n, n 96-byte points, n 32-byte scalars -> n records of 96 result bytes + 1 byte (1 = the lane took
//                           g1_scalar_mul_complete), as the mul mode of g1_eisenstein_seed.cpp forms them
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"

using namespace c12381;

namespace {

// The table passes as they stood before beta^2 x became a sum: the comparison of the table mode.
void g1e_forward_parent(int32_t* lane_tab, const fp& px, const fp& py, const fp& beta, const fp& beta2) {
    fp x1 = px, y1 = py, xj = px, yj = py, xn, yn, h, hn, bx;
    for (int i = 0; i + 1 < G1E_TAB; ++i) {
        const uint32_t dl = (EIS_CHAIN_DELTAS >> (3 * i)) & 7u, m = dl >= 3u ? dl - 3u : dl;
        if (m != 0u) {
            fp bm;
            fp_select(bm, m == 2u, beta2, beta);
            fp_mul(x1, x1, bm);
        }
        if (dl & 1u) fp_neg(y1, y1);
        g1j_zaddu(xn, yn, x1, y1, h, xj, yj);
        fp_norm1(hn, h);
        int32_t* ent = lane_tab + i * G1E_ENT_DWORDS;
        eis_store_field(ent, 0, yj, 32.0); eis_store_field(ent, 1, xj, 32.0); eis_store_field(ent, 2, hn, 32.0);
        xj = xn; yj = yn;
    }
    int32_t* last = lane_tab + (G1E_TAB - 1) * G1E_ENT_DWORDS;
    eis_store_field(last, 0, yj, 4.0); eis_store_field(last, 1, xj, 4.0);
    fp_mul(bx, xj, beta); eis_store_field(last, 2, bx, 4.0);
    fp_mul(bx, xj, beta2); eis_store_field(last, 3, bx, 4.0);
    eis_store_field(lane_tab, 0, y1, 4.0); eis_store_field(lane_tab, 1, x1, 4.0);
    fp_mul(bx, x1, beta2); eis_store_field(lane_tab, 3, bx, 4.0);
}
void g1e_backward_parent(int32_t* ent, fp& mu, bool first, const fp& beta, const fp& beta2) {
    fp m2, m3, x, y, h, bx;
    eis_load_field(y, ent, 0, 32.0); eis_load_field(x, ent, 1, 32.0); eis_load_field(h, ent, 2, 32.0);
    if (first) mu = h; else fp_mul(mu, mu, h);
    fp_sqr(m2, mu);
    fp_mul(m3, m2, mu);
    fp_mul(x, x, m2);
    fp_mul(y, y, m3);
    eis_store_field(ent, 0, y, 4.0); eis_store_field(ent, 1, x, 4.0);
    fp_mul(bx, x, beta); eis_store_field(ent, 2, bx, 4.0);
    fp_mul(bx, x, beta2); eis_store_field(ent, 3, bx, 4.0);
}
void g1e_table_parent(int32_t* lane_tab, const fp& px, const fp& py) {
    fp beta, beta2;
    fp_set_const(beta, FP_BETA_A);
    fp_set_const(beta2, FP_BETA_B);
    g1e_forward_parent(lane_tab, px, py, beta, beta2);
    fp mu, zt, h0, x, bx;
    for (int i = G1E_TAB - 2; i >= 1; --i) g1e_backward_parent(lane_tab + i * G1E_ENT_DWORDS, mu, i == G1E_TAB - 2, beta, beta2);
    eis_load_field(h0, lane_tab, 2, 32.0);
    eis_load_field(x, lane_tab, 1, 4.0);
    fp_mul(zt, mu, h0);
    fp_mul(bx, x, beta);
    eis_store_field(lane_tab, 2, bx, 4.0);
    eis_store_zt(lane_tab, zt);
}

struct aligned_tab {
    std::vector<int32_t> v = std::vector<int32_t>(G1_TAB_DWORDS + 4);
    int32_t* p = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(v.data()) + 15) & ~(uintptr_t)15);
};

bool read_n(uint64_t& n) { return std::fread(&n, 8, 1, stdin) == 1 && n <= (1u << 20); }

int add_lanes() {
    uint64_t n = 0;
    if (!read_n(n)) return 2;
    std::vector<int32_t> out(86 * n);
    for (size_t i = 0; i < n; ++i) {
        fp op[5];
        for (fp& a : op) {
            double b[2];
            if (std::fread(a.l, 4, NL, stdin) != (size_t)NL || std::fread(b, 8, 2, stdin) != 2) return 2;
            a.lb = b[0]; a.vb = b[1];
            check_actual(a, "g1_lean add: an operand past its declared limb bound");
        }
        uint32_t fl[2];
        if (std::fread(fl, 4, 2, stdin) != 2) return 2;
        const uint32_t code = fl[1];
        g1j a, b;
        a.x = op[0]; a.y = op[1]; a.z = op[2];
        b = a;
        bool ia = fl[0] != 0, ib = ia;
        g1j_add_eis(a, ia, op[3], op[4], code);
        g1j_add_signed(b, ib, op[3], op[4], ((code >> 4) & 1u) != 0u, (code & 15u) == G1E_NONE);
        int32_t* o = out.data() + 86 * i;
        for (int j = 0; j < NL; ++j) {
            o[j] = a.x.l[j]; o[NL + j] = a.y.l[j]; o[2 * NL + j] = a.z.l[j];
            o[43 + j] = b.x.l[j]; o[43 + NL + j] = b.y.l[j]; o[43 + 2 * NL + j] = b.z.l[j];
        }
        o[42] = ia; o[85] = ib;
    }
    return std::fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 2;
}

void dump_table(int32_t* o, const int32_t* tab) {
    for (int e = 0; e < G1E_TAB; ++e)
        for (int f = 0; f < 4; ++f)
            for (int j = 0; j < NL; ++j) *o++ = tab[e * G1E_ENT_DWORDS + f * G1E_FIELD + j];
    fp zt;
    eis_load_zt(zt, tab);
    for (int j = 0; j < NL; ++j) *o++ = zt.l[j];
}

int tables() {
    uint64_t n = 0;
    if (!read_n(n)) return 2;
    std::vector<uint8_t> pts(96 * n);
    if (n && std::fread(pts.data(), 96, n, stdin) != n) return 2;
    std::vector<int32_t> out(1260 * n);
    aligned_tab ta, tb;
    for (size_t i = 0; i < n; ++i) {
        uint32_t rp[24];
        std::memcpy(rp, pts.data() + 96 * i, 96);
        fp px, py;
        fp_from_raw48(px, rp); fp_from_raw48(py, rp + 12);
        g1e_table(ta.p, px, py);
        g1e_table_parent(tb.p, px, py);
        dump_table(out.data() + 1260 * i, ta.p);
        dump_table(out.data() + 1260 * i + 630, tb.p);
    }
    return std::fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 2;
}

int mul_batch() {
    uint64_t n = 0;
    if (!read_n(n)) return 2;
    std::vector<uint8_t> pts(96 * n), sc(32 * n), out(97 * n);
    if (n && (std::fread(pts.data(), 96, n, stdin) != n || std::fread(sc.data(), 32, n, stdin) != n)) return 2;
    aligned_tab t;
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
        o[96] = g1_scalar_mul_eis(acc, px, py, inf, k, t.p) ? 1 : 0;
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

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "add") return add_lanes();
    if (mode == "table") return tables();
    if (mode == "mul") return mul_batch();
    std::fprintf(stderr, "usage: g1_lean add | table | mul\n");
    return 2;
}
