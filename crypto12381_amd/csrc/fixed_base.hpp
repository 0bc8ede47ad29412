// Fixed-base scalar multiplication for the columns of a batch that share ONE public point (the public parameters of
// BBS+ verification, examples/bbs-plus/src/bbs+.cpp:57-73: g2^x, h0^r, h_i^{m_i}).  The reference multiplies every
// element generically (PAIR_G1mul / PAIR_G2mul); for a base IN the order-r subgroup the result is the same point,
// so a table of the base's multiples replaces all doublings:
//   G1: k mod r = k0 + k1 x^2 (the GLV split of g1.hpp), 16 byte-windows per half,
//       [k]B = sum_j T[j][k0_j] + sum_j endo(T[j][k1_j]),  T[j][d] = [d 2^(8j)]B affine, endo(x, y) = (beta x, -y)
//   G2: k mod r = u0 + u1|x| + u2|x|^2 + u3|x|^3 (the GS split of g2.hpp), 8 byte-windows per digit,
//       [k]Q = sum_i (-1)^i sum_j psi^i(T[j][u_i,j])
// 32 mixed additions (g1_add_affine, g2_add_affine) and no doubling per element.  The tables (4080 x 112 B, 2040 x 224 B) are built on the device,
// kept in the context and rebuilt only when the base bytes change.  A base that is not a subgroup point (or is the
// point at infinity, or not on the curve) leaves the table unused: `ok` stays 0 and the generic kernels run instead,
// which reproduce the reference for every input.
#pragma once
#include "g2.hpp"
#include "msm.hpp"

namespace c12381 {

constexpr int FB_ENTRIES = 255;                       // digits 1..255 of an 8-bit window
constexpr int FB_G1_WINDOWS = 16, FB_G2_WINDOWS = 8;
constexpr int FB_G1_DWORDS = MSM_PT_DWORDS;           // affine (x, y) Montgomery, 112 B
constexpr int FB_G2_DWORDS = 4 * NL;                  // affine (x.a, x.b, y.a, y.b), 224 B
constexpr int FB_HEADER_DWORDS = 64;                  // cached base bytes (up to 192) + state words (kernels.hpp: HDR_*), in front of the table

// P in G1  <=>  phi(P) = [-x^2]P  <=>  [x^2]P + (beta X : Y : Z) = infinity   (kernel of phi - lambda has order r)
C12381_HDN bool g1_in_subgroup(const g1p& p) {
    fp beta;
    fp_set_const(beta, FP_BETA_A);
    g1p s, t;
    g1_norm1(s, p);
    g1_mul_absx(s); g1_mul_absx(s);
    g1_norm1(s, s);
    fp_mul(t.x, p.x, beta); t.y = p.y; t.z = p.z;
    g1_norm1(t, t);
    g1_add(s, t);
    return g1_is_inf(s);
}
// Q in G2  <=>  psi(Q) = [x]Q = -[|x|]Q
C12381_HDN bool g2_in_subgroup(const g2p& q) {
    g2p s, t, n;
    g2_norm1(n, q);
    s = n;
    g2_mul_absx(s);
    g2_norm1(s, s);
    g2_psi<1>(t, n);
    g2_norm1(t, t);
    g2_add(s, t);
    return g2_is_inf(s);
}

// [d 2^shift]B with complete formulas (d < 256): 8 ladder steps, then `shift` doublings
C12381_HDN void g1_fixed_entry(g1p& acc, const g1p& base, uint32_t d, int shift) {
    g1p b;
    g1_norm1(b, base);
    g1_set_inf(acc);
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
        g1_dbl(acc);
        if ((d >> bit) & 1u) g1_add(acc, b);
    }
#pragma unroll 1
    for (int s = 0; s < shift; ++s) g1_dbl(acc);
}
C12381_HDN void g2_fixed_entry(g2p& acc, const g2p& base, uint32_t d, int shift) {
    g2p b;
    g2_norm1(b, base);
    g2_set_inf(acc);
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
        g2_dbl(acc);
        if ((d >> bit) & 1u) g2_add(acc, b);
    }
    if (shift > 0) g2_dbl_n(acc, shift);
}

C12381_HD void fb_store_g2(int32_t* dst, const fp2& x, const fp2& y) {
    msm_store_pt(dst, x.a, x.b);
    msm_store_pt(dst + MSM_PT_DWORDS, y.a, y.b);
}
C12381_HD void fb_load_g2(fp2& x, fp2& y, const int32_t* src) {
    msm_load_pt(x.a, x.b, src);
    msm_load_pt(y.a, y.b, src + MSM_PT_DWORDS);
}

// acc += [k]B from the table (k: 8 little-endian words, any value; reduced mod r here).  acc may be ANY point, related to B or not:
// g1_add_affine is complete for a finite affine addend (E(Fp) has odd order) and no table entry is the point at infinity (B has order r,
// the entries are [d 2^(8j)]B with 0 < d < 256), so sums over bases with H2 = +-H1, 2 H1, phi(H1), and sums that pass through or end at
// infinity, need no exceptional path.
C12381_HD void g1_fixed_eval_add(g1p& acc, const int32_t* tab, const uint32_t (&kin)[8]) {
    uint32_t k[8], k0[4], k1[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = kin[i];
    scalar_mod_r(k);
    scalar_glv_split(k0, k1, k);
    fp beta;
    fp_set_const(beta, FP_BETA_A);
#pragma unroll 1
    for (int j = 0; j < FB_G1_WINDOWS; ++j) {
        const uint32_t d0 = (k0[j >> 2] >> (8 * (j & 3))) & 255u, d1 = (k1[j >> 2] >> (8 * (j & 3))) & 255u;
        if (d0) {
            fp x, y;
            msm_load_pt(x, y, tab + ((size_t)j * FB_ENTRIES + (d0 - 1)) * FB_G1_DWORDS);
            g1_add_affine(acc, x, y);
        }
        if (d1) {
            fp x, y, bx, ny;
            msm_load_pt(x, y, tab + ((size_t)j * FB_ENTRIES + (d1 - 1)) * FB_G1_DWORDS);
            fp_mul(bx, x, beta);
            fp_neg(ny, y); fp_norm1(ny, ny);
            g1_add_affine(acc, bx, ny);
        }
    }
}
// acc = [k]B from the table
C12381_HD void g1_fixed_eval(g1p& acc, const int32_t* tab, const uint32_t (&kin)[8]) {
    g1_set_inf(acc);
    g1_fixed_eval_add(acc, tab, kin);
}
template <int I>
C12381_HD void g2_fixed_digit(g2p& acc, const int32_t* tab, const uint32_t (&u)[2]) {
#pragma unroll 1
    for (int j = 0; j < FB_G2_WINDOWS; ++j) {
        const uint32_t d = (u[j >> 2] >> (8 * (j & 3))) & 255u;
        if (d) {
            g2p q, e;
            fb_load_g2(q.x, q.y, tab + ((size_t)j * FB_ENTRIES + (d - 1)) * FB_G2_DWORDS);
            fp2_one(q.z);
            g2_psi_signed<I>(e, q, (I & 1) != 0);
            g2_norm1(e, e);
            g2_add_affine(acc, e.x, e.y);
        }
    }
}
// acc += [k]Q from the table (k: 8 little-endian words, any value; reduced mod r here).  acc may be ANY point of the twist, related to Q or
// not, so sums over bases with H2 = +-H1, 2 H1, psi(H1), and sums that pass through or end at infinity, need no exceptional path:
//   - g2_add_affine (g2.hpp: ECP2_add's complete formulas of Renes-Costello-Batina for a = 0, with Z2 = 1 put in) has no exceptional pair
//     with a finite affine addend on a curve without a point of order 2 over the field of definition, and #E'(Fp2) = h2 r is odd
//     (h2 = 13^2 23^2 2713 11953 262069 times a 135-digit prime, the H2 of tests/g2_twist.py, whose small-order points the tests feed in
//     as addends); acc = infinity is (0 : 1 : 0) and gives the entry itself;
//   - no table entry is the point at infinity: the table is used only for a base of order r (g2_in_subgroup, not infinity) and entry (j, d)
//     is [d 2^(8j)]Q with 0 < d < 256 < r, r prime; psi is a group automorphism of the twist, so +-psi^i of an entry is finite and affine
//     as well (psi maps Z = 1 to conj(1) = 1).
// The mixed form gives the limbs' values of the projective g2_add it replaced, one product in twelve cheaper: 2^18 lanes, nb = 8 / 32:
// 39.5 / 153.8 ms against 45.1 / 176.4 ms, one column 5.3 against 6.05 ms, digests equal (profiles/g2_fixed_sum_mixed_ab.txt).
C12381_HD void g2_fixed_eval_digits(g2p& acc, const int32_t* tab, const uint32_t (&kin)[8]) {
    uint32_t k[8], u[4][2];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = kin[i];
    scalar_mod_r(k);
    scalar_gs_split(u, k);
    g2_fixed_digit<0>(acc, tab, u[0]);
    g2_fixed_digit<1>(acc, tab, u[1]);
    g2_fixed_digit<2>(acc, tab, u[2]);
    g2_fixed_digit<3>(acc, tab, u[3]);
}
C12381_HDN void g2_fixed_eval_add(g2p& acc, const int32_t* tab, const uint32_t (&kin)[8]) { g2_fixed_eval_digits(acc, tab, kin); }
// acc = [k]Q from the table
C12381_HDN void g2_fixed_eval(g2p& acc, const int32_t* tab, const uint32_t (&kin)[8]) {
    g2_set_inf(acc);
    g2_fixed_eval_digits(acc, tab, kin);
}

// ---- The two groups as the routines that are the same text in both see them: the table entry and the per-lane sum here, the kernel bodies of
// k_fixed.hip and the host routes of c12381_hip.hip through descriptions derived from these.  What differs in substance stays per group
// above: the evaluation (GLV, 2 x 16 windows | GS behind psi, 4 x 8 windows), the subgroup test, the doublings of an entry.
struct fb_g1 {
    using point = g1p; using coord = fp;
    static constexpr int POINT_BYTES = 96, WINDOWS = FB_G1_WINDOWS, ENTRY_DWORDS = FB_G1_DWORDS;
    static C12381_HD void set_inf(g1p& p) { g1_set_inf(p); }
    static C12381_HD void norm1(g1p& r, const g1p& p) { g1_norm1(r, p); }
    static C12381_HD void add(g1p& p, const g1p& q) { g1_add(p, q); }
    static C12381_HD bool in_subgroup(const g1p& p) { return g1_in_subgroup(p); }
    static C12381_HD void eval_add(g1p& acc, const int32_t* tab, const uint32_t (&k)[8]) { g1_fixed_eval_add(acc, tab, k); }
    static C12381_HD void entry(g1p& acc, const g1p& base, uint32_t d, int shift) { g1_fixed_entry(acc, base, d, shift); }
    static C12381_HD void store_affine(int32_t* dst, const g1p& acc) {       // the table keeps (X / Z, Y / Z)
        fp zn, zi, ax, ay;
        fp_norm1(zn, acc.z);
        fp_inv(zi, zn);
        g1p an;
        g1_norm1(an, acc);
        g1_to_affine(ax, ay, an, zi);
        msm_store_pt(dst, ax, ay);
    }
};
struct fb_g2 {
    using point = g2p; using coord = fp2;
    static constexpr int POINT_BYTES = 192, WINDOWS = FB_G2_WINDOWS, ENTRY_DWORDS = FB_G2_DWORDS;
    static C12381_HD void set_inf(g2p& p) { g2_set_inf(p); }
    static C12381_HD void norm1(g2p& r, const g2p& p) { g2_norm1(r, p); }
    static C12381_HD void add(g2p& p, const g2p& q) { g2_add(p, q); }
    static C12381_HD bool in_subgroup(const g2p& p) { return g2_in_subgroup(p); }
    static C12381_HD void eval_add(g2p& acc, const int32_t* tab, const uint32_t (&k)[8]) { g2_fixed_eval_add(acc, tab, k); }
    static C12381_HD void entry(g2p& acc, const g2p& base, uint32_t d, int shift) { g2_fixed_entry(acc, base, d, shift); }
    static C12381_HD void store_affine(int32_t* dst, const g2p& acc) {
        fp2 zn, zi, ax, ay;
        fp2_norm1(zn, acc.z);
        fp2_inv(zi, zn);
        fp2_mul(ax, acc.x, zi); fp2_mul(ay, acc.y, zi);
        fp2_norm1(ax, ax); fp2_norm1(ay, ay);
        fb_store_g2(dst, ax, ay);
    }
};
// entry L = j FB_ENTRIES + d - 1 of the table of `base` (Z = 1): [d 2^(8j)]base, affine.  The table kernels' lanes and the host simulations
// of tests/host_sim/ build their entries with this one routine.
template <class G>
C12381_HD void fixed_table_put(int32_t* dst, const typename G::point& base, size_t L) {
    typename G::point acc;
    G::entry(acc, base, (uint32_t)(L % FB_ENTRIES) + 1u, 8 * (int)(L / FB_ENTRIES));
    G::store_affine(dst, acc);
}
// acc = sum_(i < nb) [k_i]B_i from nb tables `tab_stride` dwords apart, scalar(i, k) handing out the lane's k_i: one accumulator across
// all bases, base by base (the table offset is the same for every lane of a wavefront), up to 32 nb mixed additions and no doubling
template <class G, class SC>
C12381_HD void fixed_eval_sum(typename G::point& acc, const int32_t* tabs, size_t tab_stride, int nb, const SC& scalar) {
    G::set_inf(acc);
#pragma unroll 1
    for (int i = 0; i < nb; ++i) {
        uint32_t k[8];
        scalar(i, k);
        G::eval_add(acc, tabs + (size_t)i * tab_stride, k);
    }
}
// the per-group spellings of the sum, for callers that name the group (the body is fixed_eval_sum alone)
template <class SC> C12381_HD void g1_fixed_eval_sum(g1p& acc, const int32_t* tabs, size_t tab_stride, int nb, const SC& scalar) { fixed_eval_sum<fb_g1>(acc, tabs, tab_stride, nb, scalar); }
template <class SC> C12381_HD void g2_fixed_eval_sum(g2p& acc, const int32_t* tabs, size_t tab_stride, int nb, const SC& scalar) { fixed_eval_sum<fb_g2>(acc, tabs, tab_stride, nb, scalar); }

}  // namespace c12381
