// G1 arithmetic and the per-lane scalar multiplication of the batched path
// (replaces ECP_dbl / ECP_add ecp_BLS12381.cpp:550-588, 750-812, ECP_affine :329,
//  ECP_toOctet :445-488 and PAIR_G1mul + glv pair_BLS12381.cpp:759-810, 876-924 of the
//  reference's vendored MIRACL-core).
//
// Design for CDNA4: one (point, scalar) per lane, homogeneous projective coordinates with
// the Renes–Costello–Batina COMPLETE formulas for a = 0 — no exceptional cases, hence no
// data-dependent branch and no wavefront divergence (P+P, P+(-P), infinity operands and
// zero digits all go through the same instruction stream) — for the MSM, the additions and the fallback; the batched scalar
// multiplication runs Jacobian formulas over a co-Z affine table (g1_scalar_mul_eis).  GLV: k = k0 + k1*x^2 with
// psi = [x^2] : (x,y) -> (beta*x, -y).  psi^2 - psi + 1 = 0, so k0 + k1 psi is an Eisenstein integer: the single product expands it in
// base 8 with digits unit x representative — 44 digits over a table of ELEVEN points, the six units psi^u applied for nothing (x -> beta^u x,
// y -> (-1)^u y) — the top two digits as one seed, then 126 doublings and 42 additions per scalar.  The k-term sums (g1_scalar_mul_sum) and the complete fallback treat the
// halves as two 128-bit integers with signed 5-bit windows over ONE table of 16 multiples of P (125 doublings, 52 additions per term).
// Either table lives in HBM as one contiguous 2816-byte record per lane.
#pragma once
#include "fp.hpp"

namespace c12381 {

struct g1p { fp x, y, z; };      // (X:Y:Z), infinity = (0:1:0)

C12381_HD void g1_set_inf(g1p& p) { fp_zero(p.x); fp_one(p.y); fp_zero(p.z); }
C12381_HD bool g1_is_inf(const g1p& p) { return fp_is_zero(p.z); }
C12381_HD void g1_norm1(g1p& r, const g1p& p) { fp_norm1(r.x, p.x); fp_norm1(r.y, p.y); fp_norm1(r.z, p.z); }
C12381_HD void g1_norm1(g1p& p) { g1_norm1(p, p); }
// r = c ? a : b, the same instruction stream for both
C12381_HD void g1_select(g1p& r, bool c, const g1p& a, const g1p& b) { fp_select(r.x, c, a.x, b.x); fp_select(r.y, c, a.y, b.y); fp_select(r.z, c, a.z, b.z); }
// The result of a lane whose input was rejected: Z = 0 like the point at infinity, but X = 1 (Montgomery) where infinity has X = 0.  The
// kernels that write projective results set it, the finish kernel (k_g1.hip) tells the two apart with g1_is_invalid.
C12381_HD void g1_set_invalid(g1p& p) { fp_one(p.x); fp_zero(p.y); fp_zero(p.z); }
C12381_HD bool g1_is_invalid(const g1p& p) { return fp_is_zero(p.z) && !fp_is_zero(p.x); }

// P = 2P.  6M + 2S with 7 reductions (Y3 is a lazily reduced sum of two products).
// Operand limb bound: <= 2^29.
// Round 4: u = Y^2 - 9b Z^2 leaves the reduction of Y^2 with -3 (3b Z^2) injected (fp_reduce_cols_inj) — normalised, no lazy
// sum and no carry round; Y^2 itself is u + 3 (3b Z^2), used lazily (the lazy form of both formulas: profiles/r04_ab_injection_switches.txt).
C12381_HD void g1_dbl(g1p& p) {
    fp t0, t1, t2, z8, u, y3, x3, z3;
    const int32_t cm3 = fp_opaque_const(-3);
    fp_mul(t1, p.y, p.z);
    fp_sqr(t2, p.z);
    fp_mul_small(t2, t2, 12);                            // 3b Z^2
    fp_sqr_inj(u, p.y, [&](int i, int64_t& acc) { fp_inj(acc, t2, i, cm3); }, C12381_BV(3 * t2.vb), C12381_BV(3 * t2.lb));          // Y^2 - 9b Z^2
    fp_dbl(t0, t2); fp_add(t0, t0, t2); fp_add(t0, t0, u);                                                    // Y^2 = u + 9b Z^2 (limbs < 2^30)
    fp_mul_small(z8, t0, 8);                             // 8 Y^2
    fp_add(y3, t0, t2);
    fp_mul(z3, t1, z8);
    fp_mul2<false>(y3, u, y3, t2, z8);                   // (Y^2 - 9bZ^2)(Y^2 + 3bZ^2) + 3bZ^2 * 8Y^2
    fp_mul(t1, p.x, p.y);
    fp_mul(x3, u, t1);
    fp_dbl(x3, x3);
    p.x = x3; p.y = y3; p.z = z3;
}

// P = P + Q (complete).  12 products, 9 reductions.
// Operand limb bounds: P <= 2^29, Q <= 2^28 (+ carry slack): table entries are stored normalised.
C12381_HD void g1_add(g1p& p, const g1p& q) {
    fp t0, t1, t2, t3, t4, x3, y3, z3;
    fp_mul(t0, p.x, q.x);
    fp_mul(t1, p.y, q.y);
    fp_mul(t2, p.z, q.z);
    {   // the Karatsuba corrections -t0 - t1, -t1 - t2 ride in the reductions: t3, t4 normalised without a lazy sum or a carry round
        const int32_t cm1 = fp_opaque_const(-1);
        fp sa, sb;
        fp_add(sa, p.x, p.y); fp_add(sb, q.x, q.y);
        fp_mul_inj(t3, sa, sb, [&](int i, int64_t& acc) { fp_inj(acc, t0, i, cm1); fp_inj(acc, t1, i, cm1); }, C12381_BV(t0.vb + t1.vb), C12381_BV(t0.lb + t1.lb));
        fp_add(sa, p.y, p.z); fp_add(sb, q.y, q.z);
        fp_mul_inj(t4, sa, sb, [&](int i, int64_t& acc) { fp_inj(acc, t1, i, cm1); fp_inj(acc, t2, i, cm1); }, C12381_BV(t1.vb + t2.vb), C12381_BV(t1.lb + t2.lb));
    }
    fp_add(x3, p.x, p.z); fp_add(y3, q.x, q.z); fp_mul(x3, x3, y3);
    fp_add(y3, t0, t2); fp_sub(y3, x3, y3);
    fp_mul_small(t0, t0, 3);
    fp_mul_small(t2, t2, 12);
    fp_add(z3, t1, t2); fp_sub(t1, t1, t2);
    fp_mul_small(y3, y3, 12);
    fp_mul2<true>(p.x, t3, t1, y3, t4);                  // X3 = t3*t1 - y3*t4
    fp_mul2<false>(p.y, y3, t0, t1, z3);                 // Y3 = y3*t0 + t1*z3
    fp_mul2<false>(p.z, z3, t4, t0, t3);                 // Z3 = z3*t4 + t0*t3
}

// (X:Y:Z) -> (beta*X : -Y : Z) = [x^2](X:Y:Z)
C12381_HD void g1_endo_x2(g1p& r, const g1p& p) {
    fp beta;
    fp_set_const(beta, FP_BETA_A);
    fp_mul(r.x, p.x, beta);
    fp_neg(r.y, p.y);
    r.z = p.z;
}

// ------------------------------------------------------------------ Jacobian a = 0 (incomplete: the scalar multiplication's fast path)
// (X:Y:Z) stands for (X/Z^2, Y/Z^3).  None of these formulas reads the curve constant b, so they hold unchanged on every curve
// y^2 = x^3 + b', in particular on the isomorphic curve of a co-Z table (g1_scalar_mul).  Z = 0 is the point at infinity, and it
// is absorbing: a doubling gives Z3 = 2YZ, a mixed addition Z3 = Z1 H.
struct g1j { fp x, y, z; };

// P = 2P (dbl-2009-l, rearranged): 3M + 3S plus one square's columns, 6 reductions; the linear term -2D rides in the reduction of E^2
// (fp_sqr_inj), so every output coordinate is normalised.  Operand limb bound: <= 2^28 + slack (reduction outputs).
// C = Y^4 is not formed: it only ever entered linearly (D/2 = (X + B)^2 - A - C and Y3 = E (D - X3) - 8C), and a value that is never
// multiplied again needs no reduction of its own.  With G = 2Y^2 = Y (2Y) — 2Y is there for Z3 — D/2 = X G is a plain product and
// 8C = 2 G^2, whose square columns ride in the reduction of Y3 (fp_mul_msqr2; 8 B^2 itself would not fit the columns beside
// E (D - X3)).  Same values: X3 = 9X^4 - 8XY^2, Y3 = 3X^2 (4XY^2 - X3) - 8Y^4, Z3 = 2YZ.  g1j_dblu keeps C: there 8C is an output.
// G itself is a square times two and is scanned as one (fp_sqr2: 105 column products, not the 196 of Y (2Y); the same limbs): of the six
// products three are squares' scans (A, G, E^2) and three general (Z3, D/2, E (D - X3)).
C12381_HD void g1j_dbl(g1j& p) {
    fp a, g, d, e, x3, y3, z3, y2;
    const int32_t cm4 = fp_opaque_const(-4);
    fp_raw_dbl(y2, p.y);
    fp_mul(z3, y2, p.z);                                 // Z3 = 2YZ
    fp_sqr(a, p.x);                                      // A = X^2
    fp_sqr2(g, p.y);                                     // G = 2Y^2, the limbs of Y (2Y) from a square's columns
    fp_mul(d, p.x, g);                                   // D/2 = 2XY^2
    fp_mul_small(e, a, 3);                               // E = 3A
    fp_sqr_inj(x3, e, [&](int i, int64_t& acc) { fp_inj(acc, d, i, cm4); }, C12381_BV(4 * d.vb), C12381_BV(4 * d.lb));   // X3 = E^2 - 2D
    fp_raw_dbl(d, d);
    fp_sub(d, d, x3);
    fp_mul_msqr2(y3, e, d, g);                           // Y3 = E (D - X3) - 2G^2
    p.x = x3; p.y = y3; p.z = z3;
}

// r = p + (x2, y2) with (x2, y2) affine on the same curve (madd-2004-hmv): 6M + 3S and one lazily reduced pair, 10 reductions.
// Exceptional (Z3 = 0) when p = +-(x2, y2) or p is infinity; the caller selects around d = 0 and an accumulator at infinity.
C12381_HD void g1j_madd(g1j& r, const g1j& p, const fp& x2, const fp& y2) {
    fp zz, zzz, u2, s2, h, s, hh, hhh, v, x3, y3, z3, vx;
    const int32_t cm1 = fp_opaque_const(-1), cm2 = fp_opaque_const(-2);
    fp_sqr(zz, p.z);
    fp_mul(u2, x2, zz);                                  // U2 = x2 Z1^2
    fp_mul(zzz, p.z, zz);
    fp_mul(s2, y2, zzz);                                 // S2 = y2 Z1^3
    fp_sub(h, u2, p.x);                                  // H = U2 - X1
    fp_sub(s, s2, p.y);                                  // s = S2 - Y1
    fp_mul(z3, p.z, h);                                  // Z3 = Z1 H
    fp_sqr(hh, h);
    fp_mul(hhh, h, hh);
    fp_mul(v, p.x, hh);                                  // V = X1 H^2
    fp_sqr_inj(x3, s, [&](int i, int64_t& acc) { fp_inj(acc, hhh, i, cm1); fp_inj(acc, v, i, cm2); },
               C12381_BV(hhh.vb + 2 * v.vb), C12381_BV(hhh.lb + 2 * v.lb));         // X3 = s^2 - H^3 - 2V
    fp_sub(vx, v, x3);
    fp_mul2<true>(y3, s, vx, p.y, hhh);                  // Y3 = s (V - X3) - Y1 H^3
    r.x = x3; r.y = y3; r.z = z3;
}

// Co-Z steps of the table (Meloni): points that share one Z are passed without it.
// DBLU: (x, y) affine -> 2P = (x2, y2) and P = (x1, y1), both with Z = 2y.  1M + 5S.
C12381_HD void g1j_dblu(fp& x2, fp& y2, fp& x1, fp& y1, const fp& x, const fp& y) {
    fp a, b, c, d, e, xb, dd;
    const int32_t cm1 = fp_opaque_const(-1), cm4 = fp_opaque_const(-4), cm8 = fp_opaque_const(-8);
    fp_sqr(a, x);
    fp_sqr(b, y);
    fp_sqr(c, b);
    fp_add(xb, x, b);
    fp_sqr_inj(d, xb, [&](int i, int64_t& acc) { fp_inj(acc, a, i, cm1); fp_inj(acc, c, i, cm1); },
               C12381_BV(a.vb + c.vb), C12381_BV(a.lb + c.lb));                       // D/2 = 2 x y^2
    fp_mul_small(e, a, 3);
    fp_sqr_inj(x2, e, [&](int i, int64_t& acc) { fp_inj(acc, d, i, cm4); }, C12381_BV(4 * d.vb), C12381_BV(4 * d.lb));
    fp_raw_dbl(dd, d);
    fp_sub(dd, dd, x2);
    fp_mul_inj(y2, e, dd, [&](int i, int64_t& acc) { fp_inj(acc, c, i, cm8); }, C12381_BV(8 * c.vb), C12381_BV(8 * c.lb));
    fp_mul_small(x1, d, 2);                              // x (2y)^2 = D
    fp_mul_small(y1, c, 8);                              // y (2y)^3 = 8C
}
// ZADDU: P = (x1, y1), Q = (x2, y2) on one Z  ->  P + Q = (x3, y3) and P = (x1, y1) both on Z' = Z h, h = x1 - x2 returned
// lazily.  4M + 2S (Z' itself is not formed).  h = 0 (Q = +-P) gives Z' = 0.
C12381_HD void g1j_zaddu(fp& x3, fp& y3, fp& x1, fp& y1, fp& h, const fp& x2, const fp& y2) {
    fp c, w1, w2, sd, dw, a1, wx;
    const int32_t cm1 = fp_opaque_const(-1);
    fp_sub(h, x1, x2);
    fp_sqr(c, h);
    fp_mul(w1, x1, c);                                   // W1 = x1 h^2
    fp_mul(w2, x2, c);
    fp_sub(sd, y1, y2);
    fp_sub(dw, w1, w2);
    fp_mul(a1, y1, dw);                                  // A1 = y1 h^3
    fp_sqr_inj(x3, sd, [&](int i, int64_t& acc) { fp_inj(acc, w1, i, cm1); fp_inj(acc, w2, i, cm1); },
               C12381_BV(w1.vb + w2.vb), C12381_BV(w1.lb + w2.lb));                 // X3 = (y1 - y2)^2 - W1 - W2
    fp_sub(wx, w1, x3);
    fp_mul_inj(y3, sd, wx, [&](int i, int64_t& acc) { fp_inj(acc, a1, i, cm1); }, C12381_BV(a1.vb), C12381_BV(a1.lb));  // Y3 = (y1 - y2)(W1 - X3) - A1
    x1 = w1; y1 = a1;
}

// ------------------------------------------------------------------ scalars
// k (8 little-endian 32-bit words, any value < 2^256) -> k mod r.  r > 2^254, so at most
// three subtractions (the reference reduces first too: pair_BLS12381.cpp:879-881).
C12381_HD void scalar_mod_r(uint32_t (&k)[8]) {
#pragma unroll 1
    for (int round = 0; round < 3; ++round) {
        uint32_t d[8];
        uint64_t bw = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint64_t t = (uint64_t)k[i] - ORDER_R[i] - bw;
            d[i] = (uint32_t)t;
            bw = (t >> 32) & 1;
        }
        const bool ge = bw == 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) k[i] = ge ? d[i] : k[i];
    }
}
// k < r  ->  k = k0 + k1 * x^2 with 0 <= k0 < x^2 < 2^128 and k1 < 2^128  (replaces glv() pair_BLS12381.cpp:793-805,
// whose u1 = r - (e div x^2) belongs to the opposite sign convention of the endomorphism).
// Barrett division by the 128-bit constant x^2 (top bit set): q^ = floor(floor(k / 2^127) * mu / 2^129) with
// mu = floor(2^256 / x^2) satisfies q - 2 <= q^ <= q for k < 2^256, so two conditional subtractions finish it:
// ~60 multiply-adds instead of a 256-step restoring division (which was more than half of the MSM preparation kernel).
C12381_HD void scalar_glv_split(uint32_t (&k0)[4], uint32_t (&k1)[4], const uint32_t (&k)[8]) {
    uint32_t a[5], prod[10];
#pragma unroll
    for (int i = 0; i < 5; ++i) a[i] = (k[i + 3] >> 31) | (i + 4 < 8 ? k[i + 4] << 1 : 0u);
#pragma unroll
    for (int i = 0; i < 10; ++i) prod[i] = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint64_t t = (uint64_t)a[i] * GLV_MU[j] + prod[i + j] + carry;
            prod[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        prod[i + 5] = (uint32_t)carry;
    }
    uint32_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (prod[4 + i] >> 1) | (prod[5 + i] << 31);
    // rem = k - q * x^2, exact in 160 bits (0 <= rem < 3 x^2)
    uint32_t qd[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < 5) {
                const uint64_t t = (uint64_t)q[i] * GLV_X2[j] + qd[i + j] + carry;
                qd[i + j] = (uint32_t)t;
                carry = t >> 32;
            }
        }
        if (i + 4 < 5) qd[i + 4] = (uint32_t)carry;
    }
    uint32_t rem[5];
    {
        uint64_t bw = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const uint64_t t = (uint64_t)k[i] - qd[i] - bw;
            rem[i] = (uint32_t)t;
            bw = (t >> 32) & 1;
        }
    }
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        uint32_t d[5];
        uint64_t bw = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const uint64_t t = (uint64_t)rem[i] - (i < 4 ? GLV_X2[i] : 0u) - bw;
            d[i] = (uint32_t)t;
            bw = (t >> 32) & 1;
        }
        const bool ge = bw == 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) rem[i] = ge ? d[i] : rem[i];
        uint64_t c = ge ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) { c += q[i]; q[i] = (uint32_t)c; c >>= 32; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { k0[i] = rem[i]; k1[i] = q[i]; }
}

// ------------------------------------------------------------------ limb-major SoA access
// element `idx` of an array of fp stored as limb[NL][stride]
C12381_HD void soa_store_fp(int32_t* base, size_t stride, size_t idx, const fp& a) {
#pragma unroll
    for (int i = 0; i < NL; ++i) base[(size_t)i * stride + idx] = a.l[i];
}
C12381_HD void soa_load_fp(fp& a, const int32_t* base, size_t stride, size_t idx) {
#pragma unroll
    for (int i = 0; i < NL; ++i) a.l[i] = base[(size_t)i * stride + idx];
    C12381_BOUNDS(a.lb = 268435456.0 + 8.0; a.vb = 4.0; check_actual(a, "soa_load_fp");)
}
C12381_HD void soa_store_g1(int32_t* base, size_t stride, size_t idx, const g1p& p) {
    soa_store_fp(base, stride, idx, p.x);
    soa_store_fp(base + (size_t)NL * stride, stride, idx, p.y);
    soa_store_fp(base + (size_t)2 * NL * stride, stride, idx, p.z);
}
C12381_HD void soa_load_g1(g1p& p, const int32_t* base, size_t stride, size_t idx) {
    soa_load_fp(p.x, base, stride, idx);
    soa_load_fp(p.y, base + (size_t)NL * stride, stride, idx);
    soa_load_fp(p.z, base + (size_t)2 * NL * stride, stride, idx);
}

// ------------------------------------------------------------------ per-lane window table
// Signed 5-bit windows: entries 1..16 of multiples of P, each entry X|Y|Z = 42 dwords padded to 44 (176 B,
// eleven 16-byte accesses).  A lane's whole table is one contiguous 2816-byte record, so a gather of one
// entry touches 176 consecutive bytes of HBM instead of 42 scattered dwords (the limb-major layout of the
// first version moved ~16x the algorithmic bytes: profiles/r01_pmc_summary_before_table_fix.txt).
// Per scalar multiplication: 8 + 125 doublings and 7 + 52 additions.
constexpr int G1_WIN = 5;                               // against 4-bit windows on MI355X (profiles/r02_ab_g1_window5.txt): 3.5 % faster
constexpr int G1_TAB = 1 << (G1_WIN - 1);              // entries 1..16
constexpr int G1_WINDOWS = 26;                          // 26 biased fields cover 130 bits
constexpr int G1_ENT_DWORDS = 44;
constexpr int G1_TAB_DWORDS = G1_TAB * G1_ENT_DWORDS;  // 704 dwords = 2816 B per lane
struct alignas(16) q4 { int32_t v[4]; };
struct alignas(8) d2 { int32_t v[2]; };

// 16-byte words [Q0, Q0 + NQ) of a record between memory and dwords [4 Q0, 4 (Q0 + NQ)) of w.  P = pointer to q4, in whatever address
// space the caller knows the record to live in.
template <int Q0, int NQ, class P>
C12381_HD void rec_store_q4(P dst, const int32_t* w) {
#pragma unroll
    for (int i = Q0; i < Q0 + NQ; ++i) { q4 t; t.v[0] = w[4 * i]; t.v[1] = w[4 * i + 1]; t.v[2] = w[4 * i + 2]; t.v[3] = w[4 * i + 3]; dst[i] = t; }
}
template <int Q0, int NQ, class P>
C12381_HD void rec_load_q4(int32_t* w, P src) {
#pragma unroll
    for (int i = Q0; i < Q0 + NQ; ++i) { q4 t = src[i]; w[4 * i] = t.v[0]; w[4 * i + 1] = t.v[1]; w[4 * i + 2] = t.v[2]; w[4 * i + 3] = t.v[3]; }
}

// A table record holds three fields: X | Y | Z of the complete path, x | y | beta x (or X_j | Y_j | h_j while the table is built) of the
// co-Z path.  Stores write the two pad dwords as zero, or (KEEP_PADS) leave them as they are: the co-Z tables keep Z_T and digit words there.
constexpr double G1_REC_LB = 268435456.0 + 8.0;
template <bool KEEP_PADS = false>
C12381_HD void tab_store_fields(int32_t* ent, const fp& a, const fp& b, const fp& c) {
    int32_t w[G1_ENT_DWORDS];
#pragma unroll
    for (int i = 0; i < NL; ++i) { w[i] = a.l[i]; w[NL + i] = b.l[i]; w[2 * NL + i] = c.l[i]; }
    w[42] = 0; w[43] = 0;
    rec_store_q4<0, G1_ENT_DWORDS / 4 - (KEEP_PADS ? 1 : 0)>(reinterpret_cast<q4*>(ent), w);
    if (KEEP_PADS) { d2 t; t.v[0] = w[40]; t.v[1] = w[41]; *reinterpret_cast<d2*>(ent + 40) = t; }
}
template <bool KEEP_PADS = false>
C12381_HD void tab_store_rec(int32_t* ent, const fp& a, const fp& b, const fp& c, double vb_cap) {
    (void)vb_cap;
    C12381_BOUNDS(for (const fp* e : {&a, &b, &c}) { if (e->vb > vb_cap) bounds_fail("tab_store_rec value bound", e->vb, vb_cap);
                                                      if (e->lb > G1_REC_LB) bounds_fail("tab_store_rec limb bound", e->lb, G1_REC_LB); })
    tab_store_fields<KEEP_PADS>(ent, a, b, c);
}
// dwords [4 q0, 4 q0 + 4 nq) of a record into w
template <int Q0, int NQ>
C12381_HD void tab_load_q4(int32_t (&w)[G1_ENT_DWORDS], const int32_t* ent) { rec_load_q4<Q0, NQ>(w, reinterpret_cast<const q4*>(ent)); }
C12381_HD void rec_field(fp& a, const int32_t (&w)[G1_ENT_DWORDS], int off, double vb_cap) {
#pragma unroll
    for (int i = 0; i < NL; ++i) a.l[i] = w[off + i];
    (void)vb_cap;
    C12381_BOUNDS(a.lb = G1_REC_LB; a.vb = vb_cap; check_actual(a, "rec_field");)
}
C12381_HD void tab_load_rec(fp& a, fp& b, fp& c, const int32_t* ent, double vb_cap) {
    int32_t w[G1_ENT_DWORDS];
    tab_load_q4<0, G1_ENT_DWORDS / 4>(w, ent);
    rec_field(a, w, 0, vb_cap); rec_field(b, w, NL, vb_cap); rec_field(c, w, 2 * NL, vb_cap);
}
// a projective point as a record (the complete path, the MSM's buckets, g2h.hpp)
C12381_HD void tab_store_g1(int32_t* ent, const g1p& p) { tab_store_fields(ent, p.x, p.y, p.z); }
C12381_HD void tab_load_g1(g1p& p, const int32_t* ent) { tab_load_rec(p.x, p.y, p.z, ent, 4.0); }

// 5-bit windows of k' = k + sum_w 16 * 32^w (w < 26; k < 2^128, so k' < 2^130 and there is no carry window): the signed digit of window w
// is d = field - 16 in [-16, 15], and Sum_w d_w 32^w = k.
constexpr uint32_t glv_bias_word5(int i) {
    uint32_t v = 0;
    for (int w = 0; w < 26; ++w) { const int bit = 5 * w + 4; if ((bit >> 5) == i) v |= 1u << (bit & 31); }
    return v;
}
C12381_HD int glv_digit(const uint32_t (&kb)[5], int w) {
    const int bit = 5 * w, word = bit >> 5, sh = bit & 31;
    uint32_t v = kb[word] >> sh;
    if (sh > 27) v |= kb[word + 1] << (32 - sh);
    return (int)(v & 31u) - 16;
}
C12381_HD void glv_bias(uint32_t (&kb)[5], const uint32_t (&k)[4]) {
    constexpr uint32_t B[5] = {glv_bias_word5(0), glv_bias_word5(1), glv_bias_word5(2), glv_bias_word5(3), glv_bias_word5(4)};
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { c += (uint64_t)k[i] + B[i]; kb[i] = (uint32_t)c; c >>= 32; }
    kb[4] = (uint32_t)c + B[4];
}
// scalar words (any value < 2^256) -> the biased digit strings of the two GLV halves of k mod r.  `zero` (a term that takes no part:
// g1_scalar_mul_sum) replaces both halves by 0, i.e. every digit by 0.
C12381_HD void glv_scalar_digits(uint32_t (&kb0)[5], uint32_t (&kb1)[5], const uint32_t (&kin)[8], bool zero = false) {
    uint32_t k[8], k0[4], k1[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = kin[i];
    scalar_mod_r(k);
    scalar_glv_split(k0, k1, k);
#pragma unroll
    for (int i = 0; i < 4; ++i) { k0[i] = zero ? 0u : k0[i]; k1[i] = zero ? 0u : k1[i]; }
    glv_bias(kb0, k0);
    glv_bias(kb1, k1);
}
// the table record a digit selects (|d| = 0 reads entry 1 and is replaced by the point at infinity afterwards)
C12381_HD const int32_t* g1_digit_entry(const int32_t* lane_tab, int d) {
    const int mag = d < 0 ? -d : d;
    return lane_tab + ((mag == 0 ? 1 : mag) - 1) * G1_ENT_DWORDS;
}
// (round 4, profiles/r04_ab_g1_prefetch.txt) In the window loops the record of an addition is requested one operation ahead — a window's
// first before its doublings, every other one before the addition in front of its own — instead of at the head of the addition that needs
// it, where the whole latency of the gather (a 176-byte record somewhere in a slab of gigabytes) was exposed twice per window.  This fence
// keeps the request there: nothing is scheduled across it.
C12381_HD void g1_sched_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}
// q = sign(d) * T[|d|], or its image under the endomorphism; d == 0 gives the point at infinity (same instruction stream)
C12381_HD void g1_digit_fix(g1p& r, g1p q, int d, bool endo);
C12381_HD void g1_digit_point(g1p& r, const int32_t* lane_tab, int d, bool endo) {
    g1p q;
    tab_load_g1(q, g1_digit_entry(lane_tab, d));
    g1_digit_fix(r, q, d, endo);
}
C12381_HD void g1_digit_fix(g1p& r, g1p q, int d, bool endo) {
    const int mag = d < 0 ? -d : d;
    fp ny;
    g1p inf;
    fp_neg(ny, q.y);
    fp_select(q.y, d < 0, ny, q.y);
    g1_set_inf(inf);
    g1_select(q, mag == 0, inf, q);
    C12381_BOUNDS(q.x.lb = q.y.lb = q.z.lb = 268435456.0 + 8.0;)
    if (endo) g1_endo_x2(r, q); else r = q;          // compile-time constant at every call site
}
// acc += sign(d) * T[|d|]
C12381_HD void g1_add_digit(g1p& acc, const int32_t* lane_tab, int d, bool endo) {
    g1p e;
    g1_digit_point(e, lane_tab, d, endo);
    g1_add(acc, e);
}

// p <- [|x|]p, plain double-and-add over the 64-bit curve parameter (weight 6)
C12381_HDN void g1_mul_absx(g1p& p) {
    g1p base, acc;
    g1_norm1(base, p);
    acc = base;
#pragma unroll 1
    for (int i = 62; i >= 0; --i) {
        g1_dbl(acc);
        if ((BLS_X_W[i >> 5] >> (i & 31)) & 1u) g1_add(acc, base);
    }
    p = acc;
}
// The reference's glv() (pair_BLS12381.cpp:793-805) returns u1 = r - (k div x^2), and PAIR_G1mul's sign minimisation
// (:899-906) maps that back to k div x^2 — except when k div x^2 == 0: then u1 stays r and ECP_mul2 adds [r]phi(P),
// phi(P) = (beta x, y).  That term is the point at infinity for P in G1 and a point of the cofactor part otherwise.
// Reproduced (lanes with k < x^2 only; see scalar_below_x2) so results agree with `multiply` on every curve point.
// phi(P) is in G1 iff phi(phi(P)) = [-x^2]phi(P); off the subgroup [r]Q = [x^2]([x^2]Q) - [x^2]Q + Q  (r = x^4 - x^2 + 1).
C12381_HDN void g1_glv_small_scalar_term(g1p& acc, const g1p& base) {
    fp beta;
    fp_set_const(beta, FP_BETA_A);
    g1p q, s1, t;
    fp_mul(q.x, base.x, beta); q.y = base.y; q.z = base.z;            // phi(P)
    g1_norm1(q, q);
    s1 = q;
    g1_mul_absx(s1); g1_mul_absx(s1);                                  // [x^2]phi(P)
    g1_norm1(s1, s1);
    fp_mul(t.x, q.x, beta); t.y = q.y; t.z = q.z;                      // phi(phi(P))
    g1_norm1(t, t);
    {
        g1p u = s1;
        g1_add(u, t);
        if (g1_is_inf(u)) return;                                      // P in G1: the extra term vanishes
    }
    g1p s2 = s1;
    g1_mul_absx(s2); g1_mul_absx(s2);                                  // [x^4]phi(P)
    fp_neg(t.y, s1.y); t.x = s1.x; t.z = s1.z;
    g1_norm1(t, t);
    g1_add(s2, t);
    g1_norm1(s2, s2);
    g1_add(s2, q);
    g1_norm1(s2, s2);
    g1_norm1(acc, acc);
    g1_add(acc, s2);
}

// [k]P for an AFFINE input point (x, y) or infinity with the complete formulas: no exceptional case.  `lane_tab` = this lane's table
// record (G1_TAB_DWORDS).  Out of line: g1_scalar_mul_eis and g1_scalar_mul fall back to it for the rare lanes its incomplete formulas cannot serve, and
// the main loop's register allocation does not pay for the second copy.
C12381_HDN void g1_scalar_mul_complete(g1p& acc, const fp& px, const fp& py, bool p_is_inf, const uint32_t (&kin)[8], int32_t* lane_tab) {
    uint32_t kb0[5], kb1[5];
    glv_scalar_digits(kb0, kb1, kin);

    // table T[j] = j*P, j = 1..G1_TAB, stored normalised (limb bound 2^28 + slack)
    g1p base, t;
    base.x = px; base.y = py; fp_one(base.z);
    {   // infinity input: use (0:1:0) as the base so every multiple is infinity
        g1p inf;
        g1_set_inf(inf);
        g1_select(base, p_is_inf, inf, base);
    }
    tab_store_g1(lane_tab, base);                               // T[1]
    t = base;
    g1_dbl(t);
    g1_norm1(t);
    tab_store_g1(lane_tab + G1_ENT_DWORDS, t);                  // T[2]
    // even multiples by doubling the entry half as large (8 products + 7 reductions against 12 + 9 for an addition; the entry comes
    // back from the lane's own record), odd ones by adding P to the previous entry: 8 doublings + 7 additions for 16 entries
#pragma unroll 1
    for (int j = 3; j <= G1_TAB; ++j) {
        if ((j & 1) == 0) {                                     // wave-uniform
            tab_load_g1(t, lane_tab + (j / 2 - 1) * G1_ENT_DWORDS);
            g1_dbl(t);
        } else {
            g1_add(t, base);
        }
        g1_norm1(t);
        tab_store_g1(lane_tab + (j - 1) * G1_ENT_DWORDS, t);
    }

    // the top window starts the accumulator with its first digit's entry (an addition to the point at infinity would compute the same
    // point): 51 + 7 additions in all
    g1_digit_point(acc, lane_tab, glv_digit(kb0, G1_WINDOWS - 1), false);
    g1_norm1(acc);
    g1_add_digit(acc, lane_tab, glv_digit(kb1, G1_WINDOWS - 1), true);
    // records requested one operation ahead (g1_sched_fence): 44 registers across the doublings
#pragma unroll 1
    for (int w = G1_WINDOWS - 2; w >= 0; --w) {
        const int d0 = glv_digit(kb0, w), d1 = glv_digit(kb1, w);
        g1p q0, q1, e;
        tab_load_g1(q0, g1_digit_entry(lane_tab, d0));
        g1_sched_fence();                                // the loads stay in front of the doublings
        // a loop, not G1_WIN copies: this function is called, and a loop body beyond the reach of s_cbranch (+-128 KiB) gets long
        // branches whose expansion (ROCm 7.2 clang) takes s[30:31], the return address, so the call never came back and the lane
        // ran wild (an illegal memory access on the first fallback lane)
#pragma unroll 1
        for (int j = 0; j < G1_WIN; ++j) g1_dbl(acc);
        tab_load_g1(q1, g1_digit_entry(lane_tab, d1));
        g1_sched_fence();
        g1_digit_fix(e, q0, d0, false);
        g1_add(acc, e);
        g1_digit_fix(e, q1, d1, true);
        g1_add(acc, e);
    }
}

// ------------------------------------------------------------------ co-Z affine table of 16 multiples (the k-term sums: g1_scalar_mul_sum)
// Record of entry j: x | y | beta x | 2 pad dwords (44 dwords, as the complete path's X | Y | Z).  The pads of entries 1..7 carry the
// 14 limbs of Z_T, the shared Z of the table.  While the table is built, entry j holds (X_j, Y_j, h_j) instead: jP on its own Z and the
// factor h_j that carries Z_j to Z_(j+1).
// what an addition reads: x and y (dwords 0..27), or y and beta x (dwords 12..43)
C12381_HD void tab_load_xy(fp& x, fp& y, const int32_t* ent) {
    int32_t w[G1_ENT_DWORDS];
    tab_load_q4<0, 7>(w, ent);
    rec_field(x, w, 0, 4.0); rec_field(y, w, NL, 4.0);
}
C12381_HD void tab_load_ybx(fp& y, fp& bx, const int32_t* ent) {
    int32_t w[G1_ENT_DWORDS];
    tab_load_q4<3, 8>(w, ent);
    rec_field(y, w, NL, 4.0); rec_field(bx, w, 2 * NL, 4.0);
}
// the same for the entry digit d selects, requested here and not later (g1_sched_fence)
C12381_HD void tab_fetch_xy(fp& x, fp& y, const int32_t* lane_tab, int d) { tab_load_xy(x, y, g1_digit_entry(lane_tab, d)); g1_sched_fence(); }
C12381_HD void tab_fetch_ybx(fp& y, fp& bx, const int32_t* lane_tab, int d) { tab_load_ybx(y, bx, g1_digit_entry(lane_tab, d)); g1_sched_fence(); }
C12381_HD void tab_store_zt(int32_t* lane_tab, const fp& zt) {
#pragma unroll
    for (int j = 0; j < NL / 2; ++j) { d2 t; t.v[0] = zt.l[2 * j]; t.v[1] = zt.l[2 * j + 1]; *reinterpret_cast<d2*>(lane_tab + j * G1_ENT_DWORDS + 42) = t; }
}
C12381_HD void tab_load_zt(fp& zt, const int32_t* lane_tab) {
#pragma unroll
    for (int j = 0; j < NL / 2; ++j) { const d2 t = *reinterpret_cast<const d2*>(lane_tab + j * G1_ENT_DWORDS + 42); zt.l[2 * j] = t.v[0]; zt.l[2 * j + 1] = t.v[1]; }
    C12381_BOUNDS(zt.lb = G1_REC_LB; zt.vb = 4.0; check_actual(zt, "tab_load_zt");)
}

// Forward co-Z pass over the table of P = (px, py): DBLU and fourteen ZADDUs.  Leaves entries 2..15 as (X_j, Y_j, h_j), entries 1 and 16
// finished on Z_16 = Z_T = 2y h_2 ... h_15.  `on_h(j, h_j)` sees every factor as it is stored.
template <class OnH>
C12381_HD void g1_coz_forward(int32_t* lane_tab, const fp& px, const fp& py, const fp& beta, const OnH& on_h) {
    fp x1, y1, xj, yj, xn, yn, h, hn, bx;
    g1j_dblu(xj, yj, x1, y1, px, py);                           // 2P and P on Z_2 = 2y
#pragma unroll 1
    for (int j = 2; j < G1_TAB; ++j) {
        g1j_zaddu(xn, yn, x1, y1, h, xj, yj);                   // (j+1)P and P on Z_(j+1) = Z_j h_j
        fp_norm1(hn, h);
        tab_store_rec(lane_tab + (j - 1) * G1_ENT_DWORDS, xj, yj, hn, 32.0);
        on_h(j, hn);
        xj = xn; yj = yn;
    }
    fp_mul(bx, xj, beta);
    tab_store_rec(lane_tab + (G1_TAB - 1) * G1_ENT_DWORDS, xj, yj, bx, 4.0);
    fp_mul(bx, x1, beta);
    tab_store_rec(lane_tab, x1, y1, bx, 4.0);
}
// One step of the backward pass: mu <- mu h_j (mu = h_j where the chain starts: `first`, wave-uniform), and entry j = (X_j, Y_j, h_j)
// becomes (mu^2 X_j, mu^3 Y_j, beta mu^2 X_j), the point on Z_j mu.
template <bool KEEP_PADS>
C12381_HD void g1_coz_backward(int32_t* ent, fp& mu, bool first, const fp& beta) {
    fp m2, m3, x, y, h, bx;
    tab_load_rec(x, y, h, ent, 32.0);
    if (first) mu = h; else fp_mul(mu, mu, h);
    fp_sqr(m2, mu);
    fp_mul(m3, m2, mu);
    fp_mul(x, x, m2);
    fp_mul(y, y, m3);
    fp_mul(bx, x, beta);
    tab_store_rec<KEEP_PADS>(ent, x, y, bx, 4.0);
}
// the G1_WIN doublings of one window
C12381_HD void g1j_dbl_window(g1j& a) { g1j_dbl(a); g1j_dbl(a); g1j_dbl(a); g1j_dbl(a); g1j_dbl(a); }

// acc += sign(d) T[|d|], or its image (beta x, -y) under the endomorphism, given the entry's x (beta x) and y.  d = 0 keeps acc (the
// addition with entry 1 is computed and dropped); an accumulator at infinity (acc_inf) takes the looked-up point with Z = 1.
C12381_HD void g1j_add_signed(g1j& acc, bool& acc_inf, const fp& x, const fp& y, bool neg, bool keep);
C12381_HD void g1j_add_digit(g1j& acc, bool& acc_inf, const fp& x, const fp& y, int d, bool endo) {
    g1j_add_signed(acc, acc_inf, x, y, (d < 0) != endo, d == 0);
}
// acc += (x, -y) if neg, else (x, y); `keep` keeps acc (the addition is computed and dropped)
C12381_HD void g1j_add_signed(g1j& acc, bool& acc_inf, const fp& x, const fp& y, bool neg, bool keep) {
    fp ny, ys, one;
    fp_neg(ny, y);
    fp_select(ys, neg, ny, y);
    g1j r;
    g1j_madd(r, acc, x, ys);
    fp_one(one);
    fp_select(r.x, acc_inf, x, r.x); fp_select(r.y, acc_inf, ys, r.y); fp_select(r.z, acc_inf, one, r.z);
    fp_select(acc.x, keep, acc.x, r.x); fp_select(acc.y, keep, acc.y, r.y); fp_select(acc.z, keep, acc.z, r.z);
    acc_inf = acc_inf && keep;
}
// The end of the loop: a on E' (Z = zc, the shared Z of the table or tables) back to E and to homogeneous coordinates, (X Z : Y : Z^3) with
// Z = Z_a zc; the point at infinity where `inf`.  Returns true for an exceptional lane: Z = 0 mod p although the result is not infinity.
C12381_HD bool g1_coz_finish(g1p& acc, const g1j& a, const fp& zc, bool inf) {
    fp z, z2;
    fp_mul(z, a.z, zc);
    const bool exc = !inf && fp_is_zero(z);
    fp_sqr(z2, z);
    fp_mul(acc.x, a.x, z);
    acc.y = a.y;
    fp_mul(acc.z, z2, z);
    g1p o;
    g1_set_inf(o);
    g1_select(acc, inf, o, acc);
    return exc;
}

// The single product over the 16-entry table: g1_scalar_mul_sum<K>'s schedule for one term, in the form the sum grew from.  The kernels
// multiply with g1_scalar_mul_eis below; this form stays as the plain statement of the 5-bit schedule, run lane by lane under the bounds
// checker with its complete-path lanes predicted (tests/host_sim/g1_coz.cpp, tests/g1_torsion.py).
// [k]P for an AFFINE input point (x, y) or infinity, result in homogeneous coordinates.  `lane_tab` = this lane's table record
// (G1_TAB_DWORDS).  Returns true for a lane that took the complete path.
// Jacobian doublings and mixed additions over an affine table: a table whose entries share one Jacobian Z = Z_T is affine on the
// isomorphic curve E': y^2 = x^3 + 4 Z_T^6 ((x, y) -> (Z_T^2 x, Z_T^3 y)); the loop runs there (its formulas never read b), and
// (X : Y : Z) on E' is (X : Y : Z Z_T) on E.  The endomorphism commutes with the map (beta Z^2 x = Z^2 beta x).  Co-Z additions
// (Meloni) give the shared Z without an inversion: DBLU, fourteen ZADDUs, and one backward pass that carries entry j from Z_j to Z_T.
// The formulas are incomplete: an addition with acc = +-T, or a ZADDU whose operands coincide (points of small order), gives Z = 0,
// and Z = 0 survives every later step.  So one test at the end suffices: a lane whose final Z is 0 mod p while the accumulator is
// not the point at infinity recomputes its product with g1_scalar_mul_complete.  No lane of a random subgroup batch does.
C12381_HD bool g1_scalar_mul(g1p& acc, const fp& px, const fp& py, bool p_is_inf, const uint32_t (&kin)[8], int32_t* lane_tab) {
    uint32_t kb0[5], kb1[5];
    glv_scalar_digits(kb0, kb1, kin);

    fp beta;
    fp_set_const(beta, FP_BETA_A);
    g1_coz_forward(lane_tab, px, py, beta, [](int, const fp&) {});
    {   // backward pass: entry j times mu_j^2, mu_j^3 with mu_j = h_j h_(j+1) ... h_15 = Z_T / Z_j; the chain ends in Z_T for free
        fp mu, zt, y2;
#pragma unroll 1
        for (int j = G1_TAB - 1; j >= 2; --j) g1_coz_backward<false>(lane_tab + (j - 1) * G1_ENT_DWORDS, mu, j == G1_TAB - 1, beta);
        fp_raw_dbl(y2, py);
        fp_mul(zt, mu, y2);                                     // Z_T = Z_2 mu_2
        tab_store_zt(lane_tab, zt);
    }

    // the top window starts the accumulator with its first digit's entry (Z = 1)
    g1j a;
    bool acc_inf;
    {
        const int d0 = glv_digit(kb0, G1_WINDOWS - 1);
        fp x, y, ny;
        tab_load_xy(x, y, g1_digit_entry(lane_tab, d0));
        fp_neg(ny, y);
        a.x = x;
        fp_select(a.y, d0 < 0, ny, y);
        fp_one(a.z);
        acc_inf = d0 == 0;
        const int d1 = glv_digit(kb1, G1_WINDOWS - 1);
        tab_load_ybx(y, x, g1_digit_entry(lane_tab, d1));
        g1j_add_digit(a, acc_inf, x, y, d1, true);
    }
#pragma unroll 1
    for (int w = G1_WINDOWS - 2; w >= 0; --w) {
        const int d0 = glv_digit(kb0, w), d1 = glv_digit(kb1, w);
        fp x0, y0, x1, y1;
        tab_fetch_xy(x0, y0, lane_tab, d0);
        g1j_dbl_window(a);
        tab_fetch_ybx(y1, x1, lane_tab, d1);
        g1j_add_digit(a, acc_inf, x0, y0, d0, false);
        g1j_add_digit(a, acc_inf, x1, y1, d1, true);
    }

    fp zt;
    tab_load_zt(zt, lane_tab);
    const bool exc = g1_coz_finish(acc, a, zt, acc_inf || p_is_inf);
    if (exc) g1_scalar_mul_complete(acc, px, py, p_is_inf, kin, lane_tab);
    return exc;
}
// ------------------------------------------------------------------ base-8 Eisenstein digits (the single product: g1_scalar_mul_eis)
// psi = [x^2] : (x, y) -> (beta x, -y) satisfies psi^2 - psi + 1 = 0 on all of E, so k0 + k1 psi is an Eisenstein integer a + b psi (a pair
// (a, b) below; psi (a, b) = (-b, a + b)) and the six units psi^u act on an affine point for nothing: x -> beta^u x, y -> (-1)^u y.  Z[psi] / 8
// has 64 classes; the 63 non-zero ones are unit x representative for ELEVEN representatives (ten orbits of six and the orbit of 4, of three),
// so a table of eleven points serves every digit of the expansion k = sum_w d_w 8^w, d = rep(k mod 8), k <- (k - d) / 8: six bits of norm per
// addition against five of the signed 5-bit windows, and a table of 10 co-Z steps against 15.
// The representatives in chain order: each is the one before plus a unit, so the table is one co-Z chain with a unit image of P as addend.
constexpr int G1E_TAB = 11;
constexpr int G1E_DIGITS = 44;      // |k_n| <= |k| / 8^n + max|d| / 7 with |k|^2 < 3 * 2^256, max|d|^2 = 19: k_43 is 0 or a unit (tests/g1_eisenstein.py digit_bound)
constexpr uint32_t G1E_NONE = 15;   // the entry field of the digit of class 0: no addition
constexpr int EIS_REPS[G1E_TAB][2] = {{1, 0}, {2, -1}, {2, -2}, {2, -3}, {1, -3}, {0, -3}, {1, -4}, {2, -4}, {3, -5}, {3, -4}, {4, -4}};
struct eis_z { int a, b; };
constexpr eis_z eis_mul_unit(eis_z z, int u) {
    for (int i = 0; i < u; ++i) z = eis_z{-z.b, z.a + z.b};
    return z;
}
// u with REPS[i + 1] - REPS[i] = psi^u, or -1
constexpr int eis_chain_unit(int i) {
    for (int u = 0; u < 6; ++u) {
        const eis_z w = eis_mul_unit(eis_z{1, 0}, u);
        if (EIS_REPS[i + 1][0] - EIS_REPS[i][0] == w.a && EIS_REPS[i + 1][1] - EIS_REPS[i][1] == w.b) return u;
    }
    return -1;
}
// step i of the chain adds psi^(u_i) P; the running addend is carried from one step to the next through psi^(u_i - u_(i-1)) (u_(-1) = 0: P
// itself).  Three bits per step.
constexpr uint32_t eis_chain_deltas() {
    uint32_t v = 0;
    int prev = 0;
    for (int i = 0; i + 1 < G1E_TAB; ++i) {
        const int u = eis_chain_unit(i);
        v |= (uint32_t)((u - prev + 6) % 6) << (3 * i);
        prev = u;
    }
    return v;
}
constexpr bool eis_chain_ok() {
    for (int i = 0; i + 1 < G1E_TAB; ++i) if (eis_chain_unit(i) < 0) return false;
    return eis_chain_unit(G1E_TAB - 2) == 0;             // the addend ends as P itself: entry 0 on the table's Z
}
static_assert(eis_chain_ok(), "the representatives are not a chain of unit steps that ends on +P");
constexpr uint32_t EIS_CHAIN_DELTAS = eis_chain_deltas();
// class (a mod 8) + 8 (b mod 8) -> entry (bits 0..3, G1E_NONE for the class of 0) | unit (bits 4..6) | da < 0 (bit 7) | db < 0 (bit 8) of its
// representative d = psi^unit REPS[entry].  The low seven bits are the digit as the loop reads it.  Both coefficients of every d lie in
// [-5, 5], so (c - dc) / 8 = (c >> 3) + (dc < 0) for a coefficient c >= 0, which therefore stays >= 0: the recoder is unsigned.
struct eis_classes { uint16_t v[64]; };
constexpr eis_classes eis_make_classes() {
    eis_classes t{};
    for (int c = 0; c < 64; ++c) t.v[c] = 0xffff;
    t.v[0] = (uint16_t)G1E_NONE;
    for (int e = 0; e < G1E_TAB; ++e)
        for (int u = 0; u < 6; ++u) {
            const eis_z d = eis_mul_unit(eis_z{EIS_REPS[e][0], EIS_REPS[e][1]}, u);
            const int c = (d.a & 7) + 8 * (d.b & 7);
            if (t.v[c] == 0xffff && d.a >= -5 && d.a <= 5 && d.b >= -5 && d.b <= 5)
                t.v[c] = (uint16_t)(e | (u << 4) | ((d.a < 0 ? 1 : 0) << 7) | ((d.b < 0 ? 1 : 0) << 8));
        }
    return t;
}
constexpr bool eis_classes_ok(const eis_classes& t) {
    for (int c = 0; c < 64; ++c) if (t.v[c] == 0xffff) return false;
    return true;
}
C12381_CONST eis_classes EIS_CLASSES = eis_make_classes();
static_assert(eis_classes_ok(eis_make_classes()), "a class mod 8 without a representative");
// the seven-bit digit whose representative IS (a, b), not merely congruent to it mod 8; 0xff where the table's digit of that class is another
constexpr uint32_t eis_exact_code(int a, int b) {
    const uint32_t c = eis_make_classes().v[(a & 7) + 8 * (b & 7)] & 127u;
    if ((c & 15u) >= (uint32_t)G1E_TAB) return 0xffu;
    const eis_z d = eis_mul_unit(eis_z{EIS_REPS[c & 15u][0], EIS_REPS[c & 15u][1]}, (int)(c >> 4));
    return d.a == a && d.b == b ? c : 0xffu;
}
// The top two digits.  What is left of k0 + k1 psi after 42 digits is t = 8 d_43 + d_42 with both coefficients in 0..3 (a coefficient c
// becomes at most (c + 5) / 8 per digit: c_42 <= 2.6918 + 5/7).  Fourteen of those sixteen are nothing or a digit themselves (unit x
// representative exactly), and then position 43 is empty.  The other two are a digit plus one: (3, 2) = (2, 2) + 1, recoded as
// d_42 = (-5, 2) under d_43 = 1, and (3, 3) = (2, 3) + 1, recoded as d_42 = (3, -5) under d_43 = psi (tests/test_g1_eisenstein_seed.py).
constexpr uint32_t EIS_TOP_ONE = eis_exact_code(1, 0), EIS_TOP_PSI = eis_exact_code(0, 1);
constexpr uint32_t EIS_LOW_ONE = eis_exact_code(-5, 2), EIS_LOW_PSI = eis_exact_code(3, -5);
constexpr uint32_t EIS_SEED_ONE = eis_exact_code(2, 2), EIS_SEED_PSI = eis_exact_code(2, 3);
static_assert(EIS_TOP_ONE == 0u && EIS_TOP_PSI == 16u, "1 and psi are not entry 0 under the units 0 and 1");
static_assert(EIS_LOW_ONE != 0xffu && EIS_LOW_PSI != 0xffu, "the digits under a non-empty top position are not (-5, 2) and (3, -5)");
static_assert(EIS_SEED_ONE != 0xffu && EIS_SEED_PSI != 0xffu, "the table does not hold (2, 2) and (2, 3) themselves");

// c <- (c >> 3) + t
C12381_HD void eis_next(uint32_t (&c)[4], uint32_t t) {
    uint64_t s = t;
#pragma unroll
    for (int i = 0; i < 4; ++i) { s += (c[i] >> 3) | (i < 3 ? c[i + 1] << 29 : 0u); c[i] = (uint32_t)s; s >>= 32; }
}
// k0 + k1 psi (k0, k1 < 2^128) -> its G1E_DIGITS digits of seven bits in ten dwords, the TOP digit lowest (digit w in bits 7 (43 - w) ...):
// the loop reads the low seven bits and shifts.  A number that ends early is padded with digits of class 0.
C12381_HD void eis_recode(uint32_t (&kd)[10], const uint32_t (&k0)[4], const uint32_t (&k1)[4]) {
    uint32_t a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = k0[i]; b[i] = k1[i]; }
#pragma unroll
    for (int i = 0; i < 10; ++i) kd[i] = 0;
#pragma unroll
    for (int n = 0; n < G1E_DIGITS; ++n) {
        const uint32_t e = EIS_CLASSES.v[(a[0] & 7u) | ((b[0] & 7u) << 3)];
        const int pos = 7 * (G1E_DIGITS - 1 - n), word = pos >> 5, sh = pos & 31;
        kd[word] |= (e & 127u) << sh;
        if (sh > 25) kd[word + 1] |= (e & 127u) >> (32 - sh);
        eis_next(a, (e >> 7) & 1u);
        eis_next(b, (e >> 8) & 1u);
    }
}
// scalar words (any value < 2^256) -> the digits of k mod r = k0 + k1 x^2
C12381_HD void eis_scalar_digits(uint32_t (&kd)[10], const uint32_t (&kin)[8]) {
    uint32_t k[8], k0[4], k1[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = kin[i];
    scalar_mod_r(k);
    scalar_glv_split(k0, k1, k);
    eis_recode(kd, k0, k1);
}
// the next digit: the low seven bits, and the string moves down
C12381_HD uint32_t eis_pop_digit(uint32_t (&kd)[10]) {
    const uint32_t d = kd[0] & 127u;
#pragma unroll
    for (int i = 0; i < 10; ++i) kd[i] = (kd[i] >> 7) | (i < 9 ? kd[i + 1] << 25 : 0u);
    return d;
}

// Record of entry e (REPS[e] P on the table's Z_T): y | x | beta x | beta^2 x, each field 14 limbs padded to 16 dwords: 256 B, two 128-byte
// lines, eleven entries = G1_TAB_DWORDS.  An addition reads y and ONE x field, aligned 16-byte accesses.  While the table is built, entry i
// holds (Y_i, X_i, h_i) in its first three fields: the point on its own Z_i and the factor that carries Z_i to Z_(i+1).  Z_T lies in the
// pads of the y fields of entries 0..6, written last.
constexpr int G1E_FIELD = 16;
constexpr int G1E_ENT_DWORDS = 4 * G1E_FIELD;
static_assert(G1E_TAB * G1E_ENT_DWORDS == G1_TAB_DWORDS, "the Eisenstein table fills the lane's record of the 16-entry table");
C12381_HD void eis_store_field(int32_t* ent, int f, const fp& a, double vb_cap) {
    (void)vb_cap;
    C12381_BOUNDS(if (a.vb > vb_cap) bounds_fail("eis_store_field value bound", a.vb, vb_cap);
                  if (a.lb > G1_REC_LB) bounds_fail("eis_store_field limb bound", a.lb, G1_REC_LB);)
    int32_t w[G1E_FIELD];
#pragma unroll
    for (int i = 0; i < NL; ++i) w[i] = a.l[i];
    w[14] = 0; w[15] = 0;
    rec_store_q4<0, G1E_FIELD / 4>(reinterpret_cast<q4*>(ent + f * G1E_FIELD), w);
}
C12381_HD void eis_load_field(fp& a, const int32_t* ent, int f, double vb_cap) {
    int32_t w[G1E_FIELD];
    rec_load_q4<0, G1E_FIELD / 4>(w, reinterpret_cast<const q4*>(ent + f * G1E_FIELD));
#pragma unroll
    for (int i = 0; i < NL; ++i) a.l[i] = w[i];
    (void)vb_cap;
    C12381_BOUNDS(a.lb = G1_REC_LB; a.vb = vb_cap; check_actual(a, "eis_load_field");)
}
C12381_HD void eis_store_zt(int32_t* lane_tab, const fp& zt) {
#pragma unroll
    for (int j = 0; j < NL / 2; ++j) { d2 t; t.v[0] = zt.l[2 * j]; t.v[1] = zt.l[2 * j + 1]; *reinterpret_cast<d2*>(lane_tab + j * G1E_ENT_DWORDS + NL) = t; }
}
C12381_HD void eis_load_zt(fp& zt, const int32_t* lane_tab) {
#pragma unroll
    for (int j = 0; j < NL / 2; ++j) { const d2 t = *reinterpret_cast<const d2*>(lane_tab + j * G1E_ENT_DWORDS + NL); zt.l[2 * j] = t.v[0]; zt.l[2 * j + 1] = t.v[1]; }
    C12381_BOUNDS(zt.lb = G1_REC_LB; zt.vb = 4.0; check_actual(zt, "eis_load_zt");)
}
// what the addition of digit `code` reads: y and beta^(unit mod 3) x of its entry (entry 0 for the digit of class 0, dropped afterwards),
// requested here and not later (g1_sched_fence)
C12381_HD void eis_fetch(fp& x, fp& y, const int32_t* lane_tab, uint32_t code) {
    const uint32_t e = code & 15u, u = code >> 4;
    const int32_t* ent = lane_tab + (e >= (uint32_t)G1E_TAB ? 0u : e) * G1E_ENT_DWORDS;
    eis_load_field(y, ent, 0, 4.0);
    eis_load_field(x, ent, 1 + (int)(u >= 3u ? u - 3u : u), 4.0);
    g1_sched_fence();
}
// g1j_madd in NINE reductions, for this loop alone (the k-term sums keep g1j_madd: there this form spills).  H^3 and V = X1 H^2 are not
// formed: X3 = s^2 - H^2 (U2 + X1) is a square and a product under one reduction (H^3 + 2V = H^2 (H + 2 X1)), and
// Y3 = s (V - X3) - Y1 H^3 = H^2 (s X1 - Y1 H) - s X3 is two reductions of two products each.  3S + 9M.  The same values mod p, on the same
// Z3 = Z1 H: Z = 0 stays absorbing, and the lanes with H = 0 are the ones g1j_madd finds.
// Signs: with n = -s = Y1 - S2 (a difference either way round) every product but those by H^2 enters with a plus, and -H^2, negated once,
// serves both: X3 = n^2 + (-H^2)(U2 + X1), W = n X1 + Y1 H = -(s X1 - Y1 H), Y3 = (-H^2) W + n X3.
C12381_HD void g1j_madd_eis(g1j& r, const g1j& p, const fp& x2, const fp& y2) {
    fp zz, zzz, u2, s2, h, n, t, hh, nhh, w, x3, y3, z3;
    fp_sqr(zz, p.z);
    fp_mul(u2, x2, zz);                                  // U2 = x2 Z1^2
    fp_mul(zzz, p.z, zz);
    fp_mul(s2, y2, zzz);                                 // S2 = y2 Z1^3
    fp_sub(h, u2, p.x);                                  // H = U2 - X1
    fp_sub(n, p.y, s2);                                  // n = Y1 - S2 = -s
    fp_add(t, u2, p.x);                                  // U2 + X1
    fp_mul(z3, p.z, h);                                  // Z3 = Z1 H
    fp_sqr(hh, h);
    fp_raw_neg(nhh, hh);
    fp_sqr_madd(x3, n, nhh, t);                          // X3 = s^2 - H^2 (U2 + X1)
    fp_mul2<false>(w, n, p.x, p.y, h);                   // W = -(s X1 - Y1 H)
    fp_mul2<false>(y3, nhh, w, n, x3);                   // Y3 = H^2 (s X1 - Y1 H) - s X3
    r.x = x3; r.y = y3; r.z = z3;
}
// acc += psi^unit T[entry]: the sign of y is (-1)^unit.  g1j_add_signed's steps over g1j_madd_eis.
C12381_HD void g1j_add_eis(g1j& acc, bool& acc_inf, const fp& x, const fp& y, uint32_t code) {
    const bool neg = ((code >> 4) & 1u) != 0u, keep = (code & 15u) == G1E_NONE;
    fp ny, ys, one;
    fp_neg(ny, y);
    fp_select(ys, neg, ny, y);
    g1j r;
    g1j_madd_eis(r, acc, x, ys);
    fp_one(one);
    fp_select(r.x, acc_inf, x, r.x); fp_select(r.y, acc_inf, ys, r.y); fp_select(r.z, acc_inf, one, r.z);
    fp_select(acc.x, keep, acc.x, r.x); fp_select(acc.y, keep, acc.y, r.y); fp_select(acc.z, keep, acc.z, r.z);
    acc_inf = acc_inf && keep;
}

// Forward co-Z pass: ten ZADDUs.  Step i adds the running addend psi^(u_i) P to entry i (entry 0 = P on Z_0 = 1) and gives entry i + 1 and the
// addend on Z_(i+1) = Z_i h_i; between two steps the addend passes through a unit (one product by beta or beta^2 where u_i - u_(i-1) is no
// multiple of 3, a sign on y).  Leaves entries 0..9 as (Y_i, X_i, h_i), entry 10 finished, and fields y, x of entry 0 finished
// from the last addend, which is P on Z_10 = Z_T = h_0 ... h_9; h_0 stays in entry 0 until the backward pass has run, and beta x, beta^2 x
// of entry 0 follow it there.
C12381_HD void g1e_forward(int32_t* lane_tab, const fp& px, const fp& py, const fp& beta, const fp& beta2) {
    fp x1 = px, y1 = py, xj = px, yj = py, xn, yn, h, hn, bx;
#pragma unroll 1
    for (int i = 0; i + 1 < G1E_TAB; ++i) {
        const uint32_t dl = (EIS_CHAIN_DELTAS >> (3 * i)) & 7u, m = dl >= 3u ? dl - 3u : dl;       // wave-uniform
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
    eis_store_field(lane_tab, 0, y1, 4.0); eis_store_field(lane_tab, 1, x1, 2.0);   // x1 is a product: g1_scalar_mul_eis adds beta x1 to it
}
// beta^2 x = -(x + beta x) (1 + beta + beta^2 = 0): a negated lazy sum and one carry round where a product by beta^2 stood.  x and beta x
// are products here (value bounds at most 2 and 1 and a little, so the field's cap of 4 holds; the x of entry 10 is a ZADDU's X3, value
// bound 3, and keeps its product).
C12381_HD void g1e_beta2x(fp& r, const fp& x, const fp& bx) {
    fp t;
    fp_add(t, x, bx);
    fp_neg(t, t);
    fp_norm1(r, t);
}
// One step of the backward pass: mu <- mu h_i (mu = h_i where the chain starts: `first`, wave-uniform), and entry i = (Y_i, X_i, h_i) becomes
// the finished record of the point on Z_i mu.
C12381_HD void g1e_backward(int32_t* ent, fp& mu, bool first, const fp& beta) {
    fp m2, m3, x, y, h, bx, b2x;
    eis_load_field(y, ent, 0, 32.0); eis_load_field(x, ent, 1, 32.0); eis_load_field(h, ent, 2, 32.0);
    if (first) mu = h; else fp_mul(mu, mu, h);
    fp_sqr(m2, mu);
    fp_mul(m3, m2, mu);
    fp_mul(x, x, m2);
    fp_mul(y, y, m3);
    eis_store_field(ent, 0, y, 4.0); eis_store_field(ent, 1, x, 4.0);
    fp_mul(bx, x, beta); eis_store_field(ent, 2, bx, 4.0);
    g1e_beta2x(b2x, x, bx); eis_store_field(ent, 3, b2x, 4.0);
}
// The lane's table of P = (px, py): the forward pass, then the backward pass: entry i times mu_i^2, mu_i^3 with mu_i = h_i ... h_9 =
// Z_T / Z_i; Z_T = h_0 mu_1, and entry 0's beta x, beta^2 x once h_0 has been read.
C12381_HD void g1e_table(int32_t* lane_tab, const fp& px, const fp& py) {
    fp beta, beta2;
    fp_set_const(beta, FP_BETA_A);
    fp_set_const(beta2, FP_BETA_B);                             // beta^2, the other cube root of unity
    g1e_forward(lane_tab, px, py, beta, beta2);
    fp mu, zt, h0, x, bx, b2x;
#pragma unroll 1
    for (int i = G1E_TAB - 2; i >= 1; --i) g1e_backward(lane_tab + i * G1E_ENT_DWORDS, mu, i == G1E_TAB - 2, beta);
    eis_load_field(h0, lane_tab, 2, 32.0);
    eis_load_field(x, lane_tab, 1, 2.0);
    fp_mul(zt, mu, h0);
    fp_mul(bx, x, beta);
    eis_store_field(lane_tab, 2, bx, 4.0);
    g1e_beta2x(b2x, x, bx);
    eis_store_field(lane_tab, 3, b2x, 4.0);
    eis_store_zt(lane_tab, zt);
}
// r = (x1, y1) + (x2, y2), both affine on the table's curve: g1j_madd with Z1 = 1, 4M + 2S in five reductions, Z3 = x2 - x1.  Exceptional
// (Z3 = 0) when the operands are equal or opposite.
C12381_HD void g1e_add_affine(g1j& r, const fp& x1, const fp& y1, const fp& x2, const fp& y2) {
    fp h, s, hh, hhh, v, x3, y3, vx;
    const int32_t cm1 = fp_opaque_const(-1), cm2 = fp_opaque_const(-2);
    fp_sub(h, x2, x1);                                   // H = x2 - x1
    fp_sub(s, y2, y1);                                   // s = y2 - y1
    fp_sqr(hh, h);
    fp_mul(hhh, h, hh);
    fp_mul(v, x1, hh);                                   // V = x1 H^2
    fp_sqr_inj(x3, s, [&](int i, int64_t& acc) { fp_inj(acc, hhh, i, cm1); fp_inj(acc, v, i, cm2); },
               C12381_BV(hhh.vb + 2 * v.vb), C12381_BV(hhh.lb + 2 * v.lb));         // X3 = s^2 - H^3 - 2V
    fp_sub(vx, v, x3);
    fp_mul2<true>(y3, s, vx, y1, hhh);                   // Y3 = s (V - X3) - y1 H^3
    r.x = x3; r.y = y3;
    fp_norm1(r.z, h);
}

// [k]P for an AFFINE input point (x, y) or infinity, result in homogeneous coordinates.  `lane_tab` = this lane's table record
// (G1_TAB_DWORDS).  Returns true for a lane that took the complete path.
// Jacobian doublings and mixed additions over an affine table: a table whose entries share one Jacobian Z = Z_T is affine on the
// isomorphic curve E': y^2 = x^3 + 4 Z_T^6 ((x, y) -> (Z_T^2 x, Z_T^3 y)); the loop runs there (its formulas never read b), and
// (X : Y : Z) on E' is (X : Y : Z Z_T) on E.  The endomorphism commutes with the map (beta Z^2 x = Z^2 beta x).  Co-Z additions
// (Meloni) give the shared Z without an inversion: ten ZADDUs, and one backward pass that carries entry i from Z_i to Z_T.
// Schedule: the top TWO digits seed the accumulator, then 42 windows of three doublings and one mixed addition: 126 doublings and 42 additions
// per scalar (the 5-bit windows of the two halves, which g1_scalar_mul and g1_scalar_mul_sum run: 125 and 52, over a table of 15 steps).
// The seed is [8 d_43 + d_42]P: the point of digit 42 where position 43 is empty, else T[(2, 2)] + P or T[(2, 3)] + P (EIS_SEED_ONE,
// EIS_SEED_PSI above), one affine + affine addition that every lane computes and those lanes keep.
// The formulas are incomplete: an addition with acc = +-T, or a ZADDU whose operands coincide (points of small order: beta x = x on the
// points of order 3), gives Z = 0, and Z = 0 survives every later step.  So one test at the end suffices: a lane whose final Z is 0 mod p
// while the accumulator is not the point at infinity recomputes its product with g1_scalar_mul_complete.  No lane of a random subgroup
// batch does.
C12381_HD bool g1_scalar_mul_eis(g1p& acc, const fp& px, const fp& py, bool p_is_inf, const uint32_t (&kin)[8], int32_t* lane_tab) {
    uint32_t kd[10];
    eis_scalar_digits(kd, kin);

    g1e_table(lane_tab, px, py);

    // the top two digits start the accumulator: the point of digit 42 (Z = 1), or a table point plus P where position 43 is not empty
    g1j a;
    bool acc_inf;
    {
        const uint32_t top = eis_pop_digit(kd), low = eis_pop_digit(kd);
        const bool two = (top & 15u) != G1E_NONE;
        C12381_BOUNDS(if (two && !(top == EIS_TOP_ONE && low == EIS_LOW_ONE) && !(top == EIS_TOP_PSI && low == EIS_LOW_PSI))
                          bounds_fail("the top two digits are no pair the seed knows", top, low);)
        const uint32_t code = two ? (top == EIS_TOP_ONE ? EIS_SEED_ONE : EIS_SEED_PSI) : low;
        fp x, y, ny, ys, x0, y0, one;
        eis_load_field(y0, lane_tab, 0, 4.0); eis_load_field(x0, lane_tab, 1, 4.0);
        eis_fetch(x, y, lane_tab, code);
        fp_neg(ny, y);
        fp_select(ys, ((code >> 4) & 1u) != 0u, ny, y);
        g1e_add_affine(a, x, ys, x0, y0);
        fp_one(one);
        fp_select(a.x, two, a.x, x); fp_select(a.y, two, a.y, ys); fp_select(a.z, two, a.z, one);
        acc_inf = (code & 15u) == G1E_NONE;
    }
#pragma unroll 1
    for (int w = G1E_DIGITS - 3; w >= 0; --w) {
        const uint32_t code = eis_pop_digit(kd);
        fp x, y;
        eis_fetch(x, y, lane_tab, code);
        g1j_dbl(a); g1j_dbl(a); g1j_dbl(a);
        g1j_add_eis(a, acc_inf, x, y, code);
    }

    fp zt;
    eis_load_zt(zt, lane_tab);
    const bool exc = g1_coz_finish(acc, a, zt, acc_inf || p_is_inf);
    if (exc) g1_scalar_mul_complete(acc, px, py, p_is_inf, kin, lane_tab);
    return exc;
}
// ------------------------------------------------------------------ sum of K products under one doubling chain
// sum_j [k_j]P_j per lane (the reference fuses g^x * h^y the same way: double_multiply -> ECP_mul2): K co-Z tables, ONE accumulator, per
// window 5 doublings and 2K mixed additions.  `lane_tab` = K consecutive table records (K * G1_TAB_DWORDS); table j is the 16-entry co-Z
// table of signed 5-bit windows (g1_coz_forward: DBLU and fourteen ZADDUs), on its own Z_T,j.  The mixed additions need every entry affine on ONE curve y^2 = x^3 + 4 Z^6, so the
// backward pass of table j starts its mu chain from f_j = prod_(l != j) Z_T,l instead of from 1: all tables land on Z = prod_j Z_T,j
// without an inversion, and the end of the loop multiplies by that Z once.  Per table this costs 14 products for Z_T,j ahead of the
// backward pass and 8 for entries 16 and 1, which the single table leaves as they are.
// A term at infinity (or not on the curve: the kernel poisons the lane) takes part with all digits 0 and Z_T,j = 1.
// Exceptional lanes: with several terms the accumulator meets +-T_j[d] for RELATED inputs too (Q = +-P, Q = 2P, Q = phi(P), products that
// cancel to infinity), not only for torsion points.  Every such case leaves Jacobian Z = 0 (Z3 = Z1 H with H = 0; no point has order 2, so
// a doubling never does), Z = 0 is absorbing, and a degenerate table has Z_T,j = 0: the one test at the end still suffices, and the lane
// recomputes its K products with g1_scalar_mul_complete and adds them with the complete formulas.
// The pads of entries 1..7 of each record carry Z_T,j (tab_store_zt), those of entries 8..12 the ten biased digit words of the term
// between the table passes (a loop over the terms, so the table code exists once per kernel; the main loop holds all 2K x 5 words in registers).
C12381_HD void tab_store_kb(int32_t* lane_tab, const uint32_t (&kb0)[5], const uint32_t (&kb1)[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) { d2 t; t.v[0] = (int32_t)kb0[j]; t.v[1] = (int32_t)kb1[j]; *reinterpret_cast<d2*>(lane_tab + (NL / 2 + j) * G1_ENT_DWORDS + 42) = t; }
}
C12381_HD void tab_load_kb(uint32_t (&kb0)[5], uint32_t (&kb1)[5], const int32_t* lane_tab) {
#pragma unroll
    for (int j = 0; j < 5; ++j) { const d2 t = *reinterpret_cast<const d2*>(lane_tab + (NL / 2 + j) * G1_ENT_DWORDS + 42); kb0[j] = (uint32_t)t.v[0]; kb1[j] = (uint32_t)t.v[1]; }
}

// `in(j, px, py, inf, k)` hands out term j: the affine point, whether it counts as infinity, the scalar words.  It is called again for
// the terms of an exceptional lane, so the inputs do not stay in registers across the loop.  Returns true for a lane that took the
// complete path.
template <int K, class In>
C12381_HD bool g1_scalar_mul_sum(g1p& acc, const In& in, int32_t* lane_tab) {
    static_assert(K >= 1 && K <= 4, "terms per lane");
    fp beta;
    fp_set_const(beta, FP_BETA_A);
#pragma unroll 1
    for (int t = 0; t < K; ++t) {                               // digits, forward co-Z pass and Z_T,t of every term
        int32_t* tab = lane_tab + t * G1_TAB_DWORDS;
        fp px, py;
        bool p_is_inf;
        uint32_t k[8], kb0[5], kb1[5];
        in(t, px, py, p_is_inf, k);
        glv_scalar_digits(kb0, kb1, k, p_is_inf);
        // Z_T,t is needed before any backward pass, so it is multiplied up here: 14 products
        fp zrun, zt, y2, one;
        g1_coz_forward(tab, px, py, beta, [&](int j, const fp& hn) { if (j == 2) zrun = hn; else fp_mul(zrun, zrun, hn); });   // wave-uniform
        fp_raw_dbl(y2, py);
        fp_mul(zt, zrun, y2);                                   // Z_T = Z_2 h_2 ... h_15
        fp_one(one);
        fp_select(zt, p_is_inf, one, zt);
        tab_store_zt(tab, zt);
        tab_store_kb(tab, kb0, kb1);
    }
#pragma unroll 1
    for (int t = 0; t < K; ++t) {                               // backward passes onto the common Z
        int32_t* tab = lane_tab + t * G1_TAB_DWORDS;
        fp mu;
        if (K > 1) {
            fp m2, m3, x, y, h, bx;
            bool first = true;
#pragma unroll 1
            for (int l = 0; l < K; ++l) {                       // f_t = prod_(l != t) Z_T,l (wave-uniform control flow)
                if (l == t) continue;
                tab_load_zt(h, lane_tab + l * G1_TAB_DWORDS);
                if (first) mu = h; else fp_mul(mu, mu, h);
                first = false;
            }
            fp_sqr(m2, mu);
            fp_mul(m3, m2, mu);
#pragma unroll 1
            for (int e = 0; e < 2; ++e) {                       // entries 1 and 16 are on Z_T,t already
                int32_t* ent = tab + (e == 0 ? 0 : G1_TAB - 1) * G1_ENT_DWORDS;
                tab_load_rec(x, y, bx, ent, 4.0);
                fp_mul(x, x, m2);
                fp_mul(y, y, m3);
                fp_mul(bx, bx, m2);
                tab_store_rec<true>(ent, x, y, bx, 4.0);
            }
        }
        // entry j times mu_j^2, mu_j^3 with mu_j = f_t h_j ... h_15; a single table (K = 1) has f_t = 1 and starts its chain from h_15
#pragma unroll 1
        for (int j = G1_TAB - 1; j >= 2; --j) g1_coz_backward<true>(tab + (j - 1) * G1_ENT_DWORDS, mu, K == 1 && j == G1_TAB - 1, beta);
    }

    uint32_t kb[2 * K][5];
#pragma unroll
    for (int t = 0; t < K; ++t) tab_load_kb(kb[2 * t], kb[2 * t + 1], lane_tab + t * G1_TAB_DWORDS);
    // One loop over the windows and, inside it, one over the terms whose body is the two additions of g1_scalar_mul's window: the code
    // of a window is as long as the single loop's whatever K is.  The digit words rotate by one term per pass (2 x 5 moves per term
    // against two additions), so the term at work is always rows 0 and 1 and no row is indexed by the term counter.
    // The accumulator starts at infinity (acc_inf; its coordinates are then placeholders that every formula accepts) and the top
    // window has no doublings.
    g1j a;
    fp_one(a.x); a.y = a.x; a.z = a.x;
    bool acc_inf = true;
#pragma unroll 1
    for (int w = G1_WINDOWS - 1; w >= 0; --w) {
        fp x0, y0, x1, y1;
        int d0 = glv_digit(kb[0], w);
        tab_fetch_xy(x0, y0, lane_tab, d0);
        if (w < G1_WINDOWS - 1) g1j_dbl_window(a);       // wave-uniform
        const int32_t* tab = lane_tab;
#pragma unroll 1
        for (int t = 0; t < K; ++t) {
            const int d1 = glv_digit(kb[1], w);
            tab_fetch_ybx(y1, x1, tab, d1);
            g1j_add_digit(a, acc_inf, x0, y0, d0, false);
            if (K > 1) {
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const uint32_t r0 = kb[0][i], r1 = kb[1][i];
#pragma unroll
                    for (int j = 0; j + 2 < 2 * K; ++j) kb[j][i] = kb[j + 2][i];
                    kb[2 * K - 2][i] = r0; kb[2 * K - 1][i] = r1;
                }
                tab += G1_TAB_DWORDS;
                if (t + 1 < K) {                         // wave-uniform
                    d0 = glv_digit(kb[0], w);
                    tab_fetch_xy(x0, y0, tab, d0);
                }
            }
            g1j_add_digit(a, acc_inf, x1, y1, d1, true);
        }
    }

    fp zc, z;
    tab_load_zt(zc, lane_tab);
#pragma unroll 1
    for (int t = 1; t < K; ++t) {                               // the common Z = prod_j Z_T,j
        tab_load_zt(z, lane_tab + t * G1_TAB_DWORDS);
        fp_mul(zc, zc, z);
    }
    const bool exc = g1_coz_finish(acc, a, zc, acc_inf);        // acc_inf: every digit of every term was 0
    if (exc) {
#pragma unroll 1
        for (int t = 0; t < K; ++t) {
            fp px, py;
            bool p_is_inf;
            uint32_t k[8];
            in(t, px, py, p_is_inf, k);
            g1p term, n;
            g1_scalar_mul_complete(term, px, py, p_is_inf, k, lane_tab);
            g1_norm1(n, term);
            if (t == 0) { acc = n; continue; }
            g1_add(acc, n);
            g1_norm1(acc);
        }
    }
    return exc;
}
// k mod r < x^2, i.e. k div x^2 == 0: the lanes that owe g1_glv_small_scalar_term (evaluated by a separate, almost always
// empty fix-up kernel so that the main loop's register allocation does not pay for the rare branch)
C12381_HD bool scalar_below_x2(const uint32_t (&kin)[8]) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = kin[i];
    scalar_mod_r(k);
    uint64_t bw = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { uint64_t t = (uint64_t)k[i] - GLV_X2[i] - bw; bw = (t >> 32) & 1; }
    return (k[4] | k[5] | k[6] | k[7]) == 0u && bw == 1;
}

// ------------------------------------------------------------------ affine output
// x = X/Z, y = Y/Z given zinv = 1/Z; compressed tag 0x02|parity(y)  (ECP_toOctet :445-488)
C12381_HD void g1_to_affine(fp& ax, fp& ay, const g1p& p, const fp& zinv) {
    fp_mul(ax, p.x, zinv);
    fp_mul(ay, p.y, zinv);
}

// ------------------------------------------------------------------ compressed-point decoding
// ECP_setx ecp_BLS12381.cpp:302-323: y = sqrt(x^3 + 4) with parity s; fails when the right-hand side is
// not a residue (0 counts as a non-residue: FP_qr).  x is taken mod p (FP_nres), no subgroup check.
C12381_HD bool g1_set_x(fp& y, const fp& x, int s) {
    fp x2, x3, four, rhs, c, cinv, ny;
    fp_sqr(x2, x); fp_mul(x3, x2, x);
    fp_set_const(four, FP_FOUR);
    fp_add(rhs, x3, four);
    const bool qr = fp_sqrt_progen(c, cinv, rhs);
    fp_neg(ny, c);
    fp_select(y, fp_sign(c) != s, ny, c);
    return qr;
}

}  // namespace c12381
