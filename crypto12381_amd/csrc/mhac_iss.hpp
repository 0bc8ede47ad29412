// Per-lane scalar work and the batch constants of the MHAC-bbs issuance entries (examples/MHAC-bbs/src/generate_attributes.cpp, cred_iss.cpp,
// make_pres_group.cpp, make_pres_type.cpp of the reference), host- and device-compilable like mhac_bbs.hpp (tests/host_sim/mhac_iss.cpp runs it on
// the CPU under C12381_CHECK_BOUNDS):
//   mhac_iss_shape_ok        the bounds of t and nparties every entry shares
//   mhac_iss_polynomial      polynomial(x, a0, a) (zp_number.hpp:1087-1113) by Horner's rule on fr
//   mhac_iss_lagrange        lambda[k] = prod_(y != k) (-x[y] / (x[k] - x[y])) for t small integer abscissae: a constant of the batch, computed ONCE on
//                            the host (on integers: see there) and passed to the kernels by value
//   mhac_iss_parties         the argument check of a party set S and its abscissae x[k] = S[k] + 1
//   mhac_iss_attr_list, mhac_iss_pub_list, mhac_iss_type_list    the base lists of the three sums over h
//   mhac_iss_attr_rnd_*, mhac_iss_iss_rnd_*                      where the scalars sit in a credential's rnd
// polynomial and the Lagrange helper know nothing of credentials: a Shamir entry can use them as they stand.
// Values travel as CANONICAL residues (fr words, not Montgomery form) unless a name or a comment says otherwise, as in mhac_bbs.hpp.
#pragma once
#include "mhac_bbs.hpp"

namespace c12381 {

constexpr size_t MHAC_ISS_PARTIES_MAX = 64;          // C12381_MHAC_PARTIES_MAX: x^i <= 64^7 = 2^42 < 2^53, the reference's std::pow is exact

// t parties out of nparties: 1 <= t <= MHAC_BBS_T_MAX, t <= nparties <= MHAC_ISS_PARTIES_MAX
C12381_HD bool mhac_iss_shape_ok(size_t t, size_t nparties) {
    return t >= 1 && t <= MHAC_BBS_T_MAX && nparties >= t && nparties <= MHAC_ISS_PARTIES_MAX;
}

// the small integer x as a canonical residue, and in Montgomery form (x 2^256 mod r)
C12381_HD void mhac_iss_small(fr& v, uint32_t x) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v.w[i] = i == 0 ? x : 0u;
}
C12381_HD void mhac_iss_to_mont(fr& v_mont, const fr& v) {
    fr r2;
    fr_set_words(r2, FR_R2);
    fr_mul(v_mont, v, r2);
}

// a0 + sum_(i < count) a[i] x^(i + 1) for canonical a0 and coefficients, x >= 1 a small integer: ((a[count-1] x + a[count-2]) x + ..) x + a0.
// coeff(i) returns coefficient i; count = 0 (t = 1) returns a0.
template <class Coeff>
C12381_HD void mhac_iss_polynomial(fr& out, uint32_t x, const fr& a0, size_t count, Coeff coeff) {
    fr xs, x_mont, acc;
    mhac_iss_small(xs, x);
    mhac_iss_to_mont(x_mont, xs);
    mhac_iss_small(acc, 0);
#pragma unroll 1
    for (size_t i = count; i-- > 0;) {
        fr a;
        coeff(a, i);
        fr_add(acc, acc, a);
        fr_mul(acc, x_mont, acc);                    // Montgomery x canonical = canonical
    }
    fr_add(out, acc, a0);
}
// the coefficients as 32-byte random values of a lane's rnd, reduced mod r first: scalars [first, first + count)
C12381_HD void mhac_iss_polynomial_rnd(fr& out, uint32_t x, const fr& a0, const uint8_t* rnd, size_t first, size_t count) {
    mhac_iss_polynomial(out, x, a0, count, [=](fr& a, size_t i) { ac_bbs_pres_random(a, rnd, first + i); });
}

// The Lagrange coefficients at 0 of t abscissae, canonical words; lam[k] for k >= t is 0
struct mhac_iss_lambda { uint32_t w[MHAC_BBS_T_MAX][8]; };
// The entries evaluate them ONCE per call, on the host.  Under hipcc the constants of consts.hpp are device symbols, which host code cannot read,
// so this routine does not go through fr: numerator prod(-x[y]) and denominator prod(x[k] - x[y]) are integers below 2^42 in magnitude, and
// lambda[k] = +-|num| / |den| mod r needs one inverse of a SMALL d — (1 + r j) / d for the j < d with d | 1 + r j — and one product by a small
// factor.  Residues are 16 digits of 16 bits (a digit times a 43-bit factor stays inside 64 bits); r is written out here for the same reason.
struct mhac_iss_d16 { uint32_t d[16]; };
C12381_HD void mhac_iss_order16(mhac_iss_d16& r) {
    const uint32_t w[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};      // ORDER_R
    for (int i = 0; i < 8; ++i) { r.d[2 * i] = w[i] & 0xffffu; r.d[2 * i + 1] = w[i] >> 16; }
}
// a + b mod r for a, b < r
C12381_HD void mhac_iss_add16(mhac_iss_d16& out, const mhac_iss_d16& a, const mhac_iss_d16& b) {
    mhac_iss_d16 r, s;
    mhac_iss_order16(r);
    uint32_t c = 0;
    for (int i = 0; i < 16; ++i) { c += a.d[i] + b.d[i]; s.d[i] = c & 0xffffu; c >>= 16; }          // a + b < 2 r < 2^256: no carry out
    bool geq = true;
    for (int i = 15; i >= 0; --i)
        if (s.d[i] != r.d[i]) { geq = s.d[i] > r.d[i]; break; }
    int32_t bw = 0;
    for (int i = 0; i < 16; ++i) {
        int32_t v = (int32_t)s.d[i] - (geq ? (int32_t)r.d[i] : 0) + bw;
        bw = v < 0 ? -1 : 0;
        out.d[i] = (uint32_t)(v & 0xffff);
    }
}
// a s mod r for a < r and s < 2^43, by doubling
C12381_HD void mhac_iss_mul16(mhac_iss_d16& out, const mhac_iss_d16& a, uint64_t s) {
    mhac_iss_d16 acc;
    for (int i = 0; i < 16; ++i) acc.d[i] = 0;
    for (int bit = 42; bit >= 0; --bit) {
        mhac_iss_add16(acc, acc, acc);
        if ((s >> bit) & 1u) mhac_iss_add16(acc, acc, a);
    }
    out = acc;
}
// 1 / d mod r for 1 <= d < 2^43 (r is prime and larger: d is invertible)
C12381_HD void mhac_iss_inv16(mhac_iss_d16& out, uint64_t d) {
    mhac_iss_d16 r;
    mhac_iss_order16(r);
    uint64_t rd = 0;
    for (int i = 15; i >= 0; --i) rd = ((rd << 16) | r.d[i]) % d;
    // j = -1 / rd mod d by the extended Euclidean algorithm (d = 1: rd = 0 and j = 0)
    int64_t a0 = (int64_t)d, a1 = (int64_t)rd, u0 = 0, u1 = 1;
    while (a1 != 0) {
        const int64_t q = a0 / a1, a2 = a0 - q * a1, u2 = u0 - q * u1;
        a0 = a1; a1 = a2; u0 = u1; u1 = u2;
    }
    const int64_t inv = ((u0 % (int64_t)d) + (int64_t)d) % (int64_t)d;                                 // rd inv = 1 mod d
    const uint64_t j = d == 1 ? 0 : (d - (uint64_t)inv) % d;
    uint64_t T[20], c = 1;                                                                           // 1 + r j
    for (int i = 0; i < 16; ++i) { c += (uint64_t)r.d[i] * j; T[i] = c & 0xffffu; c >>= 16; }
    for (int i = 16; i < 20; ++i) { T[i] = c & 0xffffu; c >>= 16; }
    uint64_t rem = 0;
    for (int i = 19; i >= 0; --i) {
        const uint64_t cur = (rem << 16) | T[i];
        if (i < 16) out.d[i] = (uint32_t)(cur / d);                                                  // the quotient is below r: digits 16 .. 19 are 0
        rem = cur % d;
    }
}
// x: t distinct integers in [1, MHAC_ISS_PARTIES_MAX], in the caller's order
C12381_HD void mhac_iss_lagrange(mhac_iss_lambda& lam, const uint32_t* x, size_t t) {
    for (size_t k = 0; k < MHAC_BBS_T_MAX; ++k)
        for (int i = 0; i < 8; ++i) lam.w[k][i] = 0;
    for (size_t k = 0; k < t; ++k) {
        uint64_t num = 1, den = 1;
        bool neg = false;
        for (size_t y = 0; y < t; ++y) {
            if (y == k) continue;
            num *= x[y];                                                                             // -x[y]: one sign each
            neg = !neg;
            if (x[k] > x[y]) den *= x[k] - x[y]; else { den *= x[y] - x[k]; neg = !neg; }
        }
        mhac_iss_d16 inv, v, r;
        mhac_iss_inv16(inv, den);
        mhac_iss_mul16(v, inv, num);
        bool zero = true;
        for (int i = 0; i < 16; ++i) zero = zero && v.d[i] == 0;
        if (neg && !zero) {
            mhac_iss_order16(r);
            int32_t bw = 0;
            for (int i = 0; i < 16; ++i) {
                int32_t d = (int32_t)r.d[i] - (int32_t)v.d[i] + bw;
                bw = d < 0 ? -1 : 0;
                v.d[i] = (uint32_t)(d & 0xffff);
            }
        }
        for (int i = 0; i < 8; ++i) lam.w[k][i] = v.d[2 * i] | (v.d[2 * i + 1] << 16);
    }
}
// S: t party indices below nparties, no index twice -> set.at[k] = S[k], x[k] = S[k] + 1.  False otherwise (and for a null S).
struct mhac_iss_parties_set { uint8_t at[MHAC_BBS_T_MAX]; };
C12381_HD bool mhac_iss_parties(mhac_iss_parties_set& set, uint32_t* x, const uint32_t* S, size_t t, size_t nparties) {
    if (!S || !mhac_iss_shape_ok(t, nparties)) return false;
    uint64_t seen = 0;
    for (size_t k = 0; k < MHAC_BBS_T_MAX; ++k) set.at[k] = 0;
    for (size_t k = 0; k < t; ++k) {
        const uint32_t i = S[k];
        if (i >= nparties || ((seen >> i) & 1u)) return false;
        seen |= (uint64_t)1 << i;
        set.at[k] = (uint8_t)i;
        x[k] = i + 1;
    }
    return true;
}

// generate_attributes.cpp:29: C[k] = prod_ii h[Prv[ii]]^share[k][ii]; returns nPrv
C12381_HD size_t mhac_iss_attr_list(ac_bbs_order& o, const mhac_bbs_sets& s) {
    for (size_t k = 0; k < AC_BBS_MAX_ATTR; ++k) o.at[k] = k < s.nPrv ? s.prv[k] : 0;
    return s.nPrv;
}
// cred_iss.cpp:68: prod_ii h[Pub[ii]]^pub_a[ii] over the caller's public_indexes in their order.  False for nPub > m, an index >= m or a repeated
// index (pub_idx may be null when nPub = 0); m is the caller's to check.
C12381_HD bool mhac_iss_pub_list(ac_bbs_order& o, size_t m, const uint32_t* pub_idx, size_t nPub) {
    if (nPub > m || m > AC_BBS_MAX_ATTR || (nPub && !pub_idx)) return false;
    uint32_t seen = 0;
    for (size_t k = 0; k < AC_BBS_MAX_ATTR; ++k) o.at[k] = 0;
    for (size_t k = 0; k < nPub; ++k) {
        const uint32_t i = pub_idx[k];
        if (i >= m || ((seen >> i) & 1u)) return false;
        seen |= 1u << i;
        o.at[k] = (uint8_t)i;
    }
    return true;
}
// make_pres_type.cpp:30-31: positions [0, nRevPub) are h[Pub[ii]] for ii in I_Pub_in_Rev, positions [nRevPub, nPub) those for ii in I_Pub_in_Hid
// (= HidPub), both ascending; at[k] is the position in Pub whose value is the exponent of list position k.  Returns nPub.
struct mhac_iss_type_plan { ac_bbs_order list; uint8_t at[AC_BBS_MAX_ATTR]; };
C12381_HD size_t mhac_iss_type_list(mhac_iss_type_plan& p, const mhac_bbs_sets& s) {
    size_t k = 0, pos = 0;
    uint8_t pub[AC_BBS_MAX_ATTR];                     // Pub, ascending
    for (size_t i = 0; i < s.m; ++i) {
        bool prv = false;
        for (size_t ii = 0; ii < s.nPrv; ++ii) prv = prv || s.prv[ii] == i;
        if (!prv) pub[pos++] = (uint8_t)i;
    }
    for (size_t ii = 0; ii < s.nRevPub; ++ii, ++k) { p.at[k] = s.revpub[ii]; p.list.at[k] = pub[s.revpub[ii]]; }
    for (size_t ii = 0; ii < s.nHidPub; ++ii, ++k) { p.at[k] = s.hp_pub[ii]; p.list.at[k] = s.hidpub[ii]; }
    const size_t nb = k;
    for (; k < AC_BBS_MAX_ATTR; ++k) { p.at[k] = 0; p.list.at[k] = 0; }
    return nb;
}

// attr's rnd per credential: attr[0 .. m), then a[nPrv (t - 1)]; a[ii (t - 1) .. (ii + 1)(t - 1)) are the coefficients of private attribute ii
C12381_HD size_t mhac_iss_attr_rnd_count(size_t m, size_t nPrv, size_t t) { return m + nPrv * (t - 1); }
C12381_HD size_t mhac_iss_attr_rnd_coeff(size_t m, size_t t, size_t ii) { return m + ii * (t - 1); }
// iss' rnd per credential: e, then the t - 1 coefficients
C12381_HD size_t mhac_iss_iss_rnd_count(size_t t) { return t; }
C12381_HD size_t mhac_iss_iss_rnd_coeff() { return 1; }

}  // namespace c12381
