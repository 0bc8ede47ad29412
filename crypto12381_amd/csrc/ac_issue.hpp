// Per-lane scalar work of the AC issuance entries (examples/AC-bbs/src/issue.cpp, AC-rbbs/src/issue.cpp, AC-rps/src/issue.cpp and user_keygen.cpp of
// the reference), host- and device-compilable like ac_rps.hpp, whose helpers it uses (tests/host_sim/ac_issue.cpp runs it on the CPU under
// C12381_CHECK_BOUNDS):
//   ac_issue_sk            parse<Zp> / parse<Zp^2> of the issuer's secret key: every field range-checked, used or not
//   ac_issue_random        the ONE scalar the reference draws per call (w, usk, alpha) from rnd_32, reduced mod r; 0 stays 0
//   ac_issue_bbs_lane      AC-bbs / AC-rbbs: the nattr attribute columns of the fixed-base sum, w, and x + w (the argument of the inversion)
//   ac_issue_horner        ym = sum_(i < nattr) a_i y^(i+1) by Horner's rule, and ac_issue_power: y^(nattr+1) in Montgomery form
//   ac_issue_rps_lane      AC-rps: the nattr attribute columns of the G2 sum, alpha, and the two scalars of the k = 2 product over (h, Z):
//                          x + ym and alpha y^(nattr+1)
// Values travel as CANONICAL residues (fr words, not Montgomery form) unless a name or a comment says otherwise, as in ac_bbs.hpp.
// The exponents of DIFFERENT points are never merged: x + ym multiplies the point h, alpha y^(nattr+1) the point Z (include/c12381_ac_issue.h).
#pragma once
#include "ac_rps.hpp"

namespace c12381 {

constexpr size_t AC_ISSUE_MAX_ATTR = AC_BBS_MAX_ATTR;    // C12381_G1_FIXED_SUM_MAX = C12381_G2_FIXED_SUM_MAX: one fixed-base table per attribute
constexpr size_t AC_ISSUE_RPS_SK_FIELDS = 2;             // AC-rps and AC-rbbs: sk = x | y; AC-bbs: x alone
constexpr size_t AC_ISSUE_USK_BYTES = 48, AC_ISSUE_UPK_BYTES = 49;

// field k of sk48 -> out[k], k < count <= 2; returns whether every field is below r (a field that is not leaves its low 32 bytes)
C12381_HD bool ac_issue_sk(fr* out, const uint8_t* sk48, size_t count) {
    bool ok = true;
#pragma unroll 1
    for (size_t k = 0; k < count; ++k) ok = zp_parse48(out[k], sk48 + 48 * k) && ok;
    return ok;
}

// random-select_in<*Zp> with the caller's randomness: 32 big-endian bytes, any value below 2^256, reduced mod r (r and 0 both give 0)
C12381_HD void ac_issue_random(fr& v, const uint8_t* rnd32) { ac_bbs_pres_random(v, rnd32, 0); }

// AC-bbs / AC-rbbs (issue.cpp:12-16).  col0 + col_stride i: a_i as the scalar of Y_i, i < nattr; w32: w; d32: x + w, whose inverse multiplies
// the finished sum.  Returns whether every attribute is below r; the columns of a lane that fails hold the low 32 bytes of its fields.
C12381_HD bool ac_issue_bbs_lane(uint8_t* col0, size_t col_stride, uint8_t* w32, uint8_t* d32, const fr& x, const uint8_t* attr48, size_t nattr,
                                 const uint8_t* rnd32) {
    const bool ok = ac_bbs_zp_columns(col0, col_stride, attr48, nattr, nullptr);
    fr w, d;
    ac_issue_random(w, rnd32);
    fr_add(d, x, w);
    store_be32(w32, w);
    store_be32(d32, d);
    return ok;
}

// ym = a_0 y + a_1 y^2 + .. + a_(nattr-1) y^nattr = ((a_(nattr-1) y + a_(nattr-2)) y + .. + a_0) y (issue.cpp:19-25; the reference's recursion
// normalises at every level, the residue is the same).  attr48: nattr fields, read through zp_parse48 (low 32 bytes).
C12381_HD void ac_issue_horner(fr& ym, const fr& y_mont, const uint8_t* attr48, size_t nattr) {
    fr acc;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc.w[i] = 0;
#pragma unroll 1
    for (size_t i = nattr; i-- > 0;) {
        fr a;
        zp_parse48(a, attr48 + 48 * i);
        fr_add(acc, acc, a);
        fr_mul(acc, y_mont, acc);                        // Montgomery x canonical = canonical
    }
    ym = acc;
}
// y^(nattr+1) in MONTGOMERY form: y multiplied by y nattr times (issue.cpp:27-33)
C12381_HD void ac_issue_power(fr& p_mont, const fr& y_mont, size_t nattr) {
    p_mont = y_mont;
#pragma unroll 1
    for (size_t i = 0; i < nattr; ++i) fr_mul(p_mont, p_mont, y_mont);
}
C12381_HD void ac_issue_to_mont(fr& v_mont, const fr& v) {
    fr r2;
    fr_set_words(r2, FR_R2);
    fr_mul(v_mont, v, r2);
}

// AC-rps (issue.cpp:15-36).  col0 + col_stride i: a_i as the scalar of tilde_Y[i]; al32: alpha (h = g^alpha); e1_32: x + ym, the scalar of h;
// e2_32: alpha y^(nattr+1), the scalar of Z.  Returns whether every attribute is below r.
C12381_HD bool ac_issue_rps_lane(uint8_t* col0, size_t col_stride, uint8_t* al32, uint8_t* e1_32, uint8_t* e2_32, const fr& x, const fr& y,
                                 const uint8_t* attr48, size_t nattr, const uint8_t* rnd32) {
    const bool ok = ac_bbs_zp_columns(col0, col_stride, attr48, nattr, nullptr);
    fr alpha, y_mont, ym, e1, p_mont, e2;
    ac_issue_random(alpha, rnd32);
    ac_issue_to_mont(y_mont, y);
    ac_issue_horner(ym, y_mont, attr48, nattr);
    fr_add(e1, x, ym);
    ac_issue_power(p_mont, y_mont, nattr);
    fr_mul(e2, p_mont, alpha);                           // Montgomery x canonical = canonical
    store_be32(al32, alpha);
    store_be32(e1_32, e1);
    store_be32(e2_32, e2);
    return ok;
}

}  // namespace c12381
