// Per-signature scalar work of bbs04 sign (examples/bbs04/src/bbs.cpp:32-59 of the reference), host- and device-compilable like fr.hpp and
// sha3.hpp (tests/host_sim/bbs04_sign.cpp runs it on the CPU under C12381_CHECK_BOUNDS):
//   bbs04_sign_reduce      the seven scalars the reference draws, alpha, beta, r_alpha, r_beta, r_x, r_delta1, r_delta2 (32 big-endian bytes
//                          each, any value below 2^256), reduced mod r
//   bbs04_sign_columns     the nine fixed-base scalar columns (negations are mod_negate: -0 = 0)
//   bbs04_sign_responses   c, s_alpha, s_beta, s_x, s_delta1, s_delta2 from c = hash(...).to(Zp) and the member's x
// Values travel as CANONICAL residues (fr words, not Montgomery form) unless a parameter says otherwise: additions and negations do not
// care, and a product with one Montgomery operand is canonical again.
#pragma once
#include "fr.hpp"

namespace c12381 {

// 32 big-endian bytes -> little-endian numeric words
C12381_HD void words_from_be32(uint32_t (&k)[8], const uint8_t* b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint8_t* q = b + 4 * (7 - i);
        k[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    }
}
C12381_HD void store_be32(uint8_t* o, const fr& a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t v = a.w[7 - i];
        o[4 * i] = (uint8_t)(v >> 24); o[4 * i + 1] = (uint8_t)(v >> 16); o[4 * i + 2] = (uint8_t)(v >> 8); o[4 * i + 3] = (uint8_t)v;
    }
}
// serialize(Zp): 48 big-endian bytes, the upper 16 zero
C12381_HD void store_be48(uint8_t* o, const fr& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0;
    store_be32(o + 16, a);
}
// any 256-bit integer -> its canonical residue mod r (2^256 < 3r: at most two subtractions)
C12381_HD void fr_reduce_words(fr& r, const uint32_t (&k)[8]) {
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = k[i];
    if (fr_geq_r(t)) fr_sub_r(t);
    if (fr_geq_r(t)) fr_sub_r(t);
    fr_set_words(r, t);
}

enum { BBS04_ALPHA, BBS04_BETA, BBS04_RA, BBS04_RB, BBS04_RX, BBS04_RD1, BBS04_RD2, BBS04_SIGN_SCALARS };
constexpr int BBS04_SIGN_COLS = 9;

// s[k] = scalar k of rnd224 (the order of the reference's structured binding) mod r
C12381_HD void bbs04_sign_reduce(fr (&s)[BBS04_SIGN_SCALARS], const uint8_t* rnd224) {
#pragma unroll
    for (int k = 0; k < BBS04_SIGN_SCALARS; ++k) {
        uint32_t w[8];
        words_from_be32(w, rnd224 + 32 * k);
        fr_reduce_words(s[k], w);
    }
}
// The fixed-base columns of sign, base in brackets:
//   0 alpha (u)   1 beta (v)   2 alpha + beta (h)                                                         T1, T2, T3 / A
//   3 r_alpha (u)   4 r_beta (v)   5 -r_delta1 (u)   6 -r_delta2 (v)   7 -(r_delta1 + r_delta2) (h)   8 -(r_alpha + r_beta) (h)
// (r_x, the tenth scalar, multiplies the per-signature points T1, T2, T3)
C12381_HD void bbs04_sign_columns(fr (&col)[BBS04_SIGN_COLS], const fr (&s)[BBS04_SIGN_SCALARS]) {
    fr t;
    col[0] = s[BBS04_ALPHA]; col[1] = s[BBS04_BETA];
    fr_add(col[2], s[BBS04_ALPHA], s[BBS04_BETA]);
    col[3] = s[BBS04_RA]; col[4] = s[BBS04_RB];
    fr_neg(col[5], s[BBS04_RD1]); fr_neg(col[6], s[BBS04_RD2]);
    fr_add(t, s[BBS04_RD1], s[BBS04_RD2]); fr_neg(col[7], t);
    fr_add(t, s[BBS04_RA], s[BBS04_RB]); fr_neg(col[8], t);
}
// out = c, s_alpha = r_alpha + c alpha, s_beta = r_beta + c beta, s_x = r_x + cx, s_delta1 = r_delta1 + alpha cx, s_delta2 = r_delta2 + beta cx
// with cx = c x (bbs.cpp:51-56).  c_mont: c in Montgomery form, as fr_from_digest_words returns it; x canonical, below r.
C12381_HD void bbs04_sign_responses(fr (&out)[6], const fr& c_mont, const fr& x, const fr (&s)[BBS04_SIGN_SCALARS]) {
    fr one, r2, cx, cx_mont, t;
#pragma unroll
    for (int i = 0; i < 8; ++i) one.w[i] = i == 0 ? 1u : 0u;
    fr_set_words(r2, FR_R2);
    fr_mul(out[0], c_mont, one);
    fr_mul(t, c_mont, s[BBS04_ALPHA]); fr_add(out[1], s[BBS04_RA], t);
    fr_mul(t, c_mont, s[BBS04_BETA]); fr_add(out[2], s[BBS04_RB], t);
    fr_mul(cx, c_mont, x);
    fr_add(out[3], s[BBS04_RX], cx);
    fr_mul(cx_mont, cx, r2);
    fr_mul(t, cx_mont, s[BBS04_ALPHA]); fr_add(out[4], s[BBS04_RD1], t);
    fr_mul(t, cx_mont, s[BBS04_BETA]); fr_add(out[5], s[BBS04_RD2], t);
}

}  // namespace c12381
