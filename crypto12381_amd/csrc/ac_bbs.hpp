// Per-lane scalar and byte work of the AC-bbs credential entries (examples/AC-bbs/src/pres.cpp, verify.cpp of the reference), host- and
// device-compilable like fr.hpp, sha3.hpp, bbs04_sign.hpp and ps.hpp (tests/host_sim/ac_bbs.cpp runs it on the CPU under C12381_CHECK_BOUNDS):
//   ac_bbs_base_order      the disclosure set I -> the base order I_0 .. I_(nI-1), J_0 .. J_(nJ-1) (J ascending), with the argument checks
//   ac_bbs_split3          the three leading 49-byte records of a 243-byte block (PresInfo.fixed_part A_ | B_ | U; pk.fixed_part's g)
//   ac_bbs_zp_columns      parse<Zp> of consecutive 48-byte fields into base-major 32-byte scalar columns, with the range check
//   ac_bbs_encode49        a decoded 96-byte point as `hash` and `serialize` write it: 0x02 | parity(y), x; 49 zeros for infinity
//   ac_bbs_transcript      msg | A_ | B_ | U, and ac_bbs_challenge: c = SHA3-512(transcript) mod r
//   ac_bbs_pres_random     r, alpha, beta (and each delta_j) of rnd, reduced mod r
//   ac_bbs_responses       s = alpha + r c, t = beta + (-w) c, and ac_bbs_response_u: u_j = delta_j + r c a_J[j]
// Values travel as CANONICAL residues (fr words, not Montgomery form) unless a name or a comment says otherwise, as in bbs04_sign.hpp.
#pragma once
#include "ps.hpp"       // zp_parse48; bbs04_sign.hpp: words_from_be32, store_be32, store_be48, fr_reduce_words; fr.hpp; sha3.hpp

namespace c12381 {

constexpr size_t AC_BBS_FIXED_BYTES = 243;            // pk.fixed_part = g | tilde_g | tilde_X and PresInfo.fixed_part = A_ | B_ | U | s | t
constexpr size_t AC_BBS_SIG_BYTES = 97;               // Signature = A | w
constexpr size_t AC_BBS_POINT_BYTES = 3 * 49;         // the three G1 records in front of PresInfo.fixed_part: what the transcript hashes behind msg
constexpr size_t AC_BBS_MAX_ATTR = 32;                // C12381_G1_FIXED_SUM_MAX: one fixed-base table per attribute
constexpr size_t AC_BBS_PRES_RANDOM = 3;              // r, alpha, beta in front of the nJ delta_j of a lane's rnd

// position k of the base list -> attribute index: the nI disclosed ones in the caller's order, then the nJ hidden ones ascending
struct ac_bbs_order { uint8_t at[AC_BBS_MAX_ATTR]; };

// J = the indices below nattr that are not in I, ascending (pres.cpp:14-15).  Returns false for nattr = 0, nattr > AC_BBS_MAX_ATTR,
// nI > nattr, an index >= nattr or a repeated index; o is complete exactly when it returns true.
C12381_HD bool ac_bbs_base_order(ac_bbs_order& o, size_t nattr, const uint32_t* idx, size_t nI) {
    if (nattr == 0 || nattr > AC_BBS_MAX_ATTR || nI > nattr) return false;
    uint32_t seen = 0;
    for (size_t k = 0; k < nI; ++k) {
        const uint32_t i = idx[k];
        if (i >= nattr || ((seen >> i) & 1u)) return false;
        seen |= 1u << i;
        o.at[k] = (uint8_t)i;
    }
    size_t k = nI;
    for (size_t i = 0; i < nattr; ++i)
        if (!((seen >> i) & 1u)) o.at[k++] = (uint8_t)i;
    for (; k < AC_BBS_MAX_ATTR; ++k) o.at[k] = 0;
    return true;
}

// record k of block243 (k < 3) -> o[k] + 49 * at: column k of a column-major array whose columns are col_stride bytes apart
C12381_HD void ac_bbs_split3(uint8_t* o, size_t col_stride, size_t at, const uint8_t* block243) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) o[col_stride * k + 49 * at + b] = block243[49 * k + b];
}

// Column k (k < count) <- field perm[k] of f48 (perm = nullptr: field k), as 32 big-endian bytes at col0 + col_stride * k.  Returns whether
// every one of the count fields is below r (parse<Zp>, zp_number.hpp:226-236); a field that is not leaves its low 32 bytes in the column.
C12381_HD bool ac_bbs_zp_columns(uint8_t* col0, size_t col_stride, const uint8_t* f48, size_t count, const uint8_t* perm) {
    bool ok = true;
#pragma unroll 1
    for (size_t k = 0; k < count; ++k) {
        fr v;
        ok = zp_parse48(v, f48 + 48 * (perm ? perm[k] : k)) && ok;
        store_be32(col0 + col_stride * k, v);
    }
    return ok;
}

// to_bytes(point1&, compressed) of a decoded point x | y (ECP_toOctet: 0x02 | parity(y), then x); the all-zero record is infinity: 49 zeros.
// For a point that came off the wire this is the re-encoding `hash` sees: a leading 0x00 loses the bytes behind it, an x >= p its excess.
C12381_HD void ac_bbs_encode49(uint8_t* o49, const uint8_t* p96) {
    uint8_t any = 0;
#pragma unroll 1
    for (int b = 0; b < 96; ++b) any |= p96[b];
    o49[0] = any ? (uint8_t)(0x02 | (p96[95] & 1)) : 0;
#pragma unroll 1
    for (int b = 0; b < 48; ++b) o49[1 + b] = p96[b];
}

// hash(m, A_, B_, U) (pres.cpp:31, verify.cpp:20): msg_len raw bytes with no length prefix (set.hpp:355-384), then the three 49-byte encodings
C12381_HD size_t ac_bbs_transcript_bytes(size_t msg_len) { return msg_len + AC_BBS_POINT_BYTES; }
C12381_HD void ac_bbs_transcript(uint8_t* out, const uint8_t* msg, size_t msg_len, const uint8_t* a49, const uint8_t* b49, const uint8_t* u49) {
#pragma unroll 1
    for (size_t b = 0; b < msg_len; ++b) out[b] = msg[b];
#pragma unroll 1
    for (int b = 0; b < 49; ++b) { out[msg_len + b] = a49[b]; out[msg_len + 49 + b] = b49[b]; out[msg_len + 98 + b] = u49[b]; }
}
// c = SHA3-512(transcript) as a big-endian integer mod r (Zp from_hash), in MONTGOMERY form as fr_from_digest_words returns it
C12381_HD void ac_bbs_challenge(fr& c_mont, const uint8_t* tr, size_t len) {
    uint64_t h[8];
    uint32_t w[16];
    sha3_512(h, tr, len);
    sha3_digest_words_be(w, h);
    fr_from_digest_words(c_mont, w);
}
C12381_HD void fr_mont_to_canonical(fr& r, const fr& a_mont) {
    uint32_t k[8];
    fr_to_words(k, a_mont);
    fr_set_words(r, k);
}

// scalar k of a lane's rnd (r, alpha, beta, delta_0 ..: 32 big-endian bytes each, any value below 2^256), reduced mod r
C12381_HD void ac_bbs_pres_random(fr& v, const uint8_t* rnd, size_t k) {
    uint32_t w[8];
    words_from_be32(w, rnd + 32 * k);
    fr_reduce_words(v, w);
}
// s = alpha + r c, t = beta + (-w) c (pres.cpp:34-35) and rc_mont = r c in Montgomery form for ac_bbs_response_u.  negw = mod_negate(w): -0 = 0.
C12381_HD void ac_bbs_responses(fr& s, fr& t, fr& rc_mont, const fr& c_mont, const fr& r, const fr& alpha, const fr& beta, const fr& negw) {
    fr rc, wc, r2;
    fr_mul(rc, c_mont, r);                           // Montgomery x canonical = canonical
    fr_add(s, alpha, rc);
    fr_mul(wc, c_mont, negw);
    fr_add(t, beta, wc);
    fr_set_words(r2, FR_R2);
    fr_mul(rc_mont, rc, r2);
}
// u_j = delta_j + r c a_J[j] (pres.cpp:36)
C12381_HD void ac_bbs_response_u(fr& u, const fr& rc_mont, const fr& delta, const fr& a) {
    fr t;
    fr_mul(t, rc_mont, a);
    fr_add(u, delta, t);
}

}  // namespace c12381
