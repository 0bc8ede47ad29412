// Per-lane scalar and byte work of the AC-rbbs credential entries (examples/AC-rbbs/src/redact.cpp, pres.cpp, verify.cpp of the reference), host-
// and device-compilable like ac_bbs.hpp, whose helpers it uses (tests/host_sim/ac_rbbs.cpp runs it on the CPU under C12381_CHECK_BOUNDS):
//   ac_rbbs_split          the leading 49-byte records of a wire block into record columns
//   ac_rbbs_transcript     msg | A_ | B_ | C_J_ | D_ | U; c = SHA3-512(transcript) mod r is ac_bbs_challenge
//   ac_rbbs_q_prefix / _q  q_i = SHA3-512(a_I[0] | .. | a_I[nI-1] | i) mod r: the whole blocks of the shared prefix absorbed once, each i from a copy
//   ac_rbbs_conv           e_k = sum_(i in I, k - nattr + i in J) q_i a_(k - nattr + i) mod r, and whether the reference's filter keeps k
//   ac_rbbs_redact_plan    I -> the base list of redact and the three ranges of it that C_I, D and C_J sum over (host side, before any launch)
// Values travel as CANONICAL residues unless a name or a comment says otherwise, as in ac_bbs.hpp.
#pragma once
#include "ac_bbs.hpp"

namespace c12381 {

constexpr size_t AC_RBBS_PRES_BYTES = 341;            // PresInfo = A_ | B_ | C_J_ | D_ | U | s | t
constexpr size_t AC_RBBS_CACHE_BYTES = 196;           // RedactCache = C_I | C_J | B | D
constexpr size_t AC_RBBS_POINT_BYTES = 5 * 49;        // the five G1 records in front of PresInfo: what the transcript hashes behind msg
constexpr size_t AC_RBBS_REDACT_MAX_ATTR = 16;        // C12381_G1_FIXED_SUM_MAX / 2: redact's base list has up to 2 nattr - 1 entries
constexpr size_t AC_RBBS_PRES_RANDOM = 3;             // r, alpha, beta

// record k of block (k < count) -> o[col_stride * k + 49 * at]
C12381_HD void ac_rbbs_split(uint8_t* o, size_t col_stride, size_t at, const uint8_t* block, int count) {
#pragma unroll 1
    for (int k = 0; k < count; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) o[col_stride * k + 49 * at + b] = block[49 * k + b];
}

// true when every one of the n status bytes is set
C12381_HD bool ac_rbbs_all_set(const uint8_t* st, size_t n) {
    bool ok = true;
#pragma unroll 1
    for (size_t i = 0; i < n; ++i) ok = ok && st[i] != 0;
    return ok;
}

// hash(m, A_, B_, C_J_, D_, U) (pres.cpp:21, verify.cpp:14): msg_len raw bytes with no length prefix, then the five 49-byte encodings.
// e49[k]: the encodings in the order of the transcript.
C12381_HD size_t ac_rbbs_transcript_bytes(size_t msg_len) { return msg_len + AC_RBBS_POINT_BYTES; }
C12381_HD void ac_rbbs_transcript(uint8_t* out, const uint8_t* msg, size_t msg_len, const uint8_t* const* e49) {
#pragma unroll 1
    for (size_t b = 0; b < msg_len; ++b) out[b] = msg[b];
#pragma unroll 1
    for (int k = 0; k < 5; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) out[msg_len + 49 * k + b] = e49[k][b];
}

// hash(a[j] (j.in(I)), i) (verify.cpp:15, redact.cpp:21): the nI disclosed values as 48-byte canonical fields in the order of I, then the size_t i
// as its 8 object bytes, little-endian (set.hpp:371-377): 48 nI + 8 bytes.  The 48 nI-byte prefix is the same for every i of a lane: its whole
// 72-byte blocks are absorbed once (ac_rbbs_q_prefix); what is left of it, 0, 24 or 48 bytes, and the 8 bytes of i always fit the last block.
// aI48: the lane's nI fields, contiguous (read in aligned words, sha3.hpp: up to 3 bytes past a block that ends the buffer).
C12381_HD size_t ac_rbbs_q_bytes(size_t nI) { return 48 * nI + 8; }
C12381_HD void ac_rbbs_q_prefix(uint64_t (&a)[25], const uint8_t* aI48, size_t nI) {
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = 0;
    const size_t len = 48 * nI;
#pragma unroll 1
    for (size_t off = 0; len - off >= (size_t)SHA3_512_RATE; off += SHA3_512_RATE) sha3_512_absorb_block(a, aI48 + off);
}
// q_i in MONTGOMERY form as fr_from_digest_words returns it, from the state ac_rbbs_q_prefix left
C12381_HD void ac_rbbs_q(fr& q_mont, const uint64_t (&prefix)[25], const uint8_t* aI48, size_t nI, uint64_t i) {
    uint64_t a[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) a[k] = prefix[k];
    const size_t len = 48 * nI, rem = len % (size_t)SHA3_512_RATE;
    uint8_t tail[56];
#pragma unroll 1
    for (size_t b = 0; b < rem; ++b) tail[b] = aI48[len - rem + b];
#pragma unroll 1
    for (int b = 0; b < 8; ++b) tail[rem + b] = (uint8_t)(i >> (8 * b));
#pragma unroll 1
    for (size_t b = rem + 8; b < sizeof tail; ++b) tail[b] = 0;
    sha3_512_absorb_last(a, tail, rem + 8);
    uint64_t h[8];
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = a[k];
    sha3_digest_words_be(w, h);
    fr_from_digest_words(q_mont, w);
}

// The exponent of Y[k] in D (redact.cpp:23-41): e = sum of q_i a_j over the i = idx[t] with j = k - nattr + i inside [0, nattr) and outside I
// (in_I: bit i set for i in I).  q32 + q_stride t: q_idx[t] as 32 canonical big-endian bytes; attr48: the lane's nattr fields in attribute order,
// each below r.  Returns whether any i qualifies — whether the reference's filter keeps k; e = 0 when it does not.
C12381_HD bool ac_rbbs_conv(fr& e, size_t k, size_t nattr, const uint8_t* idx, size_t nI, uint32_t in_I, const uint8_t* q32, size_t q_stride,
                            const uint8_t* attr48) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) e.w[i] = 0;
#pragma unroll 1
    for (size_t t = 0; t < nI; ++t) {
        const size_t kk = k + idx[t];
        if (kk < nattr || kk >= 2 * nattr) continue;
        const size_t j = kk - nattr;
        if ((in_I >> j) & 1u) continue;
        uint32_t w[8];
        fr q_mont, a, p;
        words_from_be32(w, q32 + q_stride * t);
        fr_from_words(q_mont, w);
        zp_parse48(a, attr48 + 48 * j);
        fr_mul(p, q_mont, a);                            // Montgomery x canonical = canonical
        fr_add(e, e, p);
        any = true;
    }
    return any;
}

// The base list of redact.  Every Y-sum of redact runs over a range of ONE list of `total` records of pk.Y, so that the fixed-base tables of all of
// them stay current between calls.  With K_D = { nattr - i + j : i in I, j in J }, the k the reference's filter keeps, the list is
//   I \ K_D | I n K_D | K_D above nattr, ascending | J n K_D | J \ K_D        (I parts in the caller's order, J parts ascending)
// and C_I sums [0, nI), D sums [d_first, d_first + nD), C_J sums [cj_first, total): exactly the terms of the reference, no zero scalar anywhere.
//   y[p]       record of pk.Y at list position p
//   acol[c]    attribute index of scalar column c: the nI columns of C_I's range, then the nJ columns of C_J's
//   idx[t]     I in the caller's order (the order of the hashed prefix)
struct ac_rbbs_plan {
    uint8_t y[32], acol[AC_RBBS_REDACT_MAX_ATTR], idx[AC_RBBS_REDACT_MAX_ATTR];
    uint8_t nattr, nI, nJ, total, d_first, nD, cj_first;
    uint32_t in_I;
};
// Returns false for nattr = 0, nattr > AC_RBBS_REDACT_MAX_ATTR, nI > nattr, an index >= nattr or a repeated index
C12381_HD bool ac_rbbs_redact_plan(ac_rbbs_plan& p, size_t nattr, const uint32_t* idx, size_t nI) {
    if (nattr == 0 || nattr > AC_RBBS_REDACT_MAX_ATTR || nI > nattr) return false;
    uint32_t in_I = 0, in_K = 0;
    for (size_t t = 0; t < nI; ++t) {
        const uint32_t i = idx[t];
        if (i >= nattr || ((in_I >> i) & 1u)) return false;
        in_I |= 1u << i;
    }
    for (size_t t = 0; t < nI; ++t)
        for (size_t j = 0; j < nattr; ++j)
            if (!((in_I >> j) & 1u)) in_K |= 1u << (nattr - idx[t] + j);
    for (size_t k = 0; k < sizeof p.y; ++k) p.y[k] = 0;
    for (size_t k = 0; k < AC_RBBS_REDACT_MAX_ATTR; ++k) p.acol[k] = p.idx[k] = 0;
    size_t n = 0, c = 0;
    for (size_t t = 0; t < nI; ++t) p.idx[t] = (uint8_t)idx[t];
    for (size_t t = 0; t < nI; ++t) if (!((in_K >> idx[t]) & 1u)) p.acol[c++] = p.y[n++] = (uint8_t)idx[t];
    p.d_first = (uint8_t)n;
    for (size_t t = 0; t < nI; ++t) if ((in_K >> idx[t]) & 1u) p.acol[c++] = p.y[n++] = (uint8_t)idx[t];
    for (size_t k = nattr; k < 2 * nattr; ++k) if ((in_K >> k) & 1u) p.y[n++] = (uint8_t)k;
    p.cj_first = (uint8_t)n;
    for (size_t j = 0; j < nattr; ++j) if (!((in_I >> j) & 1u) && ((in_K >> j) & 1u)) p.acol[c++] = p.y[n++] = (uint8_t)j;
    p.nD = (uint8_t)(n - p.d_first);
    for (size_t j = 0; j < nattr; ++j) if (!((in_I >> j) & 1u) && !((in_K >> j) & 1u)) p.acol[c++] = p.y[n++] = (uint8_t)j;
    p.nattr = (uint8_t)nattr; p.nI = (uint8_t)nI; p.nJ = (uint8_t)(nattr - nI); p.total = (uint8_t)n; p.in_I = in_I;
    return true;
}

}  // namespace c12381
