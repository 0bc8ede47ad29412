// Per-lane scalar and byte work of the AC-rps credential entries (examples/AC-rps/src/redact.cpp, pres.cpp, verify.cpp of the reference), host-
// and device-compilable like ac_rbbs.hpp, whose helpers it uses (tests/host_sim/ac_rps.cpp runs it on the CPU under C12381_CHECK_BOUNDS):
//   ac_rps_copy            a run of wire bytes
//   ac_rps_encode97        a decoded 192-byte G2 point as `hash` and `serialize` write it: 0x02 | sign(y), x; 97 zeros for infinity
//   ac_rps_q_head / _q_absorb / _q   q_k = SHA3-512(sigma1_ | sigma2_ | tilde_sigma_ | idx .. | a_I .. | Ip[k]) mod r: the whole blocks of the
//                          shared prefix absorbed once, each k from a copy, the tail spilling into a second block where it has to
//   ac_rps_c0_bytes        the Schnorr transcript sigma1_ | C | C0 is ac_bbs_transcript with no message; c0 is ac_bbs_challenge
//   ac_rps_conv            e_k = sum over the ii with j = k + Ip[ii] - nattr - 1 in J of q_ii a_j mod r, and whether the reference's filter keeps k
//   ac_rps_pres_plan       I -> the base list of verify (nI + 1 records of pk.Y) and of pres (the same, then the kept k ascending)
// Values travel as CANONICAL residues unless a name or a comment says otherwise, as in ac_bbs.hpp.
#pragma once
#include "ac_rbbs.hpp"

namespace c12381 {

constexpr size_t AC_RPS_SIG_BYTES = 195;              // Signature = h | sigma | tilde_M
constexpr size_t AC_RPS_CACHE_BYTES = 97;             // RedactCache = tilde_H
constexpr size_t AC_RPS_PRES_BYTES = 389;             // PresInfo = sigma1_ | sigma2_ | sigma3_ | C | tilde_sigma_ | c0 | s0
constexpr size_t AC_RPS_USK_BYTES = 48;               // UserSecretKey = z
constexpr size_t AC_RPS_PRES_RANDOM = 3;              // r, t, rho
constexpr size_t AC_RPS_LIST_MAX = 32;                // C12381_G1_FIXED_SUM_MAX: one fixed-base table per position of the base list
constexpr size_t AC_RPS_Q_HEAD_BYTES = 195;           // sigma1_ | sigma2_ | tilde_sigma_ in front of the index list
constexpr size_t AC_RPS_C0_BYTES = 147;               // sigma1_ | C | C0

C12381_HD void ac_rps_copy(uint8_t* o, const uint8_t* src, size_t len) {
#pragma unroll 1
    for (size_t b = 0; b < len; ++b) o[b] = src[b];
}

// to_bytes(point2&, compressed) of a decoded point x.b | x.a | y.b | y.a (ECP2_toOctet: 0x02 | sign(y), then x); sign(y) is FP2_sign: the parity of
// y.a, of y.b when y.a is zero.  The all-zero record is infinity: 97 zeros.  For a point that came off the wire this is the re-encoding `hash`
// sees: a leading 0x00 loses the bytes behind it, an x >= p its excess.
C12381_HD void ac_rps_encode97(uint8_t* o97, const uint8_t* p192) {
    uint8_t any = 0, ya = 0;
#pragma unroll 1
    for (int b = 0; b < 192; ++b) any |= p192[b];
#pragma unroll 1
    for (int b = 144; b < 192; ++b) ya |= p192[b];
    o97[0] = any ? (uint8_t)(0x02 | ((ya ? p192[191] : p192[143]) & 1)) : 0;
#pragma unroll 1
    for (int b = 0; b < 96; ++b) o97[1 + b] = p192[b];
}

// hash(sigma1_, sigma2_, tilde_sigma_, indexes, a[j] (j.in(I)), i) (pres.cpp:34, verify.cpp:25): the three encodings, every index of `indexes` as
// the 8 object bytes of a size_t, little-endian (set.hpp:371-377), the nI disclosed values as 48-byte canonical fields in the order of I, then the
// size_t i: 195 + 56 nI + 8 bytes.  The 195 + 56 nI-byte prefix is the same for every i of a lane: ac_rps_q_head writes its first 195 + 8 nI bytes
// into buf, the caller puts the nI fields behind them, ac_rps_q_absorb absorbs its whole 72-byte blocks once.  What is left of it, rem = (195 + 56 nI)
// mod 72, is odd, so rem + 8 is never 72: the tail either fits the last block (rem <= 59) or, at rem = 67 (nI = 8 mod 9), fills one more block and
// leaves 3 bytes for the last.
// buf: the lane's prefix, contiguous (read in aligned words, sha3.hpp: up to 3 bytes past a block that ends the buffer).
C12381_HD size_t ac_rps_q_prefix_bytes(size_t nI) { return AC_RPS_Q_HEAD_BYTES + 56 * nI; }
C12381_HD size_t ac_rps_q_bytes(size_t nI) { return ac_rps_q_prefix_bytes(nI) + 8; }
C12381_HD size_t ac_rps_q_tail_bytes(size_t nI) { return ac_rps_q_prefix_bytes(nI) % (size_t)SHA3_512_RATE + 8; }
C12381_HD void ac_rps_q_head(uint8_t* buf, const uint8_t* s1_49, const uint8_t* s2_49, const uint8_t* ts97, const uint8_t* idx, size_t nI) {
    ac_rps_copy(buf, s1_49, 49);
    ac_rps_copy(buf + 49, s2_49, 49);
    ac_rps_copy(buf + 98, ts97, 97);
#pragma unroll 1
    for (size_t k = 0; k < nI; ++k) {
        buf[AC_RPS_Q_HEAD_BYTES + 8 * k] = idx[k];
#pragma unroll 1
        for (int b = 1; b < 8; ++b) buf[AC_RPS_Q_HEAD_BYTES + 8 * k + b] = 0;
    }
}
C12381_HD uint8_t* ac_rps_q_fields(uint8_t* buf, size_t nI) { return buf + AC_RPS_Q_HEAD_BYTES + 8 * nI; }     // where the nI 48-byte fields go
C12381_HD void ac_rps_q_absorb(uint64_t (&a)[25], const uint8_t* buf, size_t nI) {
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = 0;
    const size_t len = ac_rps_q_prefix_bytes(nI);
#pragma unroll 1
    for (size_t off = 0; len - off >= (size_t)SHA3_512_RATE; off += SHA3_512_RATE) sha3_512_absorb_block(a, buf + off);
}
// q in MONTGOMERY form as fr_from_digest_words returns it, from the state ac_rps_q_absorb left; ip: the hashed index Ip[k]
C12381_HD void ac_rps_q(fr& q_mont, const uint64_t (&prefix)[25], const uint8_t* buf, size_t nI, uint64_t ip) {
    uint64_t a[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) a[k] = prefix[k];
    const size_t len = ac_rps_q_prefix_bytes(nI), rem = len % (size_t)SHA3_512_RATE;
    alignas(8) uint8_t tail[2 * SHA3_512_RATE + 8];
#pragma unroll 1
    for (size_t b = 0; b < rem; ++b) tail[b] = buf[len - rem + b];
#pragma unroll 1
    for (int b = 0; b < 8; ++b) tail[rem + b] = (uint8_t)(ip >> (8 * b));
#pragma unroll 1
    for (size_t b = rem + 8; b < sizeof tail; ++b) tail[b] = 0;
    size_t left = rem + 8;
    const uint8_t* t = tail;
    if (left >= (size_t)SHA3_512_RATE) {               // the spilling tail: one more whole block
        sha3_512_absorb_block(a, t);
        t += SHA3_512_RATE;
        left -= SHA3_512_RATE;
    }
    sha3_512_absorb_last(a, t, left);
    uint64_t h[8];
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = a[k];
    sha3_digest_words_be(w, h);
    fr_from_digest_words(q_mont, w);
}

// The exponent of Y[k] in the cross terms of sigma3_ (pres.cpp:38-55): e = sum of q_ii a_j over the ii <= nI with j = k + Ip[ii] - nattr - 1 inside
// [0, nattr) and outside I (in_I: bit i set for i in I), Ip = idx followed by nattr.  q32 + q_stride ii: q_ii as 32 canonical big-endian bytes;
// attr48: the lane's nattr fields in attribute order, each below r.  Returns whether any ii qualifies — whether the reference's filter keeps k;
// e = 0 when it does not.
C12381_HD bool ac_rps_conv(fr& e, size_t k, size_t nattr, const uint8_t* idx, size_t nI, uint32_t in_I, const uint8_t* q32, size_t q_stride,
                           const uint8_t* attr48) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) e.w[i] = 0;
#pragma unroll 1
    for (size_t ii = 0; ii <= nI; ++ii) {
        const size_t kk = k + (ii < nI ? (size_t)idx[ii] : nattr);
        if (kk < nattr + 1 || kk > 2 * nattr) continue;
        const size_t j = kk - nattr - 1;
        if ((in_I >> j) & 1u) continue;
        if (attr48) {
            uint32_t w[8];
            fr q_mont, a, p;
            words_from_be32(w, q32 + q_stride * ii);
            fr_from_words(q_mont, w);
            zp_parse48(a, attr48 + 48 * j);
            fr_mul(p, q_mont, a);                        // Montgomery x canonical = canonical
            fr_add(e, e, p);
        }
        any = true;
    }
    return any;
}

// The base list of verify and pres: records of pk.Y, at most AC_RPS_LIST_MAX of them, ONE list for g1_fixed_sum_range so that the tables stay
// current between calls and between the two entries.
//   positions [0, nI + 1)       Y[nattr - Ip[k]] in the order of Ip — the bases of verify's S and of sigma3_'s fixed part
//   positions [nI + 1, total)   the k of [0, 2 nattr] the reference's filter keeps, ascending — the cross terms of sigma3_ (cross = true)
// exactly the reference's terms: a record in both parts takes two positions, no zero scalar is put anywhere.
//   y[p]       record of pk.Y at list position p
//   idx[t]     I in the caller's order (the order of the hashed prefix)
struct ac_rps_plan {
    uint8_t y[AC_RPS_LIST_MAX], idx[AC_BBS_MAX_ATTR];
    uint8_t nattr, nI, total;
    uint32_t in_I;
};
// Returns false for nattr = 0, nattr > AC_BBS_MAX_ATTR, nI > nattr, an index >= nattr, a repeated index, or a list longer than AC_RPS_LIST_MAX
C12381_HD bool ac_rps_pres_plan(ac_rps_plan& p, size_t nattr, const uint32_t* idx, size_t nI, bool cross) {
    if (nattr == 0 || nattr > AC_BBS_MAX_ATTR || nI > nattr || nI + 1 > AC_RPS_LIST_MAX) return false;
    uint32_t in_I = 0;
    for (size_t t = 0; t < nI; ++t) {
        const uint32_t i = idx[t];
        if (i >= nattr || ((in_I >> i) & 1u)) return false;
        in_I |= 1u << i;
    }
    for (size_t k = 0; k < AC_RPS_LIST_MAX; ++k) p.y[k] = 0;
    for (size_t k = 0; k < AC_BBS_MAX_ATTR; ++k) p.idx[k] = 0;
    size_t n = 0;
    for (size_t t = 0; t < nI; ++t) { p.idx[t] = (uint8_t)idx[t]; p.y[n++] = (uint8_t)(nattr - idx[t]); }
    p.y[n++] = 0;
    if (cross) {
        fr e;
        for (size_t k = 0; k <= 2 * nattr; ++k) {
            if (!ac_rps_conv(e, k, nattr, p.idx, nI, in_I, nullptr, 0, nullptr)) continue;
            if (n == AC_RPS_LIST_MAX) return false;
            p.y[n++] = (uint8_t)k;
        }
    }
    p.nattr = (uint8_t)nattr; p.nI = (uint8_t)nI; p.total = (uint8_t)n; p.in_I = in_I;
    return true;
}

}  // namespace c12381
