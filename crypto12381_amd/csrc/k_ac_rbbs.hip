// The AC-rbbs credential kernels (examples/AC-rbbs/src/redact.cpp, pres.cpp, verify.cpp of the reference), one credential per lane; the per-lane
// scalar and byte routines are ac_rbbs.hpp's and ac_bbs.hpp's:
//   ac_rbbs_gather_kernel         records of a key picked by index: the used pk.Y / pk.tilde_Y of verify, redact's base list
//   ac_rbbs_verify_prep_kernel    PresInfo -> the five record columns, parse<Zp> range checks, the columns s, t | a_I .., the q_i columns
//   ac_rbbs_encode_kernel         decoded points -> the 49-byte encodings the transcript hashes
//   ac_rbbs_challenge_kernel      the transcript msg | A_ | B_ | C_J_ | D_ | U and c = SHA3-512(transcript) mod r
//   ac_rbbs_verify_finish_kernel  ok = both pairing verdicts and [K^s A_^t (-B_)^c == U], or 0xff where the reference would throw
//   ac_rbbs_pres_prep_kernel      Signature, RedactCache, randomness -> the five record columns, r four times, alpha, beta
//   ac_rbbs_pres_finish_kernel    s, t from c and the record PresInfo; 0xff where the reference would throw
//   ac_rbbs_redact_prep_kernel    Signature, attributes -> A's record, the attribute columns of the base list, -w, the q_i and the exponents e_k of D
//   ac_rbbs_redact_finish_kernel  C_I, C_J, B, D -> the record RedactCache; 0xff where the reference would throw
// api_ac_rbbs.hip launches them between the library's existing kernels (and k_ac_bbs.hip's bcast and A_ / -B_ encode kernels).
#include "kernels_common.hpp"
#include "ac_rbbs.hpp"

using namespace c12381;

namespace c12381 {

// out[rec_bytes t .. ) = record ord.at[t] of `in`, t < count
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_gather_kernel(size_t count, size_t rec_bytes, ac_bbs_order ord, const uint8_t* in, uint8_t* out) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= rec_bytes * count) return;
    out[t] = in[rec_bytes * (size_t)ord.at[t / rec_bytes] + t % rec_bytes];
}

// p49: columns A_, B_, U, C_J_, D_ of n records (U third: the first three are the columns ac_bbs_encode_kernel takes).  sc3: columns s, t (c joins
// them: ac_rbbs_challenge_kernel).  sca[32 (k n + j)]: the disclosed a_idx[k] (attr48 lane-major in the order of idx); q32[32 (k n + j)]: q_idx[k].
// st[j] = 1 when every Zp field of the lane is below r.
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_verify_prep_kernel(size_t n, size_t nI, ac_bbs_order idx, const uint8_t* pres341, const uint8_t* attr48,
                                                                     uint8_t* p49, uint8_t* sc3, uint8_t* sca, uint8_t* q32, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* rec = pres341 + AC_RBBS_PRES_BYTES * j;
    ac_rbbs_split(p49, 49 * n, j, rec, 2);                                  // A_, B_
    ac_rbbs_split(p49 + 3 * 49 * n, 49 * n, j, rec + 98, 2);                // C_J_, D_
    ac_rbbs_split(p49 + 2 * 49 * n, 49 * n, j, rec + 196, 1);               // U
    bool ok = ac_bbs_zp_columns(sc3 + 32 * j, 32 * n, rec + AC_RBBS_POINT_BYTES, 2, nullptr);
    if (nI) {
        const uint8_t* aI = attr48 + 48 * nI * j;
        ok = ac_bbs_zp_columns(sca + 32 * j, 32 * n, aI, nI, nullptr) && ok;
        uint64_t pre[25];
        ac_rbbs_q_prefix(pre, aI, nI);
#pragma unroll 1
        for (size_t k = 0; k < nI; ++k) {
            fr q_mont, q;
            ac_rbbs_q(q_mont, pre, aI, nI, idx.at[k]);
            fr_mont_to_canonical(q, q_mont);
            store_be32(q32 + 32 * (k * n + j), q);
        }
    }
    st[j] = ok ? 1 : 0;
}

// e49[49 (k n + j)] = the encoding of p96[96 (k n + j)], k < count
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_encode_kernel(size_t n, size_t count, const uint8_t* p96, uint8_t* e49) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
#pragma unroll 1
    for (size_t k = 0; k < count; ++k) ac_bbs_encode49(e49 + 49 * (k * n + j), p96 + 96 * (k * n + j));
}

// tr + L j: the transcript of lane j, L = msg_len + 245; e49: five columns, u_col the column of U (2: verify; 4: pres), the others A_, B_, C_J_, D_ in
// that order; c32 + 32 j: c as 32 canonical big-endian bytes
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_challenge_kernel(size_t n, size_t msg_len, const uint8_t* msgs, const uint8_t* e49, int u_col, uint8_t* tr,
                                                                   uint8_t* c32) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t L = ac_rbbs_transcript_bytes(msg_len);
    uint8_t* t = tr + L * j;
    const uint8_t* e[5];
    int col = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (col == u_col) ++col; e[k] = e49 + 49 * ((size_t)col * n + j); ++col; }
    e[4] = e49 + 49 * ((size_t)u_col * n + j);
    ac_rbbs_transcript(t, msgs + msg_len * j, msg_len, e);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, t, L);
    fr_mont_to_canonical(c, c_mont);
    store_be32(c32 + 32 * j, c);
}

// ok[j] = 1 / 0: both pairing verdicts ok1[j], ok3[j] and r49[j] (K^s A_^t (-B_)^c, compressed) == the encoding of U (u49), or 0xff where the
// reference would throw: a Zp field >= r (st), one of the five points not decodable (st_p, five columns), or a used key record that does not
// decode (st_pub, npub statuses: every lane, and bad_flag[0] -> C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_verify_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p,
                                                                       const uint8_t* r49, const uint8_t* u49, const uint8_t* ok1, const uint8_t* ok3,
                                                                       uint8_t* ok, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    if (!ac_rbbs_all_set(st_pub, npub)) { ok[j] = 0xff; if (j == 0) *bad_flag = 1; return; }
    bool pts = st[j] != 0;
#pragma unroll 1
    for (size_t k = 0; k < 5; ++k) pts = pts && st_p[k * n + j] != 0;
    if (!pts) { ok[j] = 0xff; return; }
    uint8_t diff = 0;
#pragma unroll 1
    for (int b = 0; b < 49; ++b) diff |= r49[49 * j + b] ^ u49[49 * j + b];
    ok[j] = (ok1[j] == 1 && ok3[j] == 1 && diff == 0) ? 1 : 0;
}

// p49: columns C_I, A, B, C_J, D (the last four are ONE column of 4 n lanes that r multiplies).  scr[32 (k n + j)], k < 4: r; sc2: columns alpha, beta —
// the scalars of the k = 2 product over (C_I, A_).  st[j] = 1 when w is below r.
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_pres_prep_kernel(size_t n, const uint8_t* sig97, const uint8_t* cache196, const uint8_t* rnd, uint8_t* p49,
                                                                   uint8_t* scr, uint8_t* sc2, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t *sig = sig97 + AC_BBS_SIG_BYTES * j, *ca = cache196 + AC_RBBS_CACHE_BYTES * j, *rn = rnd + 32 * AC_RBBS_PRES_RANDOM * j;
    ac_rbbs_split(p49, 49 * n, j, ca, 1);                                   // C_I
    ac_rbbs_split(p49 + 49 * n, 49 * n, j, sig, 1);                         // A
    ac_rbbs_split(p49 + 2 * 49 * n, 49 * n, j, ca + 2 * 49, 1);             // B
    ac_rbbs_split(p49 + 3 * 49 * n, 49 * n, j, ca + 49, 1);                 // C_J
    ac_rbbs_split(p49 + 4 * 49 * n, 49 * n, j, ca + 3 * 49, 1);             // D
    fr w, v;
    st[j] = zp_parse48(w, sig + 49) ? 1 : 0;
    ac_bbs_pres_random(v, rn, 0);
#pragma unroll 1
    for (size_t k = 0; k < 4; ++k) store_be32(scr + 32 * (k * n + j), v);
    ac_bbs_pres_random(v, rn, 1); store_be32(sc2 + 32 * j, v);
    ac_bbs_pres_random(v, rn, 2); store_be32(sc2 + 32 * (n + j), v);
}

// pres341[j] = A_ | B_ | C_J_ | D_ | U (e49 columns) | s | t, status[j] = 0.  Where the reference would throw — A or a cache point does not decode
// (st_p, five columns), w >= r (st) — status[j] = 0xff and the record is 0xff bytes.
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_pres_finish_kernel(size_t n, const uint8_t* sig97, const uint8_t* rnd, const uint8_t* e49, const uint8_t* c32,
                                                                     const uint8_t* st, const uint8_t* st_p, uint8_t* pres341, uint8_t* status) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    uint8_t* o = pres341 + AC_RBBS_PRES_BYTES * j;
    bool ok = st[j] != 0;
#pragma unroll 1
    for (size_t k = 0; k < 5; ++k) ok = ok && st_p[k * n + j] != 0;
    if (!ok) {
#pragma unroll 1
        for (size_t b = 0; b < AC_RBBS_PRES_BYTES; ++b) o[b] = 0xff;
        status[j] = 0xff;
        return;
    }
    const uint8_t* rn = rnd + 32 * AC_RBBS_PRES_RANDOM * j;
    uint32_t k8[8];
    fr c_mont, r, alpha, beta, w, negw, s, t, rc_mont;
    words_from_be32(k8, c32 + 32 * j);
    fr_from_words(c_mont, k8);
    ac_bbs_pres_random(r, rn, 0); ac_bbs_pres_random(alpha, rn, 1); ac_bbs_pres_random(beta, rn, 2);
    zp_parse48(w, sig97 + AC_BBS_SIG_BYTES * j + 49);
    fr_neg(negw, w);
    ac_bbs_responses(s, t, rc_mont, c_mont, r, alpha, beta, negw);
#pragma unroll 1
    for (size_t k = 0; k < 5; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) o[49 * k + b] = e49[49 * (k * n + j) + b];
    store_be48(o + AC_RBBS_POINT_BYTES, s);
    store_be48(o + AC_RBBS_POINT_BYTES + 48, t);
    status[j] = 0;
}

// a49[j] = A's wire bytes.  sca[32 (c n + j)] = attribute pl.acol[c] (attr48: the lane's whole span of nattr fields), scw[32 j] = -w,
// aI48[48 nI j ..]: the disclosed fields in the order of idx (the hashed prefix), q32[32 (t n + j)] = q_idx[t], scd[32 (t n + j)] = the exponent of
// the base at position d_first + t of the list.  st[j] = 1 when w and every attribute are below r (the exponents of other lanes are never used).
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_redact_prep_kernel(size_t n, ac_rbbs_plan pl, const uint8_t* attr48, const uint8_t* sig97, uint8_t* a49,
                                                                     uint8_t* sca, uint8_t* scw, uint8_t* aI48, uint8_t* q32, uint8_t* scd, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t nattr = pl.nattr, nI = pl.nI;
    const uint8_t *sig = sig97 + AC_BBS_SIG_BYTES * j, *attr = attr48 + 48 * nattr * j;
    ac_rbbs_split(a49, 0, j, sig, 1);
    fr w, v;
    bool ok = zp_parse48(w, sig + 49);
    ok = ac_bbs_zp_columns(sca + 32 * j, 32 * n, attr, nattr, pl.acol) && ok;
    st[j] = ok ? 1 : 0;
    fr_neg(v, w); store_be32(scw + 32 * j, v);
    if (nI == 0) return;                              // kernel-uniform: no q, and D is the empty product
    uint8_t* aI = aI48 + 48 * nI * j;
#pragma unroll 1
    for (size_t t = 0; t < nI; ++t)
#pragma unroll 1
        for (int b = 0; b < 48; ++b) aI[48 * t + b] = attr[48 * (size_t)pl.idx[t] + b];
    uint64_t pre[25];
    ac_rbbs_q_prefix(pre, aI, nI);
#pragma unroll 1
    for (size_t t = 0; t < nI; ++t) {
        fr q_mont, q;
        ac_rbbs_q(q_mont, pre, aI, nI, pl.idx[t]);
        fr_mont_to_canonical(q, q_mont);
        store_be32(q32 + 32 * (t * n + j), q);
    }
#pragma unroll 1
    for (size_t t = 0; t < pl.nD; ++t) {
        fr e;
        ac_rbbs_conv(e, pl.y[pl.d_first + t], nattr, pl.idx, nI, pl.in_I, q32 + 32 * j, 32 * n, attr);
        store_be32(scd + 32 * (t * n + j), e);
    }
}

// cache196[j] = the encodings of o96's columns C_I, C_J, B, D, status[j] = 0.  Where the reference would throw — A does not decode (st_a), w or an
// attribute >= r (st) — status[j] = 0xff and the record is 0xff bytes; a key that does not decode (st_pub, npub statuses) does that to every
// lane and raises bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) ac_rbbs_redact_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_a,
                                                                       const uint8_t* o96, uint8_t* cache196, uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool pub = ac_rbbs_all_set(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t* o = cache196 + AC_RBBS_CACHE_BYTES * j;
    if (!pub || !st[j] || !st_a[j]) {
#pragma unroll 1
        for (size_t b = 0; b < AC_RBBS_CACHE_BYTES; ++b) o[b] = 0xff;
        status[j] = 0xff;
        return;
    }
#pragma unroll 1
    for (size_t k = 0; k < 4; ++k) ac_bbs_encode49(o + 49 * k, o96 + 96 * (k * n + j));
    status[j] = 0;
}

}  // namespace c12381
