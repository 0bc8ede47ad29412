// The AC-bbs credential kernels (examples/AC-bbs/src/pres.cpp, verify.cpp of the reference), one presentation per lane; the per-lane scalar and
// byte routines are ac_bbs.hpp's:
//   ac_bbs_key_kernel            pk.Y -> the 49-byte records in base order (disclosed attributes' Y in the caller's order, then the hidden ones)
//   ac_bbs_bcast96_kernel        one 96-byte point for every lane: K = C_I = g when nothing is disclosed
//   ac_bbs_verify_prep_kernel    PresInfo -> A_, B_, U record columns, parse<Zp> range checks, the scalar columns s, t | a_I .. | u_J ..
//   ac_bbs_encode_kernel         A_, B_, U decoded -> the 49-byte encodings the transcript hashes; verify: A_ and -B_ as terms of the k = 3 product
//   ac_bbs_challenge_kernel      the transcript msg | A_ | B_ | U and c = SHA3-512(transcript) mod r
//   ac_bbs_verify_finish_kernel  ok = pairing verdict and [K^s A_^t (-B_)^c + sum_j Y_J[j]^u_j == U], or 0xff where the reference would throw
//   ac_bbs_pres_prep_kernel      Signature, attributes, randomness -> A's record, the attribute columns in base order, delta_j, r, alpha, -w, beta
//   ac_bbs_pres_finish_kernel    s, t, u_j from c and the records PresInfo.fixed_part, PresInfo.u; 0xff where the reference would throw
// api_ac_bbs.hip launches them; decompression, the fixed-base sums, the k-way products, additions, affine conversions and the pairing half
// (c12381_ps_verify_batch_dev) are the library's existing kernels.
#include "kernels_common.hpp"
#include "ac_bbs.hpp"

using namespace c12381;

namespace {

// st_pub: the decoding statuses of g, tilde_g, tilde_X and the nattr Y
__device__ __forceinline__ bool ac_bbs_pub_ok(const uint8_t* st_pub, size_t npub) {
    bool pub = true;
#pragma unroll 1
    for (size_t i = 0; i < npub; ++i) pub = pub && st_pub[i] != 0;
    return pub;
}
__device__ __forceinline__ void copy96(uint8_t* dst, const uint8_t* src) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = s[i];
}

}  // namespace

namespace c12381 {

__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_key_kernel(size_t nattr, ac_bbs_order ord, const uint8_t* y49, uint8_t* out49) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= 49 * nattr) return;
    out49[t] = y49[49 * (size_t)ord.at[t / 49] + t % 49];
}

__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_bcast96_kernel(size_t n, const uint8_t* src96, uint8_t* dst96) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    copy96(dst96 + 96 * j, src96);
}

// p49: columns A_, B_, U of n records.  sc3: columns s, t (c joins them as the third: ac_bbs_challenge_kernel) — the scalars of K, A_, -B_.
// sca[32 (k n + j)]: the scalar of base k in base order — the disclosed a_i (k < nI, attr48 lane-major in the order of idx), then u_j.
// st[j] = 1 when every Zp field of the lane is below r.
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_verify_prep_kernel(size_t n, size_t nI, size_t nJ, const uint8_t* pres243, const uint8_t* u48,
                                                                    const uint8_t* attr48, uint8_t* p49, uint8_t* sc3, uint8_t* sca, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* rec = pres243 + AC_BBS_FIXED_BYTES * j;
    ac_bbs_split3(p49, 49 * n, j, rec);
    bool ok = ac_bbs_zp_columns(sc3 + 32 * j, 32 * n, rec + AC_BBS_POINT_BYTES, 2, nullptr);
    if (nI) ok = ac_bbs_zp_columns(sca + 32 * j, 32 * n, attr48 + 48 * nI * j, nI, nullptr) && ok;
    if (nJ) ok = ac_bbs_zp_columns(sca + 32 * (nI * n + j), 32 * n, u48 + 48 * nJ * j, nJ, nullptr) && ok;
    st[j] = ok ? 1 : 0;
}

// e49: columns A_, B_, U as `hash` and `serialize` encode the decoded points a96[j], b96[j], u96[j].  q96 (verify; null in pres): columns K, A_,
// -B_ of the k = 3 product — A_ copied, B_ with y negated (infinity stays the zero record); K is written by the fixed-base sum.
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_encode_kernel(size_t n, const uint8_t* a96, const uint8_t* b96, const uint8_t* u96, uint8_t* e49,
                                                               uint8_t* q96) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    ac_bbs_encode49(e49 + 49 * j, a96 + 96 * j);
    ac_bbs_encode49(e49 + 49 * (n + j), b96 + 96 * j);
    ac_bbs_encode49(e49 + 49 * (2 * n + j), u96 + 96 * j);
    if (!q96) return;                                 // kernel-uniform
    copy96(q96 + 96 * (n + j), a96 + 96 * j);
    uint32_t raw[12];
    fp y, ny;
    uint8_t* o = q96 + 96 * (2 * n + j);
    load_raw48(raw, b96 + 96 * j); store_raw48(o, raw);
    load_raw48(raw, b96 + 96 * j + 48); fp_from_raw48(y, raw);
    fp_neg(ny, y); fp_norm1(y, ny);
    fp_to_raw48(raw, y); store_raw48(o + 48, raw);
}

// tr + L j: the transcript of lane j, L = msg_len + 147 (e49: columns A_, B_, U); c32 + 32 j: c as 32 canonical big-endian bytes
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_challenge_kernel(size_t n, size_t msg_len, const uint8_t* msgs, const uint8_t* e49, uint8_t* tr,
                                                                  uint8_t* c32) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t L = ac_bbs_transcript_bytes(msg_len);
    uint8_t* t = tr + L * j;
    ac_bbs_transcript(t, msgs + msg_len * j, msg_len, e49 + 49 * j, e49 + 49 * (n + j), e49 + 49 * (2 * n + j));
    fr c_mont, c;
    ac_bbs_challenge(c_mont, t, L);
    fr_mont_to_canonical(c, c_mont);
    store_be32(c32 + 32 * j, c);
}

// ok[j] = 1 / 0: the pairing verdict okp[j] and r49[j] (K^s A_^t (-B_)^c + sum_j Y_J[j]^u_j, compressed) == the encoding of U (u49), or 0xff where
// the reference would throw: a Zp field >= r (st), A_ / B_ / U not decodable (st_p, three columns), or a key that does not decode (st_pub, npub
// statuses: every lane, and bad_flag[0] -> C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_verify_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p,
                                                                      const uint8_t* r49, const uint8_t* u49, const uint8_t* okp, uint8_t* ok, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    if (!ac_bbs_pub_ok(st_pub, npub)) { ok[j] = 0xff; if (j == 0) *bad_flag = 1; return; }
    if (!st[j] || !st_p[j] || !st_p[n + j] || !st_p[2 * n + j]) { ok[j] = 0xff; return; }
    uint8_t diff = 0;
#pragma unroll 1
    for (int b = 0; b < 49; ++b) diff |= r49[49 * j + b] ^ u49[49 * j + b];
    ok[j] = (okp[j] == 1 && diff == 0) ? 1 : 0;
}

// a49[j] = A's wire bytes.  sca[32 (k n + j)] = the attribute of base k in base order (attr48: the lane's whole span of nattr fields), scd: the nJ
// columns delta_j, sc2: the columns r, alpha, -w, beta — r multiplies A, and (r, -w), (alpha, beta) are the scalar pairs of the 2 n-lane k = 2
// product over (C, A_), (C_I, A_).  st[j] = 1 when w and every attribute are below r.
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_pres_prep_kernel(size_t n, size_t nattr, size_t nJ, ac_bbs_order ord, const uint8_t* attr48,
                                                                  const uint8_t* sig97, const uint8_t* rnd, uint8_t* a49, uint8_t* sca, uint8_t* scd,
                                                                  uint8_t* sc2, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t *sig = sig97 + AC_BBS_SIG_BYTES * j, *rn = rnd + 32 * (AC_BBS_PRES_RANDOM + nJ) * j;
#pragma unroll 1
    for (int b = 0; b < 49; ++b) a49[49 * j + b] = sig[b];
    fr w, v;
    bool ok = zp_parse48(w, sig + 49);
    ok = ac_bbs_zp_columns(sca + 32 * j, 32 * n, attr48 + 48 * nattr * j, nattr, ord.at) && ok;
    st[j] = ok ? 1 : 0;
    ac_bbs_pres_random(v, rn, 0); store_be32(sc2 + 32 * j, v);
    ac_bbs_pres_random(v, rn, 1); store_be32(sc2 + 32 * (n + j), v);
    fr_neg(v, w); store_be32(sc2 + 32 * (2 * n + j), v);
    ac_bbs_pres_random(v, rn, 2); store_be32(sc2 + 32 * (3 * n + j), v);
#pragma unroll 1
    for (size_t k = 0; k < nJ; ++k) { ac_bbs_pres_random(v, rn, AC_BBS_PRES_RANDOM + k); store_be32(scd + 32 * (k * n + j), v); }
}

// pres243[j] = A_ | B_ | U (e49 columns) | s | t, u48[nJ j + k] = u_k, status[j] = 0.  Where the reference would throw — A does not decode (st_a),
// w or an attribute >= r (st) — status[j] = 0xff and both records are 0xff bytes; a key that does not decode (st_pub) does that to every lane
// and raises bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) ac_bbs_pres_finish_kernel(size_t n, size_t nattr, size_t nJ, ac_bbs_order ord, const uint8_t* attr48,
                                                                    const uint8_t* sig97, const uint8_t* rnd, const uint8_t* e49, const uint8_t* c32,
                                                                    const uint8_t* st, const uint8_t* st_a, const uint8_t* st_pub, uint8_t* pres243,
                                                                    uint8_t* u48, uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool pub = ac_bbs_pub_ok(st_pub, 3 + nattr);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t *o = pres243 + AC_BBS_FIXED_BYTES * j, *ou = u48 + 48 * nJ * j;
    if (!pub || !st[j] || !st_a[j]) {
#pragma unroll 1
        for (size_t b = 0; b < AC_BBS_FIXED_BYTES; ++b) o[b] = 0xff;
#pragma unroll 1
        for (size_t b = 0; b < 48 * nJ; ++b) ou[b] = 0xff;
        status[j] = 0xff;
        return;
    }
    const uint8_t *rn = rnd + 32 * (AC_BBS_PRES_RANDOM + nJ) * j, *attr = attr48 + 48 * nattr * j;
    uint32_t k8[8];
    fr c_mont, r, alpha, beta, w, negw, s, t, rc_mont;
    words_from_be32(k8, c32 + 32 * j);
    fr_from_words(c_mont, k8);
    ac_bbs_pres_random(r, rn, 0); ac_bbs_pres_random(alpha, rn, 1); ac_bbs_pres_random(beta, rn, 2);
    zp_parse48(w, sig97 + AC_BBS_SIG_BYTES * j + 49);
    fr_neg(negw, w);
    ac_bbs_responses(s, t, rc_mont, c_mont, r, alpha, beta, negw);
#pragma unroll 1
    for (int k = 0; k < 3; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) o[49 * k + b] = e49[49 * (k * n + j) + b];
    store_be48(o + AC_BBS_POINT_BYTES, s);
    store_be48(o + AC_BBS_POINT_BYTES + 48, t);
#pragma unroll 1
    for (size_t k = 0; k < nJ; ++k) {
        fr delta, a, u;
        ac_bbs_pres_random(delta, rn, AC_BBS_PRES_RANDOM + k);
        zp_parse48(a, attr + 48 * ord.at[nattr - nJ + k]);
        ac_bbs_response_u(u, rc_mont, delta, a);
        store_be48(ou + 48 * k, u);
    }
    status[j] = 0;
}

}  // namespace c12381
