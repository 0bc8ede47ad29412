// The AC-rps credential kernels (examples/AC-rps/src/redact.cpp, pres.cpp, verify.cpp of the reference), one credential per lane; the per-lane
// scalar and byte routines are ac_rps.hpp's, ac_rbbs.hpp's and ac_bbs.hpp's:
//   ac_rps_verify_prep_kernel     PresInfo -> the four G1 record columns and tilde_sigma_'s, parse<Zp> range checks, the columns s0, c0 | a_I ..
//   ac_rps_verify_q_kernel        the hashed prefix from the re-encoded points and the q_k columns
//   ac_rps_verify_finish_kernel   ok = [c0 == hash] and both pairing verdicts, or 0xff where the reference would throw
//   ac_rps_pres_prep_kernel       Signature, RedactCache, usk, attributes, randomness -> the record columns, the scalars r | r, t | z, rho | t
//   ac_rps_pres_scalars_kernel    the hashed prefix, the q_k, and the columns of sigma3_'s sum: t q_k, then the exponents e_k of the cross terms
//   ac_rps_pres_finish_kernel     s0 from c0 and the record PresInfo; 0xff where the reference would throw
//   ac_rps_redact_prep_kernel     Signature, attributes -> the record columns and the columns a_I
//   ac_rps_g2_sub_kernel          a - b on the twist: add-the-negative, one complete addition per lane
//   ac_rps_redact_finish_kernel   tilde_H -> the record RedactCache; 0xff where the reference would throw
// api_ac_rps.hip launches them between the library's existing kernels (and k_ac_rbbs.hip's gather and encode, k_ac_bbs.hip's challenge kernel).
// These kernels do byte and hash work, a handful of Zp products per lane; the point arithmetic is the library's.
#include "kernels_common.hpp"
#include "ac_rps.hpp"

using namespace c12381;

namespace {

// q_k, k <= nI, of the lane whose prefix lies at buf, as canonical 32-byte columns q32[32 (k n + j)]
__device__ __forceinline__ void rps_q_columns(const ac_rps_plan& pl, const uint8_t* buf, size_t n, size_t j, uint8_t* q32) {
    const size_t nI = pl.nI;
    uint64_t pre[25];
    ac_rps_q_absorb(pre, buf, nI);
#pragma unroll 1
    for (size_t k = 0; k <= nI; ++k) {
        fr q_mont, q;
        ac_rps_q(q_mont, pre, buf, nI, k < nI ? pl.idx[k] : pl.nattr);
        fr_mont_to_canonical(q, q_mont);
        store_be32(q32 + 32 * (k * n + j), q);
    }
}
__device__ __forceinline__ void rps_fill(uint8_t* o, size_t len) {
#pragma unroll 1
    for (size_t b = 0; b < len; ++b) o[b] = 0xff;
}

}  // namespace

namespace c12381 {

// p49: columns sigma1_, C, sigma3_, sigma2_ of n records; p97: tilde_sigma_.  sc2: columns s0, c0 — the scalars of the k = 2 product over
// (sigma1_, C).  sca[32 (k n + j)]: the disclosed a_idx[k] (attr48 lane-major in the order of idx).  st[j] = 1 when c0 and s0 are below r,
// st_a[j] = 1 when every disclosed value is: the reference reads those only behind the c0 check.
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_verify_prep_kernel(size_t n, size_t nI, const uint8_t* pres389, const uint8_t* attr48, uint8_t* p49,
                                                                    uint8_t* p97, uint8_t* sc2, uint8_t* sca, uint8_t* st, uint8_t* st_a) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* rec = pres389 + AC_RPS_PRES_BYTES * j;
    ac_rps_copy(p49 + 49 * j, rec, 49);                                     // sigma1_
    ac_rps_copy(p49 + 49 * (n + j), rec + 147, 49);                         // C
    ac_rps_copy(p49 + 49 * (2 * n + j), rec + 98, 49);                      // sigma3_
    ac_rps_copy(p49 + 49 * (3 * n + j), rec + 49, 49);                      // sigma2_
    ac_rps_copy(p97 + 97 * j, rec + 196, 97);                               // tilde_sigma_
    fr c0, s0;
    const bool okc = zp_parse48(c0, rec + 293), oks = zp_parse48(s0, rec + 341);
    store_be32(sc2 + 32 * j, s0);
    store_be32(sc2 + 32 * (n + j), c0);
    st[j] = (okc && oks) ? 1 : 0;
    st_a[j] = (nI == 0 || ac_bbs_zp_columns(sca + 32 * j, 32 * n, attr48 + 48 * nI * j, nI, nullptr)) ? 1 : 0;
}

// pre + L j, L = 195 + 56 nI: the prefix of lane j from the encodings of the PARSED sigma1_ (s1_49), sigma2_ (s2_49) and tilde_sigma_ (ts192,
// encoded here), idx and the disclosed fields attr48 (lane-major, in the order of idx); q32: the nI + 1 columns q_k
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_verify_q_kernel(size_t n, ac_rps_plan pl, const uint8_t* s1_49, const uint8_t* s2_49, const uint8_t* ts192,
                                                                 const uint8_t* attr48, uint8_t* pre, uint8_t* q32) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t nI = pl.nI;
    uint8_t* buf = pre + ac_rps_q_prefix_bytes(nI) * j;
    uint8_t ts97[97];
    ac_rps_encode97(ts97, ts192 + 192 * j);
    ac_rps_q_head(buf, s1_49 + 49 * j, s2_49 + 49 * j, ts97, pl.idx, nI);
    if (nI) ac_rps_copy(ac_rps_q_fields(buf, nI), attr48 + 48 * nI * j, 48 * nI);
    rps_q_columns(pl, buf, n, j, q32);
}

// ok[j] = 1 / 0: c0 as parsed (sc2's second column) equals the hash (c32) and both pairing verdicts hold (okp: two columns), or 0xff where the
// reference would throw: c0 or s0 >= r (st), one of the five points not decodable (st_p, five columns), a disclosed value >= r (st_a) — the last
// only behind a matching c0, as the reference returns false before it reads the attributes — or a used key record that does not decode (st_pub,
// npub statuses: every lane, and bad_flag[0] -> C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_verify_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_a,
                                                                      const uint8_t* st_p, const uint8_t* c32, const uint8_t* sc2, const uint8_t* okp, uint8_t* ok,
                                                                      int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    if (!ac_rbbs_all_set(st_pub, npub)) { ok[j] = 0xff; if (j == 0) *bad_flag = 1; return; }
    bool pts = st[j] != 0;
#pragma unroll 1
    for (size_t k = 0; k < 5; ++k) pts = pts && st_p[k * n + j] != 0;
    if (!pts) { ok[j] = 0xff; return; }
    uint8_t diff = 0;
#pragma unroll 1
    for (int b = 0; b < 32; ++b) diff |= c32[32 * j + b] ^ sc2[32 * (n + j) + b];
    if (diff) { ok[j] = 0; return; }
    if (!st_a[j]) { ok[j] = 0xff; return; }
    ok[j] = (okp[j] == 1 && okp[n + j] == 1) ? 1 : 0;
}

// p49: columns h, sigma; p97: columns tilde_M, tilde_H.  scr: r (h^r); sc2: columns r, t (sigma^r sigma1_^t); scz: columns z, rho (one generic
// column of 2 n lanes over sigma1_); sct: t (tilde_g^t).  st[j] = 1 when z and every attribute of the lane's span are below r.
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_pres_prep_kernel(size_t n, size_t nattr, const uint8_t* attr48, const uint8_t* sig195, const uint8_t* cache97,
                                                                  const uint8_t* usk48, const uint8_t* rnd, uint8_t* p49, uint8_t* p97, uint8_t* scr, uint8_t* sc2,
                                                                  uint8_t* scz, uint8_t* sct, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t *sig = sig195 + AC_RPS_SIG_BYTES * j, *rn = rnd + 32 * AC_RPS_PRES_RANDOM * j, *attr = attr48 + 48 * nattr * j;
    ac_rps_copy(p49 + 49 * j, sig, 49);                                     // h
    ac_rps_copy(p49 + 49 * (n + j), sig + 49, 49);                          // sigma
    ac_rps_copy(p97 + 97 * j, sig + 98, 97);                                // tilde_M
    ac_rps_copy(p97 + 97 * (n + j), cache97 + AC_RPS_CACHE_BYTES * j, 97);  // tilde_H
    fr z, v;
    bool ok = zp_parse48(z, usk48 + AC_RPS_USK_BYTES * j);
#pragma unroll 1
    for (size_t k = 0; k < nattr; ++k) ok = zp_parse48(v, attr + 48 * k) && ok;
    st[j] = ok ? 1 : 0;
    ac_bbs_pres_random(v, rn, 0); store_be32(scr + 32 * j, v); store_be32(sc2 + 32 * j, v);
    ac_bbs_pres_random(v, rn, 1); store_be32(sc2 + 32 * (n + j), v); store_be32(sct + 32 * j, v);
    store_be32(scz + 32 * j, z);
    ac_bbs_pres_random(v, rn, 2); store_be32(scz + 32 * (n + j), v);
}

// pre + L j: the prefix of lane j from the encodings just made (s1_49, s2_49, ts97), idx and the disclosed fields picked from the lane's whole span
// attr48; q32: the nI + 1 columns q_k; sc3[32 (p n + j)]: the scalar of list position p — t q_p for p <= nI, then the exponent e_k of the kept
// k = pl.y[p].  A lane with a field >= r computes on the low 32 bytes; its record is discarded (ac_rps_pres_finish_kernel).
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_pres_scalars_kernel(size_t n, ac_rps_plan pl, const uint8_t* s1_49, const uint8_t* s2_49, const uint8_t* ts97,
                                                                     const uint8_t* attr48, const uint8_t* rnd, uint8_t* pre, uint8_t* q32, uint8_t* sc3) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const size_t nI = pl.nI, nattr = pl.nattr;
    const uint8_t* attr = attr48 + 48 * nattr * j;
    uint8_t* buf = pre + ac_rps_q_prefix_bytes(nI) * j;
    ac_rps_q_head(buf, s1_49 + 49 * j, s2_49 + 49 * j, ts97 + 97 * j, pl.idx, nI);
#pragma unroll 1
    for (size_t k = 0; k < nI; ++k) ac_rps_copy(ac_rps_q_fields(buf, nI) + 48 * k, attr + 48 * (size_t)pl.idx[k], 48);
    rps_q_columns(pl, buf, n, j, q32);
    fr t;
    ac_bbs_pres_random(t, rnd + 32 * AC_RPS_PRES_RANDOM * j, 1);
#pragma unroll 1
    for (size_t p = 0; p <= nI; ++p) {
        uint32_t w[8];
        fr q_mont, tq;
        words_from_be32(w, q32 + 32 * (p * n + j));
        fr_from_words(q_mont, w);
        fr_mul(tq, q_mont, t);                           // Montgomery x canonical = canonical
        store_be32(sc3 + 32 * (p * n + j), tq);
    }
#pragma unroll 1
    for (size_t p = nI + 1; p < pl.total; ++p) {
        fr e;
        ac_rps_conv(e, pl.y[p], nattr, pl.idx, nI, pl.in_I, q32 + 32 * j, 32 * n, attr);
        store_be32(sc3 + 32 * (p * n + j), e);
    }
}

// pres389[j] = sigma1_ | sigma2_ | sigma3_ | C | tilde_sigma_ | c0 | s0, status[j] = 0; e49: columns sigma2_, sigma1_, C, C0; s0 = rho + (-c0) z with
// the reference's Zp negation.  Where the reference would throw — h, sigma, tilde_M or tilde_H does not decode (st_p, four columns), z or an attribute
// >= r (st) — status[j] = 0xff and the record is 0xff bytes; a key that does not decode (st_pub, npub statuses) does that to every lane and raises
// bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_pres_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p,
                                                                    const uint8_t* e49, const uint8_t* s3_49, const uint8_t* ts97, const uint8_t* c32,
                                                                    const uint8_t* usk48, const uint8_t* rnd, uint8_t* pres389, uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool pub = ac_rbbs_all_set(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t* o = pres389 + AC_RPS_PRES_BYTES * j;
    bool ok = pub && st[j] != 0;
#pragma unroll 1
    for (size_t k = 0; k < 4; ++k) ok = ok && st_p[k * n + j] != 0;
    if (!ok) {
        rps_fill(o, AC_RPS_PRES_BYTES);
        status[j] = 0xff;
        return;
    }
    uint32_t k8[8];
    fr c_mont, negc, c0, z, rho, zc, s0;
    words_from_be32(k8, c32 + 32 * j);
    fr_from_words(c_mont, k8);
    fr_set_words(c0, k8);
    fr_neg(negc, c_mont);                                // the negative of a Montgomery form is the Montgomery form of the negative
    zp_parse48(z, usk48 + AC_RPS_USK_BYTES * j);
    ac_bbs_pres_random(rho, rnd + 32 * AC_RPS_PRES_RANDOM * j, 2);
    fr_mul(zc, negc, z);
    fr_add(s0, rho, zc);
    ac_rps_copy(o, e49 + 49 * (n + j), 49);
    ac_rps_copy(o + 49, e49 + 49 * j, 49);
    ac_rps_copy(o + 98, s3_49 + 49 * j, 49);
    ac_rps_copy(o + 147, e49 + 49 * (2 * n + j), 49);
    ac_rps_copy(o + 196, ts97 + 97 * j, 97);
    store_be48(o + 293, c0);
    store_be48(o + 341, s0);
    status[j] = 0;
}

// p49: columns h, sigma (decoded for their statuses alone); p97: tilde_M.  sca[32 (k n + j)]: the disclosed a_idx[k], picked from the lane's whole
// span attr48; st[j] = 1 when each of them is below r (the reference's parse is lazy: the hidden fields are never read).
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_redact_prep_kernel(size_t n, size_t nattr, size_t nI, ac_bbs_order idx, const uint8_t* attr48,
                                                                    const uint8_t* sig195, uint8_t* p49, uint8_t* p97, uint8_t* sca, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* sig = sig195 + AC_RPS_SIG_BYTES * j;
    ac_rps_copy(p49 + 49 * j, sig, 49);
    ac_rps_copy(p49 + 49 * (n + j), sig + 49, 49);
    ac_rps_copy(p97 + 97 * j, sig + 98, 97);
    st[j] = (nI == 0 || ac_bbs_zp_columns(sca + 32 * j, 32 * n, attr48 + 48 * nattr * j, nI, idx.at)) ? 1 : 0;
}

// out[i] = a[i] - b[i]: miracl_core::sub is add-the-negative (ECP2_neg, ECP2_add); infinity stays infinity under the negation.  A record off the
// twist marks its lane invalid and raises bad_flag, as g2_add_kernel does.
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_g2_sub_kernel(size_t n, const uint8_t* a192, const uint8_t* b192, uint8_t* out, int fmt, int* bad_flag) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    g2p p, q, inf_pt;
    bool ia, oa, ib, ob;
    g2_parse192(p.x, p.y, ia, oa, a192 + 192 * i); fp2_one(p.z);
    g2_parse192(q.x, q.y, ib, ob, b192 + 192 * i); fp2_one(q.z);
    fp2 ny;
    fp2_neg(ny, q.y); fp2_norm1(q.y, ny);
    g2_set_inf(inf_pt);
    fp2_select(p.x, ia, inf_pt.x, p.x); fp2_select(p.y, ia, inf_pt.y, p.y); fp2_select(p.z, ia, inf_pt.z, p.z);
    fp2_select(q.x, ib, inf_pt.x, q.x); fp2_select(q.y, ib, inf_pt.y, q.y); fp2_select(q.z, ib, inf_pt.z, q.z);
    g2_add(p, q);
    const bool ok = oa && ob;
    if (!ok) *bad_flag = 1;
    g2_store_affine(out + (size_t)fmt * i, p, fmt, !ok);
}

// cache97[j] = tilde_H as encoded (h97), status[j] = 0.  Where the reference would throw — h, sigma or tilde_M does not decode (st_p, three columns),
// a disclosed value >= r (st) — status[j] = 0xff and the record is 0xff bytes; a used key record that does not decode (st_pub, npub statuses) does
// that to every lane and raises bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) ac_rps_redact_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* st_p,
                                                                      const uint8_t* h97, uint8_t* cache97, uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool pub = ac_rbbs_all_set(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t* o = cache97 + AC_RPS_CACHE_BYTES * j;
    if (!pub || !st[j] || !st_p[j] || !st_p[n + j] || !st_p[2 * n + j]) {
        rps_fill(o, AC_RPS_CACHE_BYTES);
        status[j] = 0xff;
        return;
    }
    ac_rps_copy(o, h97 + 97 * j, 97);
    status[j] = 0;
}

}  // namespace c12381
