// The MHAC-bbs credential kernels (examples/MHAC-bbs/src/cred_pres.cpp, verify_pres.cpp of the reference), one presentation per lane; the per-lane
// scalar and byte routines are mhac_bbs.hpp's:
//   mhac_bbs_verify_prep_kernel    Pres, C_rev -> the record columns B_, C_rev, A_, parse<Zp> range checks, the scalar columns -ch, zr, ze | z .., zhp ..
//   mhac_bbs_verify_finish_kernel  the transcript U | A_ | B_ | revealed values over the re-encoded points, c, and ok = [c == ch] and the pairing
//                                  verdict, or 0xff where the reference would throw
//   mhac_bbs_pres_prep_kernel      Creds, PresGroup, PresType, attributes, randomness -> the record columns C_pub, D, A, C_rev, the range checks, the
//                                  scalar columns r, r | alpha, gamma .. | the exponents of the base list
//   mhac_bbs_pres_finish_kernel    the transcript, ch, zr, ze, z, zhp and the records Pres.fixed_part, Pres.z, Pres.z_hid_pub; 0xff where the
//                                  reference would throw
// api_mhac_bbs.hip launches them; the gather of the used h records (ac_bbs_key_kernel), decompression, the fixed-base sums, the k-way products,
// the G1 column, additions, affine conversions and the pairing half (c12381_ps_verify_batch_dev) are the library's existing kernels.
#include "kernels_common.hpp"
#include "mhac_bbs.hpp"

using namespace c12381;

namespace {

// st_pub: the decoding statuses of g1, g2, (w,) and the used h records
__device__ __forceinline__ bool mhac_bbs_pub_ok(const uint8_t* st_pub, size_t npub) {
    bool pub = true;
#pragma unroll 1
    for (size_t i = 0; i < npub; ++i) pub = pub && st_pub[i] != 0;
    return pub;
}
__device__ __forceinline__ void copy49(uint8_t* dst, const uint8_t* src) {
#pragma unroll 1
    for (int b = 0; b < 49; ++b) dst[b] = src[b];
}
// every one of `count` consecutive 48-byte fields is below r
__device__ __forceinline__ bool fields_ok(const uint8_t* f48, size_t count) {
    bool ok = true;
#pragma unroll 1
    for (size_t k = 0; k < count; ++k) { fr v; ok = zp_parse48(v, f48 + 48 * k) && ok; }
    return ok;
}

}  // namespace

namespace c12381 {

// p49: columns B_, C_rev, A_ of n records — the terms of the k = 3 product in its order.  sc3: its scalars -ch (the Zp negation), zr, ze.
// sca[32 (k n + j)]: the scalar of base k of the verify list — z[ii] (k < nz), then zhp[ii].  c32[j] = ch.  st[j] = 1 when every Zp field of the lane
// (ch, zr, ze, z, zhp, the nrp revealed values) is below r.
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_verify_prep_kernel(size_t n, size_t nz, size_t nhp, size_t nrp, const uint8_t* crev49,
                                                                      const uint8_t* fixed242, const uint8_t* z48, const uint8_t* zhp48,
                                                                      const uint8_t* pub48, uint8_t* p49, uint8_t* sc3, uint8_t* sca, uint8_t* c32,
                                                                      uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* rec = fixed242 + MHAC_BBS_FIXED_BYTES * j;
    copy49(p49 + 49 * j, rec + 49);
    copy49(p49 + 49 * (n + j), crev49 + 49 * j);
    copy49(p49 + 49 * (2 * n + j), rec);
    fr ch, nch;
    bool ok = zp_parse48(ch, rec + 98);
    store_be32(c32 + 32 * j, ch);
    fr_neg(nch, ch);
    store_be32(sc3 + 32 * j, nch);
    ok = ac_bbs_zp_columns(sc3 + 32 * (n + j), 32 * n, rec + 146, 2, nullptr) && ok;
    if (nz) ok = ac_bbs_zp_columns(sca + 32 * j, 32 * n, z48 + 48 * nz * j, nz, nullptr) && ok;
    if (nhp) ok = ac_bbs_zp_columns(sca + 32 * (nz * n + j), 32 * n, zhp48 + 48 * nhp * j, nhp, nullptr) && ok;
    if (nrp) ok = fields_ok(pub48 + 48 * nrp * j, nrp) && ok;
    st[j] = ok ? 1 : 0;
}

// ok[j] = 1 / 0: [ SHA3-512(U | A_ | B_ | revealed) mod r == ch ] and the pairing verdict okp[j]; p96: the decoded columns B_, C_rev, A_ (the
// transcript hashes their re-encodings), u49[j] = U compressed, tr + L j: the lane's transcript, L = 147 + 48 nrp.  0xff where the reference would
// throw: a Zp field >= r (st), A_ / B_ / C_rev not decodable (st_p, three columns), or a public record that does not decode (st_pub, npub
// statuses: every lane, and bad_flag[0] -> C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_verify_finish_kernel(size_t n, size_t nrp, size_t npub, const uint8_t* st_pub, const uint8_t* st,
                                                                        const uint8_t* st_p, const uint8_t* p96, const uint8_t* u49,
                                                                        const uint8_t* pub48, const uint8_t* c32, const uint8_t* okp, uint8_t* tr,
                                                                        uint8_t* ok, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    if (!mhac_bbs_pub_ok(st_pub, npub)) { ok[j] = 0xff; if (j == 0) *bad_flag = 1; return; }
    if (!st[j] || !st_p[j] || !st_p[n + j] || !st_p[2 * n + j]) { ok[j] = 0xff; return; }
    uint8_t a49[49], b49[49];
    ac_bbs_encode49(b49, p96 + 96 * j);
    ac_bbs_encode49(a49, p96 + 96 * (2 * n + j));
    const size_t L = mhac_bbs_transcript_bytes(nrp);
    uint8_t* t = tr + L * j;
    mhac_bbs_transcript(t, u49 + 49 * j, a49, b49, pub48 + 48 * nrp * j, nrp, nullptr);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, t, L);
    fr_mont_to_canonical(c, c_mont);
    uint8_t got[32], diff = 0;
    store_be32(got, c);
#pragma unroll 1
    for (int b = 0; b < 32; ++b) diff |= got[b] ^ c32[32 * j + b];
    ok[j] = (okp[j] == 1 && diff == 0) ? 1 : 0;
}

// p49: columns C_pub, D, A, C_rev.  scr: the columns r, r of the 2 n-lane G1 column over (C_pub * D | A).  scu: the t + 1 columns alpha, gamma[0] ..
// gamma[t - 1] of the per-lane powers of C_rev, A_ .. A_.  sch[32 (k n + j)]: the exponent of position k of the pres list — bj[ii] (k < nHid), then
// b[y] (y < (t - 1) nPrv).  st[j] = 1 when lambda, e_share, a_share and every public value are below r.
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_pres_prep_kernel(size_t n, size_t t, mhac_bbs_sets s, const uint8_t* A49, const uint8_t* D49,
                                                                    const uint8_t* crev49, const uint8_t* cpub49, const uint8_t* lam48,
                                                                    const uint8_t* eshare48, const uint8_t* ashare48, const uint8_t* pub48,
                                                                    const uint8_t* rnd, uint8_t* p49, uint8_t* scr, uint8_t* scu, uint8_t* sch,
                                                                    uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    copy49(p49 + 49 * j, cpub49 + 49 * j);
    copy49(p49 + 49 * (n + j), D49 + 49 * j);
    copy49(p49 + 49 * (2 * n + j), A49 + 49 * j);
    copy49(p49 + 49 * (3 * n + j), crev49 + 49 * j);
    bool ok = fields_ok(lam48 + 48 * t * j, t);
    ok = fields_ok(eshare48 + 48 * t * j, t) && ok;
    if (s.nPrv) ok = fields_ok(ashare48 + 48 * t * s.nPrv * j, t * s.nPrv) && ok;
    if (s.nPub) ok = fields_ok(pub48 + 48 * (size_t)s.nPub * j, s.nPub) && ok;
    st[j] = ok ? 1 : 0;
    const uint8_t* rn = rnd + 32 * mhac_bbs_rnd_count(s, t) * j;
    fr v;
    ac_bbs_pres_random(v, rn, 0); store_be32(scr + 32 * j, v); store_be32(scr + 32 * (n + j), v);
    ac_bbs_pres_random(v, rn, 1); store_be32(scu + 32 * j, v);
#pragma unroll 1
    for (size_t k = 0; k < t; ++k) { ac_bbs_pres_random(v, rn, mhac_bbs_rnd_gamma(s, t, k)); store_be32(scu + 32 * ((k + 1) * n + j), v); }
#pragma unroll 1
    for (size_t ii = 0; ii < s.nHid; ++ii) { ac_bbs_pres_random(v, rn, mhac_bbs_rnd_betaj(s, t, ii)); store_be32(sch + 32 * (ii * n + j), v); }
#pragma unroll 1
    for (size_t y = 0; y < (t - 1) * s.nPrv; ++y) { ac_bbs_pres_random(v, rn, mhac_bbs_rnd_beta(s, y)); store_be32(sch + 32 * ((s.nHid + y) * n + j), v); }
}

// fixed242[j] = A_ | B_ | ch | zr | ze, z48[nPrv j + ii], zhp48[nHidPub j + ii], status[j] = 0.  o96: the columns B_, A_ (the G1 column's output), u96: U.
// Where the reference would throw — A, D, C_rev or C_pub does not decode (st_p, four columns), a Zp field >= r (st) — status[j] = 0xff and the three
// records are 0xff bytes; a public record that does not decode (st_pub) does that to every lane and raises bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) mhac_bbs_pres_finish_kernel(size_t n, size_t t, mhac_bbs_sets s, size_t npub, const uint8_t* st_pub,
                                                                      const uint8_t* st, const uint8_t* st_p, const uint8_t* o96, const uint8_t* u96,
                                                                      const uint8_t* lam48, const uint8_t* eshare48, const uint8_t* ashare48,
                                                                      const uint8_t* pub48, const uint8_t* rnd, uint8_t* tr, uint8_t* fixed242,
                                                                      uint8_t* z48, uint8_t* zhp48, uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool pub = mhac_bbs_pub_ok(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t *o = fixed242 + MHAC_BBS_FIXED_BYTES * j, *oz = z48 + 48 * (size_t)s.nPrv * j, *ohp = zhp48 + 48 * (size_t)s.nHidPub * j;
    if (!pub || !st[j] || !st_p[j] || !st_p[n + j] || !st_p[2 * n + j] || !st_p[3 * n + j]) {
#pragma unroll 1
        for (size_t b = 0; b < MHAC_BBS_FIXED_BYTES; ++b) o[b] = 0xff;
#pragma unroll 1
        for (size_t b = 0; b < 48 * (size_t)s.nPrv; ++b) oz[b] = 0xff;
#pragma unroll 1
        for (size_t b = 0; b < 48 * (size_t)s.nHidPub; ++b) ohp[b] = 0xff;
        status[j] = 0xff;
        return;
    }
    uint8_t u49[49];
    ac_bbs_encode49(o, o96 + 96 * (n + j));
    ac_bbs_encode49(o + 49, o96 + 96 * j);
    ac_bbs_encode49(u49, u96 + 96 * j);
    const uint8_t* pa = pub48 + 48 * (size_t)s.nPub * j;
    const size_t L = mhac_bbs_transcript_bytes(s.nRevPub);
    uint8_t* tl = tr + L * j;
    mhac_bbs_transcript(tl, u49, o, o + 49, pa, s.nRevPub, s.revpub);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, tl, L);
    fr_mont_to_canonical(c, c_mont);
    store_be48(o + 98, c);
    mhac_bbs_responses(s, t, c_mont, rnd + 32 * mhac_bbs_rnd_count(s, t) * j, lam48 + 48 * t * j, eshare48 + 48 * t * j,
                       ashare48 + 48 * t * s.nPrv * j, pa, o + 146, o + 194, oz, ohp);
    status[j] = 0;
}

}  // namespace c12381
