// The MHAC-bbs issuance kernels (examples/MHAC-bbs/src/generate_attributes.cpp, cred_iss.cpp, make_pres_group.cpp, make_pres_type.cpp of the
// reference); the per-lane scalar routines, the base lists and the rnd offsets are mhac_iss.hpp's.  attr and iss run one (credential, party) pair
// per lane, lane = credential x nparties + party; group and type one presentation per lane:
//   mhac_iss_attr_kernel          randomness -> the public attributes, the shares (records and the scalar columns of the commitments' sum)
//   mhac_iss_attr_finish_kernel   0xff over every output and the bad flag where a public record does not decode
//   mhac_iss_iss_prep_kernel      sk, the public values, randomness -> gamma, e, the range checks, e_share (record and -e_share as a scalar), the
//                                 columns lambda and pub_a
//   mhac_iss_cols_kernel          the decoded C[0] .. C[t-1] of every credential as the term columns of the k-way products
//   mhac_iss_rep_kernel           A once per party of its credential
//   mhac_iss_iss_finish_kernel    the records A, D, the status, 0xff where the reference would throw, the bad flags
//   mhac_iss_group_prep_kernel    the D records of S as columns, lambda as records and as scalar columns, the gather of the rows of S
//   mhac_iss_group_finish_kernel  the record D, the status, 0xff where a D record of S does not decode
//   mhac_iss_type_prep_kernel     the range check of the public span and the columns of the type list
//   mhac_iss_type_finish_kernel   the records C_rev, C_pub, the status, 0xff, the bad flag
// api_mhac_iss.hip launches them; decompression, the fixed-base sums, the k-way products, the G1 columns, additions and the simultaneous inversion
// are the library's existing kernels.
#include "kernels_common.hpp"
#include "mhac_iss.hpp"

using namespace c12381;

namespace {

__device__ __forceinline__ bool mhac_iss_pub_ok(const uint8_t* st_pub, size_t npub) {
    bool pub = true;
#pragma unroll 1
    for (size_t i = 0; i < npub; ++i) pub = pub && st_pub[i] != 0;
    return pub;
}
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, size_t count) {
#pragma unroll 1
    for (size_t b = 0; b < count; ++b) dst[b] = src[b];
}
__device__ __forceinline__ void fill_ff(uint8_t* dst, size_t count) {
#pragma unroll 1
    for (size_t b = 0; b < count; ++b) dst[b] = 0xff;
}
// one 96-byte record, both 16-byte aligned
__device__ __forceinline__ void copy96(uint8_t* dst, const uint8_t* src) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = s[i];
}

}  // namespace

namespace c12381 {

// L = k np lanes.  rnd: mhac_iss_attr_rnd_count scalars per credential.  pub48[nPub j + q] = attr[Pub[q]] (party 0's lane writes it),
// ashare48[nPrv lane + ii] = share[party][ii], sc[32 (ii L + lane)] the same value as the exponent of h[Prv[ii]].  s: the sets of (m, Prv, {}), whose
// hidpub is Pub ascending.
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_attr_kernel(size_t k, size_t np, size_t t, mhac_bbs_sets s, const uint8_t* rnd, uint8_t* pub48,
                                                               uint8_t* ashare48, uint8_t* sc) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, L = k * np;
    if (lane >= L) return;
    const size_t j = lane / np, p = lane % np, nPrv = s.nPrv, nPub = s.nPub;
    const uint8_t* rn = rnd + 32 * mhac_iss_attr_rnd_count(s.m, nPrv, t) * j;
#pragma unroll 1
    for (size_t ii = 0; ii < nPrv; ++ii) {
        fr a0, share;
        ac_bbs_pres_random(a0, rn, s.prv[ii]);
        mhac_iss_polynomial_rnd(share, (uint32_t)(p + 1), a0, rn, mhac_iss_attr_rnd_coeff(s.m, t, ii), t - 1);
        store_be48(ashare48 + 48 * (nPrv * lane + ii), share);
        store_be32(sc + 32 * (ii * L + lane), share);
    }
    if (p == 0) {
#pragma unroll 1
        for (size_t q = 0; q < nPub; ++q) {
            fr a;
            ac_bbs_pres_random(a, rn, s.hidpub[q]);
            store_be48(pub48 + 48 * (nPub * j + q), a);
        }
    }
}
// A pp or used h record that does not decode (st_pub, npub statuses): every output byte 0xff and bad_flag[0] (C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_attr_finish_kernel(size_t L, size_t np, size_t nPrv, size_t nPub, size_t npub, const uint8_t* st_pub,
                                                                      uint8_t* pub48, uint8_t* ashare48, uint8_t* C49, int* bad_flag) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (lane >= L || mhac_iss_pub_ok(st_pub, npub)) return;
    if (lane == 0) *bad_flag = 1;
    fill_ff(C49 + 49 * lane, 49);
    fill_ff(ashare48 + 48 * nPrv * lane, 48 * nPrv);
    if (lane % np == 0) fill_ff(pub48 + 48 * nPub * (lane / np), 48 * nPub);
}

// L = k np lanes.  rnd: e, then the t - 1 coefficients, per credential.  eshare48[lane] = polynomial(party + 1, e, a), nes[lane] its Zp negation as a
// scalar.  Party 0's lane: e32[j] = e, scl[32 (i k + j)] = lambda_i, scp[32 (ii k + j)] = pub_a[ii], st[j] = 1 when every public value is below r.
// Lane 0: gam = gamma as 32 bytes, gam[32] = 1 when sk is below r; otherwise bad_flag[2] (C12381_E_ARG).
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_iss_prep_kernel(size_t k, size_t np, size_t t, size_t nPub, mhac_iss_lambda lam, const uint8_t* sk48,
                                                                   const uint8_t* pub48, const uint8_t* rnd, uint8_t* gam, uint8_t* st, uint8_t* e32,
                                                                   uint8_t* scl, uint8_t* scp, uint8_t* nes, uint8_t* eshare48, int* bad_flag) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (lane >= k * np) return;
    const size_t j = lane / np, p = lane % np;
    const uint8_t* rn = rnd + 32 * mhac_iss_iss_rnd_count(t) * j;
    fr e, es, neg;
    ac_bbs_pres_random(e, rn, 0);
    mhac_iss_polynomial_rnd(es, (uint32_t)(p + 1), e, rn, mhac_iss_iss_rnd_coeff(), t - 1);
    store_be48(eshare48 + 48 * lane, es);
    fr_neg(neg, es);
    store_be32(nes + 32 * lane, neg);
    if (p == 0) {
        store_be32(e32 + 32 * j, e);
#pragma unroll 1
        for (size_t i = 0; i < t; ++i) {
            fr l;
            fr_set_words(l, lam.w[i]);
            store_be32(scl + 32 * (i * k + j), l);
        }
        st[j] = (nPub == 0 || ac_bbs_zp_columns(scp + 32 * j, 32 * k, pub48 + 48 * nPub * j, nPub, nullptr)) ? 1 : 0;
    }
    if (lane == 0) {
        fr g;
        const bool ok = zp_parse48(g, sk48);
        store_be32(gam, g);
        gam[32] = ok ? 1 : 0;
        if (!ok) bad_flag[2] = 1;
    }
}
// q96[i k + j] = c96[j np + i] for i < t: term column i of the products
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_cols_kernel(size_t k, size_t np, size_t t, const uint8_t* c96, uint8_t* q96) {
    const size_t idx = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= t * k) return;
    const size_t i = idx / k, j = idx % k;
    copy96(q96 + 96 * idx, c96 + 96 * (j * np + i));
}
// r96[lane] = a96[lane / np]
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_rep_kernel(size_t L, size_t np, const uint8_t* a96, uint8_t* r96) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (lane >= L) return;
    copy96(r96 + 96 * lane, a96 + 96 * (lane / np));
}
// D49[lane] = w96[lane] encoded; party 0's lane: A49[j], status[j] = 0.  Where the reference would throw — one of the credential's nparties C records
// does not decode (st_c), a public value >= r (st) — the credential's A, e_share, D are 0xff bytes and status[j] = 0xff.  sk >= r (gam[32] = 0) and a
// public record that does not decode (st_pub: bad_flag[0], C12381_E_POINT) do that to every credential.
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_iss_finish_kernel(size_t L, size_t np, size_t npub, const uint8_t* st_pub, const uint8_t* gam,
                                                                     const uint8_t* st, const uint8_t* st_c, const uint8_t* a96, const uint8_t* w96,
                                                                     uint8_t* A49, uint8_t* eshare48, uint8_t* D49, uint8_t* status, int* bad_flag) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (lane >= L) return;
    const size_t j = lane / np, p = lane % np;
    const bool pub = mhac_iss_pub_ok(st_pub, npub);
    if (!pub && lane == 0) *bad_flag = 1;
    bool ok = pub && gam[32] && st[j];
#pragma unroll 1
    for (size_t i = 0; i < np; ++i) ok = ok && st_c[j * np + i] != 0;
    if (ok) {
        ac_bbs_encode49(D49 + 49 * lane, w96 + 96 * lane);
        if (p == 0) { ac_bbs_encode49(A49 + 49 * j, a96 + 96 * j); status[j] = 0; }
    } else {
        fill_ff(D49 + 49 * lane, 49);
        fill_ff(eshare48 + 48 * lane, 48);
        if (p == 0) { fill_ff(A49 + 49 * j, 49); status[j] = 0xff; }
    }
}

// Per presentation j: p49[k n + j] = D_share[S[k]] of its credential, sc[32 (k n + j)] = lambda[k], lam48[t j + k] the same as a record; eS48[t j + k] =
// eshare48[np j + S[k]] and aS48[(t j + k) nPrv ..] = ashare48[(np j + S[k]) nPrv ..] copied verbatim (each pair may be null).  Parties outside S are
// not read.
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_group_prep_kernel(size_t n, size_t np, size_t t, size_t nPrv, mhac_iss_parties_set S, mhac_iss_lambda lam,
                                                                     const uint8_t* D49, const uint8_t* eshare48, const uint8_t* ashare48, uint8_t* p49,
                                                                     uint8_t* sc, uint8_t* lam48, uint8_t* eS48, uint8_t* aS48) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
#pragma unroll 1
    for (size_t k = 0; k < t; ++k) {
        const size_t row = np * j + S.at[k];
        copy_bytes(p49 + 49 * (k * n + j), D49 + 49 * row, 49);
        fr l;
        fr_set_words(l, lam.w[k]);
        store_be32(sc + 32 * (k * n + j), l);
        store_be48(lam48 + 48 * (t * j + k), l);
        if (eS48) copy_bytes(eS48 + 48 * (t * j + k), eshare48 + 48 * row, 48);
        if (aS48) copy_bytes(aS48 + 48 * nPrv * (t * j + k), ashare48 + 48 * nPrv * row, 48 * nPrv);
    }
}
// Dg49[j] = u96[j] encoded, status[j] = 0; where a D record of S does not decode (st_p, t columns) status[j] = 0xff and the presentation's D, lambda
// and gathered rows are 0xff bytes
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_group_finish_kernel(size_t n, size_t t, size_t nPrv, const uint8_t* st_p, const uint8_t* u96, uint8_t* Dg49,
                                                                       uint8_t* lam48, uint8_t* eS48, uint8_t* aS48, uint8_t* status) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    bool ok = true;
#pragma unroll 1
    for (size_t k = 0; k < t; ++k) ok = ok && st_p[k * n + j] != 0;
    if (ok) { ac_bbs_encode49(Dg49 + 49 * j, u96 + 96 * j); status[j] = 0; return; }
    fill_ff(Dg49 + 49 * j, 49);
    fill_ff(lam48 + 48 * t * j, 48 * t);
    if (eS48) fill_ff(eS48 + 48 * t * j, 48 * t);
    if (aS48) fill_ff(aS48 + 48 * nPrv * t * j, 48 * nPrv * t);
    status[j] = 0xff;
}

// sca[32 (k n + j)] = pub_a[at[k]] for the nb = nPub positions of the type list (a permutation of the span); st[j] = 1 when every value is below r
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_type_prep_kernel(size_t n, size_t nPub, mhac_iss_type_plan plan, const uint8_t* pub48, uint8_t* sca,
                                                                    uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    st[j] = (nPub == 0 || ac_bbs_zp_columns(sca + 32 * j, 32 * n, pub48 + 48 * nPub * j, nPub, plan.at)) ? 1 : 0;
}
// crev49[j], cpub49[j] = r96[j], p96[j] encoded, status[j] = 0; a public value >= r (st): both records 0xff and status[j] = 0xff; a public record that
// does not decode (st_pub): every lane, and bad_flag[0] (C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) mhac_iss_type_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* st, const uint8_t* r96,
                                                                      const uint8_t* p96, uint8_t* crev49, uint8_t* cpub49, uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool pub = mhac_iss_pub_ok(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    if (pub && st[j]) {
        ac_bbs_encode49(crev49 + 49 * j, r96 + 96 * j);
        ac_bbs_encode49(cpub49 + 49 * j, p96 + 96 * j);
        status[j] = 0;
    } else {
        fill_ff(crev49 + 49 * j, 49);
        fill_ff(cpub49 + 49 * j, 49);
        status[j] = 0xff;
    }
}

}  // namespace c12381
