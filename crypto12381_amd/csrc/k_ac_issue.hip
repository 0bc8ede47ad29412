// The AC issuance kernels (examples/AC-bbs/src/issue.cpp, AC-rbbs/src/issue.cpp, AC-rps/src/issue.cpp, user_keygen.cpp of the reference), one
// credential per lane; the per-lane scalar routines are ac_issue.hpp's:
//   ac_issue_bbs_prep_kernel       sk, attributes, rnd -> the attribute columns, w, x + w, the parse status; sk >= r raises bad_flag[2]
//   ac_issue_bbs_finish_kernel     Signature = A | w; 0xff where the reference would throw, the bad flag where a key record does not decode
//   ac_issue_keygen_prep_kernel    rnd -> usk as the scalar of g
//   ac_issue_keygen_finish_kernel  usk as a record; 0xff over both outputs and the bad flag where pk.fixed_part does not decode
//   ac_issue_rps_prep_kernel       sk, attributes, rnd -> the attribute columns, alpha, x + ym | alpha y^(nattr+1), the parse status
//   ac_issue_rps_finish_kernel     Signature = h | sigma | tilde_M; 0xff where the reference would throw, the bad flags
// api_ac_issue.hip launches them between the library's existing kernels (decompression, the fixed-base sums, the simultaneous inversion, the G1
// column, the k = 2 product, k_ac_rbbs.hip's encode).  These kernels do byte work and a handful of Zp products per lane — nattr + 2 for AC-rps —;
// the point arithmetic is the library's.  sk is read here, on the device, by every lane: 48 or 96 bytes from one address.
#include "kernels_common.hpp"
#include "ac_issue.hpp"

using namespace c12381;

namespace {

__device__ __forceinline__ void issue_fill(uint8_t* o, size_t len) {
#pragma unroll 1
    for (size_t b = 0; b < len; ++b) o[b] = 0xff;
}

}  // namespace

namespace c12381 {

// nsk: the fields of sk (AC-bbs 1: x; AC-rbbs 2: x, y — y is range-checked and not used).  sca[32 (i n + j)] = a_i, w32[j] = rnd mod r,
// d32[j] = x + w.  st[j] = 1 when every attribute of the lane is below r.  Lane 0: a field of sk >= r raises bad_flag[2] (C12381_E_ARG).
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_bbs_prep_kernel(size_t n, size_t nattr, size_t nsk, const uint8_t* sk48, const uint8_t* attr48,
                                                                   const uint8_t* rnd32, uint8_t* sca, uint8_t* w32, uint8_t* d32, uint8_t* st,
                                                                   int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    const bool sk_ok = ac_issue_sk(sk, sk48, nsk);
    if (j == 0 && !sk_ok) bad_flag[2] = 1;
    st[j] = ac_issue_bbs_lane(sca + 32 * j, 32 * n, w32 + 32 * j, d32 + 32 * j, sk[0], attr48 + 48 * nattr * j, nattr, rnd32 + 32 * j) ? 1 : 0;
}

// sig97[j] = a96[j] encoded | w as a 48-byte field, status[j] = 0.  An attribute >= r (st): the record is 0xff bytes and status[j] = 0xff.  A field
// of sk >= r, or g, tilde_g, tilde_X or a used Y record that does not decode (st_pub, npub statuses: bad_flag[0], C12381_E_POINT): every lane.
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_bbs_finish_kernel(size_t n, size_t npub, size_t nsk, const uint8_t* st_pub, const uint8_t* sk48,
                                                                     const uint8_t* st, const uint8_t* a96, const uint8_t* w32, uint8_t* sig97,
                                                                     uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    const bool sk_ok = ac_issue_sk(sk, sk48, nsk), pub = ac_rbbs_all_set(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t* o = sig97 + AC_BBS_SIG_BYTES * j;
    if (!pub || !sk_ok || !st[j]) {
        issue_fill(o, AC_BBS_SIG_BYTES);
        status[j] = 0xff;
        return;
    }
    ac_bbs_encode49(o, a96 + 96 * j);
#pragma unroll 1
    for (int b = 0; b < 16; ++b) o[49 + b] = 0;
    ac_rps_copy(o + 65, w32 + 32 * j, 32);
    status[j] = 0;
}

// sc[32 j] = usk = rnd mod r
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_keygen_prep_kernel(size_t n, const uint8_t* rnd32, uint8_t* sc) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr usk;
    ac_issue_random(usk, rnd32 + 32 * j);
    store_be32(sc + 32 * j, usk);
}
// usk48[j] = sc[j] as a 48-byte field; upk49[j] holds g^usk already.  g, tilde_g or tilde_X does not decode (st_pub, 3 statuses): both outputs are
// 0xff bytes on every lane and bad_flag[0] (C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_keygen_finish_kernel(size_t n, const uint8_t* st_pub, const uint8_t* sc, uint8_t* usk48, uint8_t* upk49,
                                                                        int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    uint8_t* o = usk48 + AC_ISSUE_USK_BYTES * j;
    if (!ac_rbbs_all_set(st_pub, 3)) {
        if (j == 0) *bad_flag = 1;
        issue_fill(o, AC_ISSUE_USK_BYTES);
        issue_fill(upk49 + AC_ISSUE_UPK_BYTES * j, AC_ISSUE_UPK_BYTES);
        return;
    }
#pragma unroll 1
    for (int b = 0; b < 16; ++b) o[b] = 0;
    ac_rps_copy(o + 16, sc + 32 * j, 32);
}

// sca[32 (i n + j)] = a_i, al32[j] = alpha = rnd mod r, sc2: columns x + ym, alpha y^(nattr+1) — the scalars of the k = 2 product over (h, Z).
// st[j] = 1 when every attribute of the lane is below r.  Lane 0: x or y >= r raises bad_flag[2] (C12381_E_ARG).
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_rps_prep_kernel(size_t n, size_t nattr, const uint8_t* sk96, const uint8_t* attr48, const uint8_t* rnd32,
                                                                   uint8_t* sca, uint8_t* al32, uint8_t* sc2, uint8_t* st, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    const bool sk_ok = ac_issue_sk(sk, sk96, AC_ISSUE_RPS_SK_FIELDS);
    if (j == 0 && !sk_ok) bad_flag[2] = 1;
    st[j] = ac_issue_rps_lane(sca + 32 * j, 32 * n, al32 + 32 * j, sc2 + 32 * j, sc2 + 32 * (n + j), sk[0], sk[1], attr48 + 48 * nattr * j, nattr,
                              rnd32 + 32 * j) ? 1 : 0;
}

// sig195[j] = h | sigma (e49: two columns) | tilde_M (tm97), status[j] = 0.  An attribute >= r (st) or a upk that does not decode (st_z): the record
// is 0xff bytes and status[j] = 0xff.  x or y >= r, or g, tilde_g, tilde_X or a used tilde_Y record that does not decode (st_pub, npub statuses:
// bad_flag[0], C12381_E_POINT): every lane.
__global__ void __launch_bounds__(BLOCK, 2) ac_issue_rps_finish_kernel(size_t n, size_t npub, const uint8_t* st_pub, const uint8_t* sk96, const uint8_t* st,
                                                                     const uint8_t* st_z, const uint8_t* e49, const uint8_t* tm97, uint8_t* sig195,
                                                                     uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    const bool sk_ok = ac_issue_sk(sk, sk96, AC_ISSUE_RPS_SK_FIELDS), pub = ac_rbbs_all_set(st_pub, npub);
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t* o = sig195 + AC_RPS_SIG_BYTES * j;
    if (!pub || !sk_ok || !st[j] || !st_z[j]) {
        issue_fill(o, AC_RPS_SIG_BYTES);
        status[j] = 0xff;
        return;
    }
    ac_rps_copy(o, e49 + 49 * j, 49);
    ac_rps_copy(o + 49, e49 + 49 * (n + j), 49);
    ac_rps_copy(o + 98, tm97 + 97 * j, 97);
    status[j] = 0;
}

}  // namespace c12381
