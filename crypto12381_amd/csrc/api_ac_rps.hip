// The AC-rps credential entries of the C ABI (include/c12381_ac.h): redaction caches, presentations and their verification, from the wire formats
// of the reference's examples/AC-rps.  Kernels: k_ac_rps.hip (and k_ac_rbbs.hip's gather and encode, k_ac_bbs.hip's challenge); the per-lane
// scalar work, the q_k hashes and the base list: ac_rps.hpp; the shared host pieces: host.hpp.
#include "host.hpp"

#include "../../include/c12381_ac.h"
#include "ac_rps.hpp"

using namespace c12381;
using namespace c12381_host;

static_assert(AC_RPS_LIST_MAX == C12381_G1_FIXED_SUM_MAX, "the base list of verify and pres: one fixed-base table per position");
static_assert(AC_BBS_MAX_ATTR <= C12381_G2_FIXED_SUM_MAX, "the G2 sums of verify and redact take up to nattr bases");
static_assert(AC_RPS_LIST_MAX <= sizeof(ac_bbs_order::at), "the base list travels to the gather kernel as an ac_bbs_order");
constexpr size_t AC_RPS_CHUNK = (size_t)1 << 18;

static ac_bbs_order rps_order(const uint8_t* at, size_t count) {
    ac_bbs_order o = {};
    for (size_t k = 0; k < count; ++k) o.at[k] = at[k];
    return o;
}

// ---------------------------------------------------------------- verify (verify.cpp:6-38)
// The used key records — Y[nattr - Ip[k]] for k <= nI (the base list of ac_rps.hpp), tilde_Y[idx[k]] for k < nI and tilde_Y[nattr] — are gathered
// and decoded on the side stream with g, tilde_g and tilde_X; the reference's parse of pk.Y / pk.tilde_Y is lazy, so no other record is read.
// Per presentation: split and range-check (ac_rps_verify_prep_kernel), decode the five points, C0 = sigma1_^s0 C^c0 as ONE k = 2 product, the
// re-encoded sigma1_, C, sigma2_ (ac_rbbs_encode_kernel), c0's hash (ac_bbs_challenge_kernel with no message), the q_k (ac_rps_verify_q_kernel),
// S by the G1 fixed-base sum, W = tilde_X + sum_I a_i tilde_Y[i] by the G2 fixed-base sum plus tilde_sigma_ by one addition per lane, then five
// Miller values — the running-point loop for (S, tilde_sigma_) and (sigma1_, W), whose G2 argument is per lane and unchecked; the line tables for
// (sigma3_, tilde_g), (sigma2_, tilde_g) and (C, tilde_Y[nattr]) — joined as the reference's header joins them: left side, conjugate of the right
// side, multiply, one final exponentiation, is_unity, both equations as one column of 2 m lanes; and the verdict (ac_rps_verify_finish_kernel).
static int ac_rps_verify_args(size_t nattr, size_t nI, const uint32_t* idx, const void* pk, const void* Y, const void* tY, const void* pres, const void* attr,
                              const void* ok, ac_rps_plan& p) {
    if ((nI && !idx) || !ac_rps_pres_plan(p, nattr, idx, nI, false)) return C12381_E_ARG;
    return (!pk || !Y || !tY || !pres || !ok || (nI && !attr)) ? C12381_E_ARG : 0;
}
int c12381_ac_rps_verify_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                   const uint8_t* tY_97, const uint8_t* pres_389, const uint8_t* attr_48, uint8_t* ok) {
    ac_rps_plan pl;
    int rc = bind(c) ?: ac_rps_verify_args(nattr, nI, idx, pk_243, Y_49, tY_97, pres_389, attr_48, ok, pl);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_RPS_CHUNK ? n : AC_RPS_CHUNK, nb = nI + 1;
    if ((rc = ensure(c, c12381_ctx::WS_AC_RPS, ac_rps_verify_layout(nullptr, ch, nI).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_RPS];
    const ac_rps_public pub(d);
    const ac_bbs_order list = rps_order(pl.y, nb);
    ac_bbs_order tlist = rps_order(pl.idx, nI);
    tlist.at[nI] = (uint8_t)nattr;
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_243, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pk_243 + 49, pub.g2, pub.st + 1, 0);
    LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(49 * nb)), dim3(BLOCK), c->side, nb, (size_t)49, list, Y_49, pub.y49);
    LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(97 * nb)), dim3(BLOCK), c->side, nb, (size_t)97, tlist, tY_97, pub.ty97);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nb, (const uint8_t*)pub.y49, pub.l96, pub.st + 3, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nb, (const uint8_t*)pub.ty97, pub.ty192, pub.st + 3 + nb, 0);
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_rps_verify_slab s = ac_rps_verify_layout(d, m, nI);
        uint8_t *S96 = s.a96, *s1_96 = s.a96 + 96 * m, *C96 = s.a96 + 192 * m, *s3_96 = s.a96 + 288 * m, *s2_96 = s.a96 + 384 * m;
        uint8_t *ts192 = s.q192, *W192 = s.q192 + 192 * m;
        const uint8_t* attr = nI ? attr_48 + 48 * nI * off : attr_48;
        LAUNCH(c, ac_rps_verify_prep_kernel, m, m, nI, pres_389 + 389 * off, attr, s.p49, s.p97, s.sc2, s.sca, s.st, s.st_a);
        LAUNCH(c, g1_decompress_kernel, 4 * m, 4 * m, s.p49, s1_96, s.st_p, 0);
        LAUNCH(c, g2_decompress_kernel, m, m, s.p97, ts192, s.st_p + 4 * m, 0);
        if ((rc = c12381_g1_mul_sum_batch_dev(c, m, 2, s1_96, s.sc2, s.e49 + 98 * m, 49, 0u))) return rc;                      // C0
        LAUNCH(c, ac_rbbs_encode_kernel, m, m, (size_t)2, (const uint8_t*)s1_96, s.e49);                                      // sigma1_, C
        LAUNCH(c, ac_rbbs_encode_kernel, m, m, (size_t)1, (const uint8_t*)s2_96, s.e49 + 147 * m);                            // sigma2_
        LAUNCH(c, ac_bbs_challenge_kernel, m, m, (size_t)0, (const uint8_t*)s.e49, (const uint8_t*)s.e49, s.tr, s.c32);
        LAUNCH(c, ac_rps_verify_q_kernel, m, m, pl, (const uint8_t*)s.e49, (const uint8_t*)(s.e49 + 147 * m), (const uint8_t*)ts192, attr, s.pre, s.q32);
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = g1_fixed_sum_range(c, m, nb, 0, nb, pub.l96, nullptr, s.q32, S96, 96))) return rc;                          // S
        if (nI) {
            if ((rc = g2_fixed_sum_range(c, m, nI, 0, nI, pub.ty192, pub.g2 + 192, s.sca, s.w192, 192))) return rc;
            LAUNCH(c, g2_add_kernel, m, m, (const uint8_t*)s.w192, (size_t)192, (const uint8_t*)ts192, W192, 192, c->d_flag, (const int32_t*)nullptr);
        } else {
            LAUNCH(c, g2_add_kernel, m, m, (const uint8_t*)(pub.g2 + 192), (size_t)0, (const uint8_t*)ts192, W192, 192, c->d_flag, (const int32_t*)nullptr);
        }
        // Miller values, 576 bytes each: gt slot 0 is kept for the left side of the first equation, 1 | 2 = (sigma3_, tilde_g) | (sigma2_, tilde_g),
        // 3 | 4 = (S, tilde_sigma_) | (sigma1_, W); ge = (C, tilde_Y[nattr])
        uint8_t *v0 = s.gt, *v1 = s.gt + 576 * m, *v2 = s.gt + 2 * 576 * m, *v3 = s.gt + 3 * 576 * m, *v4 = s.gt + 4 * 576 * m;
        if ((rc = c12381_pair_product_fixed_g2_batch_dev(c, m, 1, C96, pub.ty192 + 192 * nI, s.ge, C12381_F_MILLER_ONLY))) return rc;
        if ((rc = c12381_pair_product_fixed_g2_batch_dev(c, 2 * m, 1, s3_96, pub.g2, v1, C12381_F_MILLER_ONLY))) return rc;
        if ((rc = c12381_miller_batch_dev(c, 2 * m, S96, s.q192, v3))) return rc;
        if ((rc = c12381_gt_op_batch_dev(c, 0, m, v4, s.ge, v0))) return rc;                 // e(sigma1_, W) e(C, tilde_Y[nattr]) | (sigma3_, tilde_g)
        if ((rc = c12381_gt_op_batch_dev(c, 1, 2 * m, v2, nullptr, s.gh))) return rc;        // conjugates of (sigma2_, tilde_g) | (S, tilde_sigma_)
        if ((rc = c12381_gt_op_batch_dev(c, 0, 2 * m, v0, s.gh, v2))) return rc;
        if ((rc = c12381_gt_op_batch_dev(c, 3, 2 * m, v2, nullptr, s.gh))) return rc;
        if ((rc = c12381_gt_is_unity_batch_dev(c, 2 * m, s.gh, s.okp))) return rc;
        LAUNCH(c, ac_rps_verify_finish_kernel, m, m, 3 + 2 * nb, (const uint8_t*)pub.st, (const uint8_t*)s.st, (const uint8_t*)s.st_a, (const uint8_t*)s.st_p,
               (const uint8_t*)s.c32, (const uint8_t*)s.sc2, (const uint8_t*)s.okp, ok + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rps_verify_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                               const uint8_t* tY_97, const uint8_t* pres_389, const uint8_t* attr_48, uint8_t* ok) {
    ac_rps_plan pl;
    int rc = bind(c) ?: ac_rps_verify_args(nattr, nI, idx, pk_243, Y_49, tY_97, pres_389, attr_48, ok, pl);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {Y_49, 49 * (2 * nattr + 1)}, {tY_97, 97 * (nattr + 1)}, {pres_389, 389 * n}, {nI ? attr_48 : nullptr, 48 * nI * n}},
                     {{ok, n}}, [&](const staging& s) {
        return c12381_ac_rps_verify_batch_dev(c, n, nattr, nI, idx, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.out[0]);
    });
}

// ---------------------------------------------------------------- pres (pres.cpp:8-62)
// The reference materialises pk.Y: all 2 nattr + 1 records are decoded on the side stream, with g, tilde_g and tilde_X, and the base list of the plan
// (ac_rps.hpp) is gathered from them.  Per presentation: the records and the scalars (ac_rps_pres_prep_kernel), decode h, sigma, tilde_M, tilde_H,
// sigma1_ = h^r by the generic column, sigma2_ = sigma^r sigma1_^t as ONE k = 2 product, C | C0 = sigma1_^z | sigma1_^rho as one generic column of
// 2 m lanes, tilde_sigma_ = tilde_g^t (the fixed G2 base) + tilde_H, the q_k and the scalar columns of sigma3_ (ac_rps_pres_scalars_kernel), sigma3_
// as ONE sum over the whole list through g1_fixed_sum_range — its first nI + 1 positions are verify's list, so the two entries share those
// tables — c0 (ac_bbs_challenge_kernel with no message), s0 and the record (ac_rps_pres_finish_kernel).
static int ac_rps_pres_args(size_t nattr, size_t nI, const uint32_t* idx, const void* pk, const void* Y, const void* attr, const void* sig, const void* cache,
                            const void* usk, const void* rnd, const void* pres, const void* status, ac_rps_plan& p) {
    if ((nI && !idx) || !ac_rps_pres_plan(p, nattr, idx, nI, true)) return C12381_E_ARG;
    return (!pk || !Y || !attr || !sig || !cache || !usk || !rnd || !pres || !status) ? C12381_E_ARG : 0;
}
int c12381_ac_rps_pres_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                 const uint8_t* attr_48, const uint8_t* sig_195, const uint8_t* cache_97, const uint8_t* usk_48, const uint8_t* rnd,
                                 uint8_t* pres_389, uint8_t* status) {
    ac_rps_plan pl;
    int rc = bind(c) ?: ac_rps_pres_args(nattr, nI, idx, pk_243, Y_49, attr_48, sig_195, cache_97, usk_48, rnd, pres_389, status, pl);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_RPS_CHUNK ? n : AC_RPS_CHUNK, total = pl.total, nY = 2 * nattr + 1;
    if ((rc = ensure(c, c12381_ctx::WS_AC_RPS, ac_rps_pres_layout(nullptr, ch, nI, total).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_RPS];
    const ac_rps_public pub(d);
    const ac_bbs_order list = rps_order(pl.y, total);
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_243, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pk_243 + 49, pub.g2, pub.st + 1, 0);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nY, Y_49, pub.y96, pub.st + 3, 0);
    LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(96 * total)), dim3(BLOCK), c->side, total, (size_t)96, list, (const uint8_t*)pub.y96, pub.l96);
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_rps_pres_slab s = ac_rps_pres_layout(d, m, nI, total);
        const uint8_t *attr = attr_48 + 48 * nattr * off, *usk = usk_48 + 48 * off, *rn = rnd + 32 * AC_RPS_PRES_RANDOM * off;
        uint8_t *h96 = s.a96, *sg96 = s.a96 + 96 * m, *s1_96 = s.a96 + 192 * m;
        uint8_t *e_s2 = s.e49, *e_s1 = s.e49 + 49 * m, *e_c = s.e49 + 98 * m;
        LAUNCH(c, ac_rps_pres_prep_kernel, m, m, nattr, attr, sig_195 + 195 * off, cache_97 + 97 * off, usk, rn, s.p49, s.p97, s.scr, s.sc2, s.scz, s.sct, s.st);
        LAUNCH(c, g1_decompress_kernel, 2 * m, 2 * m, s.p49, h96, s.st_p, 0);
        LAUNCH(c, g2_decompress_kernel, 2 * m, 2 * m, s.p97, s.m192, s.st_p + 2 * m, 0);
        if ((rc = c12381_g1_mul_batch_dev(c, m, h96, s.scr, s1_96, 96))) return rc;                                          // sigma1_
        if ((rc = c12381_g1_mul_sum_batch_dev(c, m, 2, sg96, s.sc2, e_s2, 49, 0u))) return rc;                                // sigma2_
        LAUNCH(c, ac_rbbs_encode_kernel, m, m, (size_t)1, (const uint8_t*)s1_96, e_s1);
        HIPCK(c, hipMemcpyAsync(s.b96, s1_96, 96 * m, hipMemcpyDeviceToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(s.b96 + 96 * m, s1_96, 96 * m, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = c12381_g1_mul_batch_dev(c, 2 * m, s.b96, s.scz, e_c, 49))) return rc;                                       // C | C0
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = c12381_g2_mul_fixed_batch_dev(c, m, pub.g2, s.sct, s.t192, 192))) return rc;                                // tilde_g^t
        LAUNCH(c, g2_add_kernel, m, m, (const uint8_t*)s.t192, (size_t)192, (const uint8_t*)(s.m192 + 192 * m), s.ts97, 97, c->d_flag, (const int32_t*)nullptr);
        LAUNCH(c, ac_rps_pres_scalars_kernel, m, m, pl, (const uint8_t*)e_s1, (const uint8_t*)e_s2, (const uint8_t*)s.ts97, attr, rn, s.pre, s.q32, s.sc3);
        if ((rc = g1_fixed_sum_range(c, m, total, 0, total, pub.l96, nullptr, s.sc3, s.s3_49, 49))) return rc;                 // sigma3_
        LAUNCH(c, ac_bbs_challenge_kernel, m, m, (size_t)0, (const uint8_t*)e_s1, (const uint8_t*)e_s1, s.tr, s.c32);
        LAUNCH(c, ac_rps_pres_finish_kernel, m, m, 3 + nY, (const uint8_t*)pub.st, (const uint8_t*)s.st, (const uint8_t*)s.st_p, (const uint8_t*)s.e49,
               (const uint8_t*)s.s3_49, (const uint8_t*)s.ts97, (const uint8_t*)s.c32, usk, rn, pres_389 + 389 * off, status + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rps_pres_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                             const uint8_t* attr_48, const uint8_t* sig_195, const uint8_t* cache_97, const uint8_t* usk_48, const uint8_t* rnd,
                             uint8_t* pres_389, uint8_t* status) {
    ac_rps_plan pl;
    int rc = bind(c) ?: ac_rps_pres_args(nattr, nI, idx, pk_243, Y_49, attr_48, sig_195, cache_97, usk_48, rnd, pres_389, status, pl);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {Y_49, 49 * (2 * nattr + 1)}, {attr_48, 48 * nattr * n}, {sig_195, 195 * n}, {cache_97, 97 * n}, {usk_48, 48 * n},
                         {rnd, 32 * AC_RPS_PRES_RANDOM * n}}, {{pres_389, 389 * n}, {status, n}}, [&](const staging& s) {
        return c12381_ac_rps_pres_batch_dev(c, n, nattr, nI, idx, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.out[0], s.out[1]);
    });
}

// ---------------------------------------------------------------- redact (redact.cpp:6-16)
// The nI used records tilde_Y[idx[k]] are gathered and decoded on the side stream — the positions of verify's G2 sum, so the two entries share those
// tables; the reference parses neither pk.fixed_part nor any other record.  Per credential: the records and the columns a_I
// (ac_rps_redact_prep_kernel), decode h, sigma (for their statuses alone) and tilde_M, the G2 fixed-base sum with no addend, tilde_M minus it
// (ac_rps_g2_sub_kernel; nI = 0: minus infinity, tilde_M re-encoded) and the record (ac_rps_redact_finish_kernel).
static int ac_rps_redact_args(size_t nattr, size_t nI, const uint32_t* idx, const void* tY, const void* attr, const void* sig, const void* cache, const void* status,
                              ac_bbs_order& o) {
    if ((nI && !idx) || !ac_bbs_base_order(o, nattr, idx, nI)) return C12381_E_ARG;
    return (!tY || !attr || !sig || !cache || !status) ? C12381_E_ARG : 0;
}
int c12381_ac_rps_redact_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* tY_97, const uint8_t* attr_48,
                                   const uint8_t* sig_195, uint8_t* cache_97, uint8_t* status) {
    ac_bbs_order ord;
    int rc = bind(c) ?: ac_rps_redact_args(nattr, nI, idx, tY_97, attr_48, sig_195, cache_97, status, ord);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_RPS_CHUNK ? n : AC_RPS_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_AC_RPS, ac_rps_redact_layout(nullptr, ch, nI).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_RPS];
    const ac_rps_public pub(d);
    if (nI) {
        if ((rc = fork_side(c))) return rc;
        LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(97 * nI)), dim3(BLOCK), c->side, nI, (size_t)97, ord, tY_97, pub.ty97);
        LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nI, (const uint8_t*)pub.ty97, pub.ty192, pub.st, 0);
    }
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_rps_redact_slab s = ac_rps_redact_layout(d, m, nI);
        LAUNCH(c, ac_rps_redact_prep_kernel, m, m, nattr, nI, ord, attr_48 + 48 * nattr * off, sig_195 + 195 * off, s.p49, s.p97, s.sca, s.st);
        LAUNCH(c, g1_decompress_kernel, 2 * m, 2 * m, s.p49, s.a96, s.st_p, 0);
        LAUNCH(c, g2_decompress_kernel, m, m, s.p97, s.m192, s.st_p + 2 * m, 0);
        if (nI) {
            if (off == 0 && (rc = join_side(c))) return rc;
            if ((rc = g2_fixed_sum_range(c, m, nI, 0, nI, pub.ty192, nullptr, s.sca, s.w192, 192))) return rc;
        } else {
            HIPCK(c, hipMemsetAsync(s.w192, 0, 192 * m, c->stream));
        }
        LAUNCH(c, ac_rps_g2_sub_kernel, m, m, (const uint8_t*)s.m192, (const uint8_t*)s.w192, s.h97, 97, c->d_flag);
        LAUNCH(c, ac_rps_redact_finish_kernel, m, m, nI, (const uint8_t*)pub.st, (const uint8_t*)s.st, (const uint8_t*)s.st_p, (const uint8_t*)s.h97,
               cache_97 + 97 * off, status + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rps_redact_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* tY_97, const uint8_t* attr_48,
                               const uint8_t* sig_195, uint8_t* cache_97, uint8_t* status) {
    ac_bbs_order ord;
    int rc = bind(c) ?: ac_rps_redact_args(nattr, nI, idx, tY_97, attr_48, sig_195, cache_97, status, ord);
    if (rc || n == 0) return rc;
    return host_form(c, {{tY_97, 97 * (nattr + 1)}, {attr_48, 48 * nattr * n}, {sig_195, 195 * n}}, {{cache_97, 97 * n}, {status, n}},
                     [&](const staging& s) { return c12381_ac_rps_redact_batch_dev(c, n, nattr, nI, idx, s.in[0], s.in[1], s.in[2], s.out[0], s.out[1]); });
}
