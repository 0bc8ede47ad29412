// The MHAC-bbs credential entries of the C ABI (include/c12381_mhac.h): verification of multi-holder presentations and their creation, from the wire
// formats of the reference's examples/MHAC-bbs.  Kernels: k_mhac_bbs.hip (and ac_bbs_key_kernel of k_ac_bbs.hip for the gather of the used h
// records); the per-lane scalar work, the index sets and the base lists: mhac_bbs.hpp; the shared host pieces: host.hpp.
#include "host.hpp"

#include "../../include/c12381_mhac.h"
#include "mhac_bbs.hpp"

using namespace c12381;
using namespace c12381_host;

static_assert(MHAC_BBS_MAX_ATTR == C12381_G1_FIXED_SUM_MAX, "one fixed-base table per position of a base list");
static_assert(MHAC_BBS_T_MAX == C12381_MHAC_T_MAX, "the public bound of t");
constexpr size_t MHAC_BBS_CHUNK = (size_t)1 << 18;

// The index sets of the batch and the entry's base list (nb positions of h: mhac_bbs_verify_list / mhac_bbs_pres_list)
struct mhac_bbs_plan { mhac_bbs_sets s; ac_bbs_order list; size_t nb; };
static int mhac_bbs_set_args(size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, mhac_bbs_plan& p) {
    return ((nPrv && !prv) || (nRev && !rev) || !mhac_bbs_derive(p.s, m, prv, nPrv, rev, nRev)) ? C12381_E_ARG : 0;
}
// pp, pk and the used h records on the side stream: g1 and g2 are decoded where they lie in pp, w (verify alone: pk_97 is null in pres) from pk, the
// h records after the gather into the base list; the caller joins the side stream before its first use of them.  Returns the number of statuses.
static int mhac_bbs_pub(c12381_ctx* c, const mhac_bbs_plan& p, const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* pk_97, const ac_bbs_public& pub,
                        size_t& npub) {
    int rc;
    if ((rc = fork_side(c))) return rc;
    size_t k = 0;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pp_146, pub.g96, pub.st + k++, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pp_146 + 49, pub.g2, pub.st + k++, 0);
    if (pk_97) LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_97, pub.g2 + 192, pub.st + k++, 0);
    if (p.nb) {
        LAUNCH_ON(c, ac_bbs_key_kernel, dim3(grid_for(49 * p.nb)), dim3(BLOCK), c->side, p.nb, p.list, h_49, pub.y49);
        LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, p.nb, (const uint8_t*)pub.y49, pub.y96, pub.st + k, 0);
    }
    npub = k + p.nb;
    return 0;
}

// ---------------------------------------------------------------- verify (verify_pres.cpp:6-46)
// Per presentation: split and range-check (mhac_bbs_verify_prep_kernel), decode B_, C_rev, A_, R = B_^(-ch) C_rev^zr A_^ze as ONE k = 3 product under
// one doubling chain (-ch the Zp negation, on B_ itself), C_hid by the fixed-base sum over the verify list, U = R + C_hid compressed, the pairing
// half as c12381_ps_verify_batch_dev with no messages (g2, X2 = w, s1 = A_, s2 = B_; its generic route serves a w outside G2), then the transcript,
// c and the verdict (mhac_bbs_verify_finish_kernel).  Batches run in chunks of MHAC_BBS_CHUNK.
static int mhac_bbs_verify_args(size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const void* pp, const void* h, const void* pk,
                                const void* crev, const void* fixed, const void* z, const void* zhp, const void* pub, const void* ok, mhac_bbs_plan& p) {
    int rc = mhac_bbs_set_args(m, nPrv, prv, nRev, rev, p);
    if (rc) return rc;
    p.nb = mhac_bbs_verify_list(p.list, p.s);
    return (!pp || !h || !pk || !crev || !fixed || !ok || (p.s.nPrv && !z) || (p.s.nHidPub && !zhp) || (p.s.nRevPub && !pub)) ? C12381_E_ARG : 0;
}
int c12381_mhac_bbs_verify_batch_dev(c12381_ctx* c, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                                     const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* pk_97, const uint8_t* crev_49, const uint8_t* fixed_242,
                                     const uint8_t* z_48, const uint8_t* zhp_48, const uint8_t* pub_48, uint8_t* ok) {
    mhac_bbs_plan p;
    int rc = bind(c) ?: mhac_bbs_verify_args(m, nPrv, prv, nRev, rev, pp_146, h_49, pk_97, crev_49, fixed_242, z_48, zhp_48, pub_48, ok, p);
    if (rc || n == 0) return rc;
    const size_t ch = n < MHAC_BBS_CHUNK ? n : MHAC_BBS_CHUNK, nz = p.s.nPrv, nhp = p.s.nHidPub, nrp = p.s.nRevPub, nb = p.nb;
    if ((rc = ensure(c, c12381_ctx::WS_MHAC_BBS, mhac_bbs_verify_layout(nullptr, ch, nb, nrp).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_MHAC_BBS];
    const ac_bbs_public pub(d);
    size_t npub;
    if ((rc = mhac_bbs_pub(c, p, pp_146, h_49, pk_97, pub, npub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t k = n - off < ch ? n - off : ch;
        const mhac_bbs_verify_slab s = mhac_bbs_verify_layout(d, k, nb, nrp);
        const uint8_t* pa = nrp ? pub_48 + 48 * nrp * off : pub_48;
        LAUNCH(c, mhac_bbs_verify_prep_kernel, k, k, nz, nhp, nrp, crev_49 + 49 * off, fixed_242 + MHAC_BBS_FIXED_BYTES * off,
               nz ? z_48 + 48 * nz * off : z_48, nhp ? zhp_48 + 48 * nhp * off : zhp_48, pa, s.p49, s.sc3, s.sca, s.c32, s.st);
        LAUNCH(c, g1_decompress_kernel, 3 * k, 3 * k, s.p49, s.p96, s.st_p, 0);
        const uint8_t *B96 = s.p96, *A96 = s.p96 + 192 * k;
        if ((rc = c12381_g1_mul_sum_batch_dev(c, k, 3, s.p96, s.sc3, nb ? s.r96 : s.u49, nb ? 96 : 49, 0u))) return rc;       // R
        if (off == 0 && (rc = join_side(c))) return rc;
        if (nb) {
            if ((rc = g1_fixed_sum_range(c, k, nb, 0, nb, pub.y96, nullptr, s.sca, s.s96, 96))) return rc;                     // C_hid
            if ((rc = ac_bbs_add(c, k, s.r96, s.s96, s.u49, 49))) return rc;
        }
        if ((rc = c12381_ps_verify_batch_dev(c, k, 0, pub.g2, pub.g2 + 192, nullptr, A96, B96, nullptr, s.okp))) return rc;
        LAUNCH(c, mhac_bbs_verify_finish_kernel, k, k, nrp, npub, pub.st, s.st, s.st_p, s.p96, s.u49, pa, s.c32, s.okp, s.tr, ok + off, c->d_flag);
    }
    return 0;
}
int c12381_mhac_bbs_verify_batch(c12381_ctx* c, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const uint8_t* pp_146,
                                 const uint8_t* h_49, const uint8_t* pk_97, const uint8_t* crev_49, const uint8_t* fixed_242, const uint8_t* z_48,
                                 const uint8_t* zhp_48, const uint8_t* pub_48, uint8_t* ok) {
    mhac_bbs_plan p;
    int rc = bind(c) ?: mhac_bbs_verify_args(m, nPrv, prv, nRev, rev, pp_146, h_49, pk_97, crev_49, fixed_242, z_48, zhp_48, pub_48, ok, p);
    if (rc || n == 0) return rc;
    const size_t nz = p.s.nPrv, nhp = p.s.nHidPub, nrp = p.s.nRevPub;
    return host_form(c, {{pp_146, 146}, {h_49, 49 * m}, {pk_97, 97}, {crev_49, 49 * n}, {fixed_242, MHAC_BBS_FIXED_BYTES * n}, {nz ? z_48 : nullptr, 48 * nz * n},
                         {nhp ? zhp_48 : nullptr, 48 * nhp * n}, {nrp ? pub_48 : nullptr, 48 * nrp * n}}, {{ok, n}}, [&](const staging& s) {
        return c12381_mhac_bbs_verify_batch_dev(c, n, m, nPrv, prv, nRev, rev, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.in[7], s.out[0]);
    });
}

// ---------------------------------------------------------------- pres (cred_pres.cpp:6-113, j = 0)
// Per presentation: the records, the range checks and the scalar columns (mhac_bbs_pres_prep_kernel), decode C_pub, D, A, C_rev, C_pub * D, then
// B_ = (C_pub * D)^r and A_ = A^r as ONE G1 column of 2 m lanes; the t + 1 per-lane powers C_rev^alpha, A_^gamma[0] .. A_^gamma[t - 1] — each a multiply
// of its own, A_ is an unchecked point — as products of at most C12381_G1_MUL_SUM_MAX terms joined by additions; the h terms as ONE fixed-base sum over
// the pres list, which holds exactly the reference's terms (a repeated base keeps its positions: the sum merges nothing on the generic route); then
// the transcript, ch, the responses and the records (mhac_bbs_pres_finish_kernel).
static int mhac_bbs_pres_args(size_t m, size_t t, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const void* pp, const void* h,
                              const void* A, const void* D, const void* lam, const void* eshare, const void* ashare, const void* crev, const void* cpub,
                              const void* pub, const void* rnd, const void* fixed, const void* z, const void* zhp, const void* status, mhac_bbs_plan& p) {
    int rc = mhac_bbs_set_args(m, nPrv, prv, nRev, rev, p);
    if (rc) return rc;
    if (t == 0 || t > MHAC_BBS_T_MAX || mhac_bbs_pres_list_len(p.s, t) > MHAC_BBS_MAX_ATTR) return C12381_E_ARG;
    p.nb = mhac_bbs_pres_list(p.list, p.s, t);
    return (!pp || !h || !A || !D || !lam || !eshare || !crev || !cpub || !rnd || !fixed || !status || (p.s.nPrv && (!ashare || !z)) || (p.s.nPub && !pub) ||
            (p.s.nHidPub && !zhp)) ? C12381_E_ARG : 0;
}
int c12381_mhac_bbs_pres_batch_dev(c12381_ctx* c, size_t n, size_t m, size_t t, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                                   const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* A_49, const uint8_t* D_49, const uint8_t* lam_48,
                                   const uint8_t* eshare_48, const uint8_t* ashare_48, const uint8_t* crev_49, const uint8_t* cpub_49, const uint8_t* pub_48,
                                   const uint8_t* rnd, uint8_t* fixed_242, uint8_t* z_48, uint8_t* zhp_48, uint8_t* status) {
    mhac_bbs_plan p;
    int rc = bind(c) ?: mhac_bbs_pres_args(m, t, nPrv, prv, nRev, rev, pp_146, h_49, A_49, D_49, lam_48, eshare_48, ashare_48, crev_49, cpub_49, pub_48, rnd,
                                           fixed_242, z_48, zhp_48, status, p);
    if (rc || n == 0) return rc;
    const size_t ch = n < MHAC_BBS_CHUNK ? n : MHAC_BBS_CHUNK, nz = p.s.nPrv, nhp = p.s.nHidPub, nPub = p.s.nPub, nrp = p.s.nRevPub, total = p.nb;
    const size_t nrnd = mhac_bbs_rnd_count(p.s, t), nA = t < 4 ? t : 4;
    if ((rc = ensure(c, c12381_ctx::WS_MHAC_BBS, mhac_bbs_pres_layout(nullptr, ch, t, total, nrp).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_MHAC_BBS];
    const ac_bbs_public pub(d);
    size_t npub;
    if ((rc = mhac_bbs_pub(c, p, pp_146, h_49, nullptr, pub, npub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t k = n - off < ch ? n - off : ch;
        const mhac_bbs_pres_slab s = mhac_bbs_pres_layout(d, k, t, total, nrp);
        const uint8_t *lam = lam_48 + 48 * t * off, *es = eshare_48 + 48 * t * off, *as = nz ? ashare_48 + 48 * t * nz * off : ashare_48;
        const uint8_t *pa = nPub ? pub_48 + 48 * nPub * off : pub_48, *rn = rnd + 32 * nrnd * off;
        LAUNCH(c, mhac_bbs_pres_prep_kernel, k, k, t, p.s, A_49 + 49 * off, D_49 + 49 * off, crev_49 + 49 * off, cpub_49 + 49 * off, lam, es, as, pa, rn,
               s.p49, s.scr, s.scu, s.sch, s.st);
        LAUNCH(c, g1_decompress_kernel, 4 * k, 4 * k, s.p49, s.p96, s.st_p, 0);
        // p96: C_pub | D | A | C_rev; C_pub * D takes D's place, so that (C_pub * D | A) ^ (r | r) = (B_ | A_) is one column of 2 k lanes
        uint8_t *CD = s.p96 + 96 * k, *A_ = s.o96 + 96 * k;
        if ((rc = ac_bbs_add(c, k, s.p96, CD, CD, 96))) return rc;
        if ((rc = c12381_g1_mul_batch_dev(c, 2 * k, CD, s.scr, s.o96, 96))) return rc;
        // q96: C_rev | A_ x nA — product 0 takes the columns from C_rev, every later one columns of A_ alone; scu: alpha | gamma[0] ..
        HIPCK(c, hipMemcpyAsync(s.q96, s.p96 + 288 * k, 96 * k, hipMemcpyDeviceToDevice, c->stream));
        for (size_t i = 0; i < nA; ++i) HIPCK(c, hipMemcpyAsync(s.q96 + 96 * k * (1 + i), A_, 96 * k, hipMemcpyDeviceToDevice, c->stream));
        for (size_t first = 0; first < t + 1; first += C12381_G1_MUL_SUM_MAX) {
            const size_t kk = t + 1 - first < C12381_G1_MUL_SUM_MAX ? t + 1 - first : C12381_G1_MUL_SUM_MAX;
            if ((rc = c12381_g1_mul_sum_batch_dev(c, k, (int)kk, first ? s.q96 + 96 * k : s.q96, s.scu + 32 * k * first, first ? s.v96 : s.u96, 96, 0u))) return rc;
            if (first && (rc = ac_bbs_add(c, k, s.u96, s.v96, s.u96, 96))) return rc;
        }
        if (off == 0 && (rc = join_side(c))) return rc;
        if (total) {
            if ((rc = g1_fixed_sum_range(c, k, total, 0, total, pub.y96, nullptr, s.sch, s.v96, 96))) return rc;
            if ((rc = ac_bbs_add(c, k, s.u96, s.v96, s.u96, 96))) return rc;
        }
        LAUNCH(c, mhac_bbs_pres_finish_kernel, k, k, t, p.s, npub, pub.st, s.st, s.st_p, s.o96, s.u96, lam, es, as, pa, rn, s.tr,
               fixed_242 + MHAC_BBS_FIXED_BYTES * off, nz ? z_48 + 48 * nz * off : z_48, nhp ? zhp_48 + 48 * nhp * off : zhp_48, status + off, c->d_flag);
    }
    return 0;
}
int c12381_mhac_bbs_pres_batch(c12381_ctx* c, size_t n, size_t m, size_t t, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                               const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* A_49, const uint8_t* D_49, const uint8_t* lam_48,
                               const uint8_t* eshare_48, const uint8_t* ashare_48, const uint8_t* crev_49, const uint8_t* cpub_49, const uint8_t* pub_48,
                               const uint8_t* rnd, uint8_t* fixed_242, uint8_t* z_48, uint8_t* zhp_48, uint8_t* status) {
    mhac_bbs_plan p;
    int rc = bind(c) ?: mhac_bbs_pres_args(m, t, nPrv, prv, nRev, rev, pp_146, h_49, A_49, D_49, lam_48, eshare_48, ashare_48, crev_49, cpub_49, pub_48, rnd,
                                           fixed_242, z_48, zhp_48, status, p);
    if (rc || n == 0) return rc;
    const size_t nz = p.s.nPrv, nhp = p.s.nHidPub, nPub = p.s.nPub;
    return host_form(c, {{pp_146, 146}, {h_49, 49 * m}, {A_49, 49 * n}, {D_49, 49 * n}, {lam_48, 48 * t * n}, {eshare_48, 48 * t * n},
                         {nz ? ashare_48 : nullptr, 48 * t * nz * n}, {crev_49, 49 * n}, {cpub_49, 49 * n}, {nPub ? pub_48 : nullptr, 48 * nPub * n},
                         {rnd, 32 * mhac_bbs_rnd_count(p.s, t) * n}},
                     {{fixed_242, MHAC_BBS_FIXED_BYTES * n}, {z_48, 48 * nz * n}, {zhp_48, 48 * nhp * n}, {status, n}}, [&](const staging& s) {
        return c12381_mhac_bbs_pres_batch_dev(c, n, m, t, nPrv, prv, nRev, rev, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.in[7], s.in[8],
                                              s.in[9], s.in[10], s.out[0], s.out[1], s.out[2], s.out[3]);
    });
}
