// The MHAC-bbs issuance entries of the C ABI (include/c12381_mhac.h): generate_attributes, cred_iss, make_pres_group and make_pres_type of the
// reference's examples/MHAC-bbs from their wire formats — everything that produces the inputs of c12381_mhac_bbs_pres_batch.  Kernels:
// k_mhac_iss.hip (and ac_bbs_key_kernel, ac_bbs_bcast96_kernel of k_ac_bbs.hip); polynomial, the Lagrange coefficients, the base lists and the rnd
// offsets: mhac_iss.hpp; the shared host pieces: host.hpp.  lambda is a constant of the batch: computed once here, on the host, and passed by value.
#include "host.hpp"

#include "../../include/c12381_mhac.h"
#include "mhac_iss.hpp"

using namespace c12381;
using namespace c12381_host;

static_assert(MHAC_ISS_PARTIES_MAX == C12381_MHAC_PARTIES_MAX, "the public bound of nparties");
static_assert(MHAC_BBS_T_MAX == C12381_MHAC_T_MAX && MHAC_BBS_MAX_ATTR == C12381_G1_FIXED_SUM_MAX, "the public bounds of t and m");
constexpr size_t MHAC_ISS_CHUNK = (size_t)1 << 18;

// pp and the nb used h records (the entry's base list) on the side stream: g1 and g2 decoded where they lie in pp, the h records after the gather;
// the caller joins the side stream before its first use of them.  npub: the number of statuses at pub.st
static int mhac_iss_pub(c12381_ctx* c, const ac_bbs_order& list, size_t nb, const uint8_t* pp_146, const uint8_t* h_49, const ac_bbs_public& pub, size_t& npub) {
    int rc;
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pp_146, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pp_146 + 49, pub.g2, pub.st + 1, 0);
    if (nb) {
        LAUNCH_ON(c, ac_bbs_key_kernel, dim3(grid_for(49 * nb)), dim3(BLOCK), c->side, nb, list, h_49, pub.y49);
        LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nb, (const uint8_t*)pub.y49, pub.y96, pub.st + 2, 0);
    }
    npub = 2 + nb;
    return 0;
}
// out[j] = prod_(i < t) pts[i k + j]^sc[i k + j]: each power a multiply of its own, in products of at most C12381_G1_MUL_SUM_MAX terms joined by
// additions (tmp: one further point per lane)
static int mhac_iss_powers(c12381_ctx* c, size_t k, size_t t, const uint8_t* pts96, const uint8_t* sc, uint8_t* out96, uint8_t* tmp96) {
    int rc;
    for (size_t first = 0; first < t; first += C12381_G1_MUL_SUM_MAX) {
        const size_t kk = t - first < C12381_G1_MUL_SUM_MAX ? t - first : C12381_G1_MUL_SUM_MAX;
        if ((rc = c12381_g1_mul_sum_batch_dev(c, k, (int)kk, pts96 + 96 * k * first, sc + 32 * k * first, first ? tmp96 : out96, 96, 0u))) return rc;
        if (first && (rc = ac_bbs_add(c, k, out96, tmp96, out96, 96))) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------- attr (generate_attributes.cpp:6-37)
// Per (credential, party) lane: the shares as records and as the nPrv scalar columns (mhac_iss_attr_kernel), then the commitments as ONE fixed-base
// sum of k nparties lanes over h[Prv[ii]], written as 49-byte records where the caller wants them; nPrv = 0: the empty product, infinity.
struct mhac_iss_attr_plan { mhac_bbs_sets s; ac_bbs_order list; size_t nb; };
static int mhac_iss_attr_args(size_t m, size_t t, size_t nparties, size_t nPrv, const uint32_t* prv, const void* pp, const void* h, const void* rnd,
                              const void* pub, const void* ashare, const void* C, mhac_iss_attr_plan& p) {
    if (!mhac_iss_shape_ok(t, nparties) || (nPrv && !prv) || !mhac_bbs_derive(p.s, m, prv, nPrv, nullptr, 0)) return C12381_E_ARG;
    p.nb = mhac_iss_attr_list(p.list, p.s);
    return (!pp || !h || !rnd || !C || (p.s.nPub && !pub) || (p.s.nPrv && !ashare)) ? C12381_E_ARG : 0;
}
int c12381_mhac_bbs_attr_batch_dev(c12381_ctx* c, size_t n, size_t m, size_t t, size_t nparties, size_t nPrv, const uint32_t* prv, const uint8_t* pp_146,
                                   const uint8_t* h_49, const uint8_t* rnd, uint8_t* pub_48, uint8_t* ashare_48, uint8_t* C_49) {
    mhac_iss_attr_plan p;
    int rc = bind(c) ?: mhac_iss_attr_args(m, t, nparties, nPrv, prv, pp_146, h_49, rnd, pub_48, ashare_48, C_49, p);
    if (rc || n == 0) return rc;
    const size_t cap = mhac_iss_chunk(nparties), ch = n < cap ? n : cap, np = nparties, nPub = p.s.nPub, nrnd = mhac_iss_attr_rnd_count(m, nPrv, t);
    if ((rc = ensure(c, c12381_ctx::WS_MHAC_BBS, mhac_iss_attr_layout(nullptr, ch, np, nPrv).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_MHAC_BBS];
    const ac_bbs_public pub(d);
    size_t npub;
    if ((rc = mhac_iss_pub(c, p.list, p.nb, pp_146, h_49, pub, npub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t k = n - off < ch ? n - off : ch, L = k * np;
        const mhac_iss_attr_slab s = mhac_iss_attr_layout(d, k, np, nPrv);
        uint8_t *pa = nPub ? pub_48 + 48 * nPub * off : pub_48, *as = nPrv ? ashare_48 + 48 * nPrv * np * off : ashare_48, *C = C_49 + 49 * np * off;
        LAUNCH(c, mhac_iss_attr_kernel, L, k, np, t, p.s, rnd + 32 * nrnd * off, pa, as, s.sc);
        if (off == 0 && (rc = join_side(c))) return rc;
        if (nPrv) {
            if ((rc = g1_fixed_sum_range(c, L, nPrv, 0, nPrv, pub.y96, nullptr, s.sc, C, 49))) return rc;
        } else {
            HIPCK(c, hipMemsetAsync(C, 0, 49 * L, c->stream));
        }
        LAUNCH(c, mhac_iss_attr_finish_kernel, L, L, np, nPrv, nPub, npub, (const uint8_t*)pub.st, pa, as, C, c->d_flag);
    }
    return 0;
}
int c12381_mhac_bbs_attr_batch(c12381_ctx* c, size_t n, size_t m, size_t t, size_t nparties, size_t nPrv, const uint32_t* prv, const uint8_t* pp_146,
                               const uint8_t* h_49, const uint8_t* rnd, uint8_t* pub_48, uint8_t* ashare_48, uint8_t* C_49) {
    mhac_iss_attr_plan p;
    int rc = bind(c) ?: mhac_iss_attr_args(m, t, nparties, nPrv, prv, pp_146, h_49, rnd, pub_48, ashare_48, C_49, p);
    if (rc || n == 0) return rc;
    const size_t nPub = p.s.nPub;
    return host_form(c, {{pp_146, 146}, {h_49, 49 * m}, {rnd, 32 * mhac_iss_attr_rnd_count(m, nPrv, t) * n}},
                     {{pub_48, 48 * nPub * n}, {ashare_48, 48 * nPrv * nparties * n}, {C_49, 49 * nparties * n}}, [&](const staging& s) {
        return c12381_mhac_bbs_attr_batch_dev(c, n, m, t, nparties, nPrv, prv, s.in[0], s.in[1], s.in[2], nPub ? s.out[0] : nullptr, nPrv ? s.out[1] : nullptr,
                                              s.out[2]);
    });
}

// ---------------------------------------------------------------- iss (cred_iss.cpp:43-85)
// Per credential of a chunk: gamma, e, the range checks, e_share and -e_share, the columns lambda and pub_a (mhac_iss_iss_prep_kernel); the nparties
// C records decoded where they lie; C[0] .. C[t-1] as term columns, prod C[i]^lambda_i by per-term multiplies (mhac_iss_powers); g1 * prod h^pub_a
// as one fixed-base sum with addend g1; C_a their sum; inverse(gamma + e) by the simultaneous inversion; A = C_a^inverse as a generic G1 column; A
// replicated over its nparties lanes, A^(-e_share) as ONE generic G1 column of k nparties lanes, D = C + that; then the records and the status
// (mhac_iss_iss_finish_kernel).
struct mhac_iss_iss_plan { ac_bbs_order list; mhac_iss_lambda lam; };
static int mhac_iss_iss_args(size_t m, size_t t, size_t nparties, size_t nPub, const uint32_t* pub_idx, const void* pp, const void* h, const void* sk,
                             const void* C, const void* pub, const void* rnd, const void* A, const void* eshare, const void* D, const void* status,
                             mhac_iss_iss_plan& p) {
    if (m == 0 || m > MHAC_BBS_MAX_ATTR || !mhac_iss_shape_ok(t, nparties) || !mhac_iss_pub_list(p.list, m, pub_idx, nPub)) return C12381_E_ARG;
    uint32_t x[MHAC_BBS_T_MAX];
    for (size_t i = 0; i < t; ++i) x[i] = (uint32_t)i + 1;
    mhac_iss_lagrange(p.lam, x, t);
    return (!pp || !h || !sk || !C || !rnd || !A || !eshare || !D || !status || (nPub && !pub)) ? C12381_E_ARG : 0;
}
int c12381_mhac_bbs_iss_batch_dev(c12381_ctx* c, size_t n, size_t m, size_t t, size_t nparties, size_t nPub, const uint32_t* pub_idx, const uint8_t* pp_146,
                                  const uint8_t* h_49, const uint8_t* sk_48, const uint8_t* C_49, const uint8_t* pub_48, const uint8_t* rnd, uint8_t* A_49,
                                  uint8_t* eshare_48, uint8_t* D_49, uint8_t* status) {
    mhac_iss_iss_plan p;
    int rc = bind(c) ?: mhac_iss_iss_args(m, t, nparties, nPub, pub_idx, pp_146, h_49, sk_48, C_49, pub_48, rnd, A_49, eshare_48, D_49, status, p);
    if (rc || n == 0) return rc;
    const size_t cap = mhac_iss_chunk(nparties), ch = n < cap ? n : cap, np = nparties;
    if ((rc = ensure(c, c12381_ctx::WS_MHAC_BBS, mhac_iss_iss_layout(nullptr, ch, np, t, nPub).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_MHAC_BBS];
    const ac_bbs_public pub(d);
    size_t npub;
    if ((rc = mhac_iss_pub(c, p.list, nPub, pp_146, h_49, pub, npub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t k = n - off < ch ? n - off : ch, L = k * np;
        const mhac_iss_iss_slab s = mhac_iss_iss_layout(d, k, np, t, nPub);
        uint8_t *es = eshare_48 + 48 * np * off, *D = D_49 + 49 * np * off;
        LAUNCH(c, mhac_iss_iss_prep_kernel, L, k, np, t, nPub, p.lam, sk_48, nPub ? pub_48 + 48 * nPub * off : pub_48, rnd + 32 * mhac_iss_iss_rnd_count(t) * off,
               s.gam, s.st, s.e32, s.scl, s.scp, s.nes, es, c->d_flag);
        LAUNCH(c, g1_decompress_kernel, L, L, C_49 + 49 * np * off, s.c96, s.st_c, 0);
        LAUNCH(c, mhac_iss_cols_kernel, t * k, k, np, t, (const uint8_t*)s.c96, s.q96);
        if ((rc = mhac_iss_powers(c, k, t, s.q96, s.scl, s.u96, s.v96))) return rc;
        if (off == 0 && (rc = join_side(c))) return rc;
        if (nPub) {
            if ((rc = g1_fixed_sum_range(c, k, nPub, 0, nPub, pub.y96, pub.g96, s.scp, s.v96, 96))) return rc;
        } else {
            LAUNCH(c, ac_bbs_bcast96_kernel, k, k, (const uint8_t*)pub.g96, s.v96);
        }
        if ((rc = ac_bbs_add(c, k, s.u96, s.v96, s.u96, 96))) return rc;                                                       // C_a
        if ((rc = zp_batch_inverse(c, k, s.e32, s.gam, s.inv))) return rc;
        if ((rc = c12381_g1_mul_batch_dev(c, k, s.u96, s.inv, s.a96, 96))) return rc;                                          // A
        LAUNCH(c, mhac_iss_rep_kernel, L, L, np, (const uint8_t*)s.a96, s.r96);
        if ((rc = c12381_g1_mul_batch_dev(c, L, s.r96, s.nes, s.w96, 96))) return rc;                                          // A^(-e_share[i])
        if ((rc = ac_bbs_add(c, L, s.c96, s.w96, s.w96, 96))) return rc;                                                       // D[i]
        LAUNCH(c, mhac_iss_iss_finish_kernel, L, L, np, npub, (const uint8_t*)pub.st, (const uint8_t*)s.gam, (const uint8_t*)s.st, (const uint8_t*)s.st_c,
               (const uint8_t*)s.a96, (const uint8_t*)s.w96, A_49 + 49 * off, es, D, status + off, c->d_flag);
    }
    return 0;
}
int c12381_mhac_bbs_iss_batch(c12381_ctx* c, size_t n, size_t m, size_t t, size_t nparties, size_t nPub, const uint32_t* pub_idx, const uint8_t* pp_146,
                              const uint8_t* h_49, const uint8_t* sk_48, const uint8_t* C_49, const uint8_t* pub_48, const uint8_t* rnd, uint8_t* A_49,
                              uint8_t* eshare_48, uint8_t* D_49, uint8_t* status) {
    mhac_iss_iss_plan p;
    int rc = bind(c) ?: mhac_iss_iss_args(m, t, nparties, nPub, pub_idx, pp_146, h_49, sk_48, C_49, pub_48, rnd, A_49, eshare_48, D_49, status, p);
    if (rc || n == 0) return rc;
    return host_form(c, {{pp_146, 146}, {h_49, 49 * m}, {sk_48, 48}, {C_49, 49 * nparties * n}, {nPub ? pub_48 : nullptr, 48 * nPub * n},
                         {rnd, 32 * mhac_iss_iss_rnd_count(t) * n}},
                     {{A_49, 49 * n}, {eshare_48, 48 * nparties * n}, {D_49, 49 * nparties * n}, {status, n}}, [&](const staging& s) {
        return c12381_mhac_bbs_iss_batch_dev(c, n, m, t, nparties, nPub, pub_idx, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.out[0], s.out[1],
                                             s.out[2], s.out[3]);
    });
}

// ---------------------------------------------------------------- group (make_pres_group.cpp:6-21)
// Per presentation: the t D records of S as columns, lambda as records and scalar columns, the gather of the rows of S (mhac_iss_group_prep_kernel),
// decode, D = prod D_share[S[k]]^lambda[k] by per-term multiplies, the record and the status (mhac_iss_group_finish_kernel).  No key: nothing runs
// on the side stream.
struct mhac_iss_group_plan { mhac_iss_parties_set S; mhac_iss_lambda lam; };
static int mhac_iss_group_args(size_t nparties, size_t t, const uint32_t* S, size_t nPrv, const void* D, const void* eshare, const void* ashare, const void* lam,
                               const void* Dg, const void* eS, const void* aS, const void* status, mhac_iss_group_plan& p) {
    uint32_t x[MHAC_BBS_T_MAX];
    if (nPrv > MHAC_BBS_MAX_ATTR || !mhac_iss_parties(p.S, x, S, t, nparties)) return C12381_E_ARG;
    mhac_iss_lagrange(p.lam, x, t);
    return (!D || !lam || !Dg || !status || !eshare != !eS || (nPrv && !ashare != !aS)) ? C12381_E_ARG : 0;
}
int c12381_mhac_bbs_group_batch_dev(c12381_ctx* c, size_t n, size_t nparties, size_t t, const uint32_t* S, size_t nPrv, const uint8_t* D_49,
                                    const uint8_t* eshare_48, const uint8_t* ashare_48, uint8_t* lam_48, uint8_t* Dg_49, uint8_t* eS_48, uint8_t* aS_48,
                                    uint8_t* status) {
    mhac_iss_group_plan p;
    int rc = bind(c) ?: mhac_iss_group_args(nparties, t, S, nPrv, D_49, eshare_48, ashare_48, lam_48, Dg_49, eS_48, aS_48, status, p);
    if (rc || n == 0) return rc;
    const size_t ch = n < MHAC_ISS_CHUNK ? n : MHAC_ISS_CHUNK, np = nparties;
    const bool rows_e = eS_48 != nullptr, rows_a = nPrv && aS_48;
    if ((rc = ensure(c, c12381_ctx::WS_MHAC_BBS, mhac_iss_group_layout(nullptr, ch, t).bytes))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t k = n - off < ch ? n - off : ch;
        const mhac_iss_group_slab s = mhac_iss_group_layout(c->ws[c12381_ctx::WS_MHAC_BBS], k, t);
        uint8_t *lam = lam_48 + 48 * t * off, *eS = rows_e ? eS_48 + 48 * t * off : nullptr, *aS = rows_a ? aS_48 + 48 * nPrv * t * off : nullptr;
        LAUNCH(c, mhac_iss_group_prep_kernel, k, k, np, t, nPrv, p.S, p.lam, D_49 + 49 * np * off, rows_e ? eshare_48 + 48 * np * off : nullptr,
               rows_a ? ashare_48 + 48 * nPrv * np * off : nullptr, s.p49, s.sc, lam, eS, aS);
        LAUNCH(c, g1_decompress_kernel, t * k, t * k, s.p49, s.p96, s.st_p, 0);
        if ((rc = mhac_iss_powers(c, k, t, s.p96, s.sc, s.u96, s.v96))) return rc;
        LAUNCH(c, mhac_iss_group_finish_kernel, k, k, t, nPrv, (const uint8_t*)s.st_p, (const uint8_t*)s.u96, Dg_49 + 49 * off, lam, eS, aS, status + off);
    }
    return 0;
}
int c12381_mhac_bbs_group_batch(c12381_ctx* c, size_t n, size_t nparties, size_t t, const uint32_t* S, size_t nPrv, const uint8_t* D_49, const uint8_t* eshare_48,
                                const uint8_t* ashare_48, uint8_t* lam_48, uint8_t* Dg_49, uint8_t* eS_48, uint8_t* aS_48, uint8_t* status) {
    mhac_iss_group_plan p;
    int rc = bind(c) ?: mhac_iss_group_args(nparties, t, S, nPrv, D_49, eshare_48, ashare_48, lam_48, Dg_49, eS_48, aS_48, status, p);
    if (rc || n == 0) return rc;
    const bool rows_e = eS_48 != nullptr, rows_a = nPrv && aS_48;
    return host_form(c, {{D_49, 49 * nparties * n}, {rows_e ? eshare_48 : nullptr, 48 * nparties * n}, {rows_a ? ashare_48 : nullptr, 48 * nPrv * nparties * n}},
                     {{lam_48, 48 * t * n}, {Dg_49, 49 * n}, {eS_48, rows_e ? 48 * t * n : 0}, {aS_48, rows_a ? 48 * nPrv * t * n : 0}, {status, n}},
                     [&](const staging& s) {
        return c12381_mhac_bbs_group_batch_dev(c, n, nparties, t, S, nPrv, s.in[0], s.in[1], s.in[2], s.out[0], s.out[1], rows_e ? s.out[2] : nullptr,
                                               rows_a ? s.out[3] : nullptr, s.out[4]);
    });
}

// ---------------------------------------------------------------- type (make_pres_type.cpp:6-38)
// The Pub records of h form ONE base list, the revealed positions in front (mhac_iss_type_list).  Per presentation: the range check and the columns
// (mhac_iss_type_prep_kernel), C_rev = g1 + the sum over [0, nRevPub), the sum over [nRevPub, nPub), C_pub = C_rev + that (ac_bbs_add: C_rev is a
// per-lane addend); an empty range leaves its addend.  Then the records and the status (mhac_iss_type_finish_kernel).
struct mhac_iss_type_args_plan { mhac_bbs_sets s; mhac_iss_type_plan tp; size_t nb; };
static int mhac_iss_type_args(size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const void* pp, const void* h, const void* pub,
                              const void* crev, const void* cpub, const void* status, mhac_iss_type_args_plan& p) {
    if ((nPrv && !prv) || (nRev && !rev) || !mhac_bbs_derive(p.s, m, prv, nPrv, rev, nRev)) return C12381_E_ARG;
    p.nb = mhac_iss_type_list(p.tp, p.s);
    return (!pp || !h || !crev || !cpub || !status || (p.s.nPub && !pub)) ? C12381_E_ARG : 0;
}
int c12381_mhac_bbs_type_batch_dev(c12381_ctx* c, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const uint8_t* pp_146,
                                   const uint8_t* h_49, const uint8_t* pub_48, uint8_t* crev_49, uint8_t* cpub_49, uint8_t* status) {
    mhac_iss_type_args_plan p;
    int rc = bind(c) ?: mhac_iss_type_args(m, nPrv, prv, nRev, rev, pp_146, h_49, pub_48, crev_49, cpub_49, status, p);
    if (rc || n == 0) return rc;
    const size_t ch = n < MHAC_ISS_CHUNK ? n : MHAC_ISS_CHUNK, nPub = p.s.nPub, nrp = p.s.nRevPub, nhp = p.s.nHidPub;
    if ((rc = ensure(c, c12381_ctx::WS_MHAC_BBS, mhac_iss_type_layout(nullptr, ch, nPub).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_MHAC_BBS];
    const ac_bbs_public pub(d);
    size_t npub;
    if ((rc = mhac_iss_pub(c, p.tp.list, p.nb, pp_146, h_49, pub, npub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t k = n - off < ch ? n - off : ch;
        const mhac_iss_type_slab s = mhac_iss_type_layout(d, k, nPub);
        LAUNCH(c, mhac_iss_type_prep_kernel, k, k, nPub, p.tp, nPub ? pub_48 + 48 * nPub * off : pub_48, s.sca, s.st);
        if (off == 0 && (rc = join_side(c))) return rc;
        if (nrp) {
            if ((rc = g1_fixed_sum_range(c, k, nPub, 0, nrp, pub.y96, pub.g96, s.sca, s.r96, 96))) return rc;                  // C_rev
        } else {
            LAUNCH(c, ac_bbs_bcast96_kernel, k, k, (const uint8_t*)pub.g96, s.r96);
        }
        if (nhp) {
            if ((rc = g1_fixed_sum_range(c, k, nPub, nrp, nhp, pub.y96, nullptr, s.sca + 32 * nrp * k, s.v96, 96))) return rc;
            if ((rc = ac_bbs_add(c, k, s.r96, s.v96, s.p96, 96))) return rc;                                                   // C_pub
        } else {
            HIPCK(c, hipMemcpyAsync(s.p96, s.r96, 96 * k, hipMemcpyDeviceToDevice, c->stream));
        }
        LAUNCH(c, mhac_iss_type_finish_kernel, k, k, npub, (const uint8_t*)pub.st, (const uint8_t*)s.st, (const uint8_t*)s.r96, (const uint8_t*)s.p96,
               crev_49 + 49 * off, cpub_49 + 49 * off, status + off, c->d_flag);
    }
    return 0;
}
int c12381_mhac_bbs_type_batch(c12381_ctx* c, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const uint8_t* pp_146,
                               const uint8_t* h_49, const uint8_t* pub_48, uint8_t* crev_49, uint8_t* cpub_49, uint8_t* status) {
    mhac_iss_type_args_plan p;
    int rc = bind(c) ?: mhac_iss_type_args(m, nPrv, prv, nRev, rev, pp_146, h_49, pub_48, crev_49, cpub_49, status, p);
    if (rc || n == 0) return rc;
    const size_t nPub = p.s.nPub;
    return host_form(c, {{pp_146, 146}, {h_49, 49 * m}, {nPub ? pub_48 : nullptr, 48 * nPub * n}}, {{crev_49, 49 * n}, {cpub_49, 49 * n}, {status, n}},
                     [&](const staging& s) { return c12381_mhac_bbs_type_batch_dev(c, n, m, nPrv, prv, nRev, rev, s.in[0], s.in[1], s.in[2], s.out[0], s.out[1], s.out[2]); });
}
