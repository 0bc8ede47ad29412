// The AC-rbbs credential entries of the C ABI (include/c12381_ac.h): redaction caches, presentations and their verification, from the wire formats
// of the reference's examples/AC-rbbs.  Kernels: k_ac_rbbs.hip (and two of k_ac_bbs.hip); the per-lane scalar work, the q_i hashes and redact's base
// list: ac_rbbs.hpp; the shared host pieces: host.hpp.
#include "host.hpp"

#include "../../include/c12381_ac.h"
#include "ac_rbbs.hpp"

using namespace c12381;
using namespace c12381_host;

static_assert(2 * AC_RBBS_REDACT_MAX_ATTR == C12381_G1_FIXED_SUM_MAX, "redact's base list: up to 2 nattr - 1 fixed-base tables");
static_assert(AC_BBS_MAX_ATTR <= C12381_G2_FIXED_SUM_MAX, "the G2 sum of verify takes up to nattr bases");
constexpr size_t AC_RBBS_CHUNK = (size_t)1 << 18;

// ---------------------------------------------------------------- verify (verify.cpp:6-24)
// The used key records — Y_i and tilde_Y[nattr-1-i] for i in I, in the order of idx — are gathered and decoded on the side stream with g, tilde_g and
// tilde_X; the reference's parse of pk.Y / pk.tilde_Y is lazy, so no other record is read.  Per presentation: split, range-check and the q_i
// (ac_rbbs_verify_prep_kernel), decode the five points, re-encode them and set up the terms A_, -B_ (ac_bbs_encode_kernel, ac_rbbs_encode_kernel),
// c (ac_rbbs_challenge_kernel), K = g + sum_I a_i Y_i by the fixed-base sum, R = K^s A_^t (-B_)^c as ONE k = 3 product, C_J_ + B_, the first pairing
// equation as c12381_ps_verify_batch_dev with no messages (s1 = A_, s2 = C_J_ + B_), the second as the same body without X2 (ps_verify_core: s1 =
// C_J_, s2 = D_, Y2 = the used tilde_Y, messages q_i), and the verdict (ac_rbbs_verify_finish_kernel).
struct ac_rbbs_set { ac_bbs_order idx, tidx; };       // the records of pk.Y and of pk.tilde_Y that verify uses
static int ac_rbbs_verify_args(size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const void* pk, const void* Y, const void* tY, const void* pres,
                               const void* attr, const void* msgs, const void* ok, ac_rbbs_set& s) {
    if ((nI && !idx) || !ac_bbs_base_order(s.idx, nattr, idx, nI)) return C12381_E_ARG;
    s.tidx = {};
    for (size_t k = 0; k < nI; ++k) s.tidx.at[k] = (uint8_t)(nattr - 1 - idx[k]);
    return (!pk || !Y || !tY || !pres || !ok || (nI && !attr) || (msg_len && !msgs)) ? C12381_E_ARG : 0;
}
int c12381_ac_rbbs_verify_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                    const uint8_t* Y_49, const uint8_t* tY_97, const uint8_t* pres_341, const uint8_t* attr_48, const uint8_t* msgs,
                                    uint8_t* ok) {
    ac_rbbs_set set;
    int rc = bind(c) ?: ac_rbbs_verify_args(nattr, nI, idx, msg_len, pk_243, Y_49, tY_97, pres_341, attr_48, msgs, ok, set);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_RBBS_CHUNK ? n : AC_RBBS_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_AC_RBBS, ac_rbbs_verify_layout(nullptr, ch, nI, msg_len).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_RBBS];
    const ac_rbbs_public pub(d);
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_243, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pk_243 + 49, pub.g2, pub.st + 1, 0);
    if (nI) {
        LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(49 * nI)), dim3(BLOCK), c->side, nI, (size_t)49, set.idx, Y_49, pub.y49);
        LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(97 * nI)), dim3(BLOCK), c->side, nI, (size_t)97, set.tidx, tY_97, pub.ty97);
        LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nI, (const uint8_t*)pub.y49, pub.y96, pub.st + 3, 0);
        LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nI, (const uint8_t*)pub.ty97, pub.ty192, pub.st + 3 + nI, 0);
    }
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_rbbs_verify_slab s = ac_rbbs_verify_layout(d, m, nI, msg_len);
        LAUNCH(c, ac_rbbs_verify_prep_kernel, m, m, nI, set.idx, pres_341 + 341 * off, nI ? attr_48 + 48 * nI * off : attr_48, s.p49, s.sc3, s.sca, s.q32, s.st);
        LAUNCH(c, g1_decompress_kernel, 5 * m, 5 * m, s.p49, s.p96, s.st_p, 0);
        const uint8_t *A96 = s.p96, *B96 = s.p96 + 96 * m, *U96 = s.p96 + 192 * m, *CJ96 = s.p96 + 288 * m, *D96 = s.p96 + 384 * m;
        LAUNCH(c, ac_bbs_encode_kernel, m, m, A96, B96, U96, s.e49, s.q96);
        LAUNCH(c, ac_rbbs_encode_kernel, m, m, (size_t)2, CJ96, s.e49 + 147 * m);
        LAUNCH(c, ac_rbbs_challenge_kernel, m, m, msg_len, msg_len ? msgs + msg_len * off : msgs, (const uint8_t*)s.e49, 2, s.tr, s.sc3 + 64 * m);
        if (off == 0 && (rc = join_side(c))) return rc;
        if (nI) {
            if ((rc = g1_fixed_sum_range(c, m, nI, 0, nI, pub.y96, pub.g96, s.sca, s.q96, 96))) return rc;                    // K
        } else {
            LAUNCH(c, ac_bbs_bcast96_kernel, m, m, (const uint8_t*)pub.g96, s.q96);
        }
        if ((rc = c12381_g1_mul_sum_batch_dev(c, m, 3, s.q96, s.sc3, s.r49, 49, 0u))) return rc;                               // R
        if ((rc = ac_bbs_add(c, m, CJ96, B96, s.s96, 96))) return rc;
        if ((rc = c12381_ps_verify_batch_dev(c, m, 0, pub.g2, pub.g2 + 192, nullptr, A96, s.s96, nullptr, s.ok1))) return rc;
        if ((rc = ps_verify_core(c, m, nI, pub.g2, nullptr, pub.ty192, CJ96, D96, s.q32, s.ok3))) return rc;
        LAUNCH(c, ac_rbbs_verify_finish_kernel, m, m, 3 + 2 * nI, (const uint8_t*)pub.st, (const uint8_t*)s.st, (const uint8_t*)s.st_p, (const uint8_t*)s.r49,
               (const uint8_t*)(s.e49 + 98 * m), (const uint8_t*)s.ok1, (const uint8_t*)s.ok3, ok + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rbbs_verify_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243, const uint8_t* Y_49,
                                const uint8_t* tY_97, const uint8_t* pres_341, const uint8_t* attr_48, const uint8_t* msgs, uint8_t* ok) {
    ac_rbbs_set set;
    int rc = bind(c) ?: ac_rbbs_verify_args(nattr, nI, idx, msg_len, pk_243, Y_49, tY_97, pres_341, attr_48, msgs, ok, set);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {Y_49, 49 * 2 * nattr}, {tY_97, 97 * nattr}, {pres_341, 341 * n}, {nI ? attr_48 : nullptr, 48 * nI * n},
                         {msg_len ? msgs : nullptr, msg_len * n}}, {{ok, n}}, [&](const staging& s) {
        return c12381_ac_rbbs_verify_batch_dev(c, n, nattr, nI, idx, msg_len, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.out[0]);
    });
}

// ---------------------------------------------------------------- pres (pres.cpp:6-27)
// Per presentation: the records C_I | A, B, C_J, D and r four times, alpha, beta (ac_rbbs_pres_prep_kernel), decode the five, A_, B_, C_J_, D_ as ONE
// generic column of 4 m lanes, U = C_I^alpha A_^beta as one k = 2 product, the encodings, c, the responses and the record
// (ac_rbbs_pres_finish_kernel).  No key and no index set: nothing runs on the side stream.
static int ac_rbbs_pres_args(size_t msg_len, const void* sig, const void* cache, const void* msgs, const void* rnd, const void* pres, const void* status) {
    return (!sig || !cache || !rnd || !pres || !status || (msg_len && !msgs)) ? C12381_E_ARG : 0;
}
int c12381_ac_rbbs_pres_batch_dev(c12381_ctx* c, size_t n, size_t msg_len, const uint8_t* sig_97, const uint8_t* cache_196, const uint8_t* msgs,
                                  const uint8_t* rnd, uint8_t* pres_341, uint8_t* status) {
    int rc = bind(c) ?: ac_rbbs_pres_args(msg_len, sig_97, cache_196, msgs, rnd, pres_341, status);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_RBBS_CHUNK ? n : AC_RBBS_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_AC_RBBS, ac_rbbs_pres_layout(nullptr, ch, msg_len).bytes))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_rbbs_pres_slab s = ac_rbbs_pres_layout(c->ws[c12381_ctx::WS_AC_RBBS], m, msg_len);
        const uint8_t *sig = sig_97 + 97 * off, *rn = rnd + 32 * AC_RBBS_PRES_RANDOM * off;
        LAUNCH(c, ac_rbbs_pres_prep_kernel, m, m, sig, cache_196 + 196 * off, rn, s.p49, s.scr, s.sc2, s.st);
        LAUNCH(c, g1_decompress_kernel, 5 * m, 5 * m, s.p49, s.p96, s.st_p, 0);
        if ((rc = c12381_g1_mul_batch_dev(c, 4 * m, s.p96 + 96 * m, s.scr, s.o96, 96))) return rc;                           // A_ | B_ | C_J_ | D_
        HIPCK(c, hipMemcpyAsync(s.t96, s.p96, 96 * m, hipMemcpyDeviceToDevice, c->stream));                                   // C_I
        HIPCK(c, hipMemcpyAsync(s.t96 + 96 * m, s.o96, 96 * m, hipMemcpyDeviceToDevice, c->stream));                          // A_
        if ((rc = c12381_g1_mul_sum_batch_dev(c, m, 2, s.t96, s.sc2, s.o96 + 384 * m, 96, 0u))) return rc;                     // U
        LAUNCH(c, ac_rbbs_encode_kernel, m, m, (size_t)5, (const uint8_t*)s.o96, s.e49);
        LAUNCH(c, ac_rbbs_challenge_kernel, m, m, msg_len, msg_len ? msgs + msg_len * off : msgs, (const uint8_t*)s.e49, 4, s.tr, s.c32);
        LAUNCH(c, ac_rbbs_pres_finish_kernel, m, m, sig, rn, (const uint8_t*)s.e49, (const uint8_t*)s.c32, (const uint8_t*)s.st, (const uint8_t*)s.st_p,
               pres_341 + 341 * off, status + off);
    }
    return 0;
}
int c12381_ac_rbbs_pres_batch(c12381_ctx* c, size_t n, size_t msg_len, const uint8_t* sig_97, const uint8_t* cache_196, const uint8_t* msgs, const uint8_t* rnd,
                              uint8_t* pres_341, uint8_t* status) {
    int rc = bind(c) ?: ac_rbbs_pres_args(msg_len, sig_97, cache_196, msgs, rnd, pres_341, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{sig_97, 97 * n}, {cache_196, 196 * n}, {msg_len ? msgs : nullptr, msg_len * n}, {rnd, 32 * AC_RBBS_PRES_RANDOM * n}},
                     {{pres_341, 341 * n}, {status, n}}, [&](const staging& s) {
        return c12381_ac_rbbs_pres_batch_dev(c, n, msg_len, s.in[0], s.in[1], s.in[2], s.in[3], s.out[0], s.out[1]);
    });
}

// ---------------------------------------------------------------- redact (redact.cpp:7-44)
// The reference materialises pk.Y: all 2 nattr records are decoded on the side stream, with g, tilde_g and tilde_X, and the base list of the plan
// (ac_rbbs.hpp) is gathered from them.  Per credential: A's record, the attribute columns, -w, the q_i and the exponents of D
// (ac_rbbs_redact_prep_kernel), decode A, then C_I = g + sum over [0, nI), C_J = sum over [cj_first, total) and D = sum over [d_first, d_first + nD)
// of that ONE list through g1_fixed_sum_range — a later call with the same key and set builds no table — A^(-w) by the generic column, B = C_I +
// A^(-w), and the record (ac_rbbs_redact_finish_kernel).  An empty range is the empty product: infinity (C_I: g).
static int ac_rbbs_redact_args(size_t nattr, size_t nI, const uint32_t* idx, const void* pk, const void* Y, const void* attr, const void* sig, const void* cache,
                               const void* status, ac_rbbs_plan& p) {
    if ((nI && !idx) || !ac_rbbs_redact_plan(p, nattr, idx, nI)) return C12381_E_ARG;
    return (!pk || !Y || !attr || !sig || !cache || !status) ? C12381_E_ARG : 0;
}
int c12381_ac_rbbs_redact_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                    const uint8_t* attr_48, const uint8_t* sig_97, uint8_t* cache_196, uint8_t* status) {
    ac_rbbs_plan pl;
    int rc = bind(c) ?: ac_rbbs_redact_args(nattr, nI, idx, pk_243, Y_49, attr_48, sig_97, cache_196, status, pl);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_RBBS_CHUNK ? n : AC_RBBS_CHUNK, nJ = pl.nJ, nD = pl.nD, total = pl.total;
    if ((rc = ensure(c, c12381_ctx::WS_AC_RBBS, ac_rbbs_redact_layout(nullptr, ch, nattr, nI, nD).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_RBBS];
    const ac_rbbs_public pub(d);
    ac_bbs_order list = {};
    for (size_t k = 0; k < total; ++k) list.at[k] = pl.y[k];
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_243, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pk_243 + 49, pub.g2, pub.st + 1, 0);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, 2 * nattr, Y_49, pub.y96, pub.st + 3, 0);
    LAUNCH_ON(c, ac_rbbs_gather_kernel, dim3(grid_for(96 * total)), dim3(BLOCK), c->side, total, (size_t)96, list, (const uint8_t*)pub.y96, pub.l96);
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_rbbs_redact_slab s = ac_rbbs_redact_layout(d, m, nattr, nI, nD);
        uint8_t *CI = s.o96, *CJ = s.o96 + 96 * m, *B = s.o96 + 192 * m, *D = s.o96 + 288 * m;
        LAUNCH(c, ac_rbbs_redact_prep_kernel, m, m, pl, attr_48 + 48 * nattr * off, sig_97 + 97 * off, s.a49, s.sca, s.scw, s.aI48, s.q32, s.scd, s.st);
        LAUNCH(c, g1_decompress_kernel, m, m, s.a49, s.a96, s.st_a, 0);
        if ((rc = c12381_g1_mul_batch_dev(c, m, s.a96, s.scw, s.t96, 96))) return rc;                                        // A^(-w)
        if (off == 0 && (rc = join_side(c))) return rc;
        if (nI) {
            if ((rc = g1_fixed_sum_range(c, m, total, 0, nI, pub.l96, pub.g96, s.sca, CI, 96))) return rc;
        } else {
            LAUNCH(c, ac_bbs_bcast96_kernel, m, m, (const uint8_t*)pub.g96, CI);
        }
        if (nJ) {
            if ((rc = g1_fixed_sum_range(c, m, total, pl.cj_first, nJ, pub.l96, nullptr, s.sca + 32 * nI * m, CJ, 96))) return rc;
        } else {
            HIPCK(c, hipMemsetAsync(CJ, 0, 96 * m, c->stream));
        }
        if (nD) {
            if ((rc = g1_fixed_sum_range(c, m, total, pl.d_first, nD, pub.l96, nullptr, s.scd, D, 96))) return rc;
        } else {
            HIPCK(c, hipMemsetAsync(D, 0, 96 * m, c->stream));
        }
        if ((rc = ac_bbs_add(c, m, CI, s.t96, B, 96))) return rc;
        LAUNCH(c, ac_rbbs_redact_finish_kernel, m, m, 3 + 2 * nattr, (const uint8_t*)pub.st, (const uint8_t*)s.st, (const uint8_t*)s.st_a, (const uint8_t*)s.o96,
               cache_196 + 196 * off, status + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rbbs_redact_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                const uint8_t* attr_48, const uint8_t* sig_97, uint8_t* cache_196, uint8_t* status) {
    ac_rbbs_plan pl;
    int rc = bind(c) ?: ac_rbbs_redact_args(nattr, nI, idx, pk_243, Y_49, attr_48, sig_97, cache_196, status, pl);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {Y_49, 49 * 2 * nattr}, {attr_48, 48 * nattr * n}, {sig_97, 97 * n}}, {{cache_196, 196 * n}, {status, n}},
                     [&](const staging& s) { return c12381_ac_rbbs_redact_batch_dev(c, n, nattr, nI, idx, s.in[0], s.in[1], s.in[2], s.in[3], s.out[0], s.out[1]); });
}
