// The AC-bbs credential entries of the C ABI (include/c12381_ac.h): verification of presentations and their creation, from the wire formats of the
// reference's examples/AC-bbs.  Kernels: k_ac_bbs.hip; the per-lane scalar work and the base order: ac_bbs.hpp; the shared host pieces: host.hpp.
#include "host.hpp"

#include "../../include/c12381_ac.h"
#include "ac_bbs.hpp"

using namespace c12381;
using namespace c12381_host;

static_assert(AC_BBS_MAX_ATTR == C12381_G1_FIXED_SUM_MAX, "one fixed-base table per attribute");
constexpr size_t AC_BBS_CHUNK = (size_t)1 << 18;

// The disclosure set as the entries use it: the base order (ac_bbs.hpp) and both counts.  Every Y-sum of both entries runs over a range of ONE
// base list, Y in base order — K / C_I over [0, nI), the u_j / a_J / delta_j sums over [nI, nattr) — through g1_fixed_sum_range, which keeps the
// tables of all nattr positions current: a call with the key and the set I of the call before builds no table, whichever entry it is.
struct ac_bbs_set { ac_bbs_order ord; size_t nattr, nI, nJ; };
static int ac_bbs_set_args(size_t nattr, size_t nI, const uint32_t* idx, ac_bbs_set& s) {
    if ((nI && !idx) || !ac_bbs_base_order(s.ord, nattr, idx, nI)) return C12381_E_ARG;
    s.nattr = nattr; s.nI = nI; s.nJ = nattr - nI;
    return 0;
}
// pk on the side stream: g, tilde_g and tilde_X are decoded where they lie in pk.fixed_part, pk.Y after the gather into base order; the caller
// joins the side stream before its first use of them
static int ac_bbs_pub(c12381_ctx* c, const ac_bbs_set& s, const uint8_t* pk_243, const uint8_t* Y_49, const ac_bbs_public& pub) {
    int rc;
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, ac_bbs_key_kernel, dim3(grid_for(49 * s.nattr)), dim3(BLOCK), c->side, s.nattr, s.ord, Y_49, pub.y49);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_243, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pk_243 + 49, pub.g2, pub.st + 1, 0);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, s.nattr, (const uint8_t*)pub.y49, pub.y96, pub.st + 3, 0);
    return 0;
}
// out96[j] = addend + sum over the bases [first, first + nb) of the key; nb = 0: the addend for every lane (only asked for with one)
static int ac_bbs_y_sum(c12381_ctx* c, size_t m, const ac_bbs_set& s, const ac_bbs_public& pub, size_t first, size_t nb, const uint8_t* addend,
                        const uint8_t* sc, uint8_t* out96) {
    if (nb == 0) { LAUNCH(c, ac_bbs_bcast96_kernel, m, m, addend, out96); return 0; }
    return g1_fixed_sum_range(c, m, s.nattr, first, nb, pub.y96, addend, sc, out96, 96);
}
// out[j] = a96[j] + b96[j] (host.hpp: api_ac_rbbs.hip adds with it too)
int c12381_host::ac_bbs_add(c12381_ctx* c, size_t m, const uint8_t* a96, const uint8_t* b96, uint8_t* out, int fmt) {
    proj_slab w;
    int rc;
    if ((rc = proj_ws(c, m, w))) return rc;
    LAUNCH(c, g1_add_kernel, m, m, a96, b96, w.p, w.stride, c->d_flag);
    return g1_finish(c, m, w.p, w.stride, out, fmt);
}

// ---------------------------------------------------------------- verify (verify.cpp:6-26)
// Per presentation: split and range-check (ac_bbs_verify_prep_kernel), decode A_, B_, U, re-encode them for the transcript and set up the terms
// A_, -B_ (ac_bbs_encode_kernel), K = g + sum_I a_i Y_i by the fixed-base sum, c (ac_bbs_challenge_kernel), R = K^s A_^t (-B_)^c as ONE k = 3
// product under one doubling chain (multiply(-B, c) = -multiply(B, c): every term of the GLV form is linear in the point), the fixed-base sum
// over Y_J, one addition and compression, the pairing half as c12381_ps_verify_batch_dev with no messages (g2 = tilde_g, X2 = tilde_X, s1 = A_,
// s2 = B_; its generic route serves key points outside G2), and the verdict (ac_bbs_verify_finish_kernel).  Batches run in chunks of AC_BBS_CHUNK.
static int ac_bbs_verify_args(size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const void* pk, const void* Y, const void* pres, const void* u,
                              const void* attr, const void* msgs, const void* ok, ac_bbs_set& s) {
    int rc = ac_bbs_set_args(nattr, nI, idx, s);
    if (rc) return rc;
    return (!pk || !Y || !pres || !ok || (s.nJ && !u) || (nI && !attr) || (msg_len && !msgs)) ? C12381_E_ARG : 0;
}
int c12381_ac_bbs_verify_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                   const uint8_t* Y_49, const uint8_t* pres_243, const uint8_t* u_48, const uint8_t* attr_48, const uint8_t* msgs, uint8_t* ok) {
    ac_bbs_set set;
    int rc = bind(c) ?: ac_bbs_verify_args(nattr, nI, idx, msg_len, pk_243, Y_49, pres_243, u_48, attr_48, msgs, ok, set);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_BBS_CHUNK ? n : AC_BBS_CHUNK, nJ = set.nJ;
    if ((rc = ensure(c, c12381_ctx::WS_AC_BBS, ac_bbs_verify_layout(nullptr, ch, nattr, msg_len).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_BBS];
    const ac_bbs_public pub(d);
    if ((rc = ac_bbs_pub(c, set, pk_243, Y_49, pub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_bbs_verify_slab s = ac_bbs_verify_layout(d, m, nattr, msg_len);
        LAUNCH(c, ac_bbs_verify_prep_kernel, m, m, nI, nJ, pres_243 + 243 * off, nJ ? u_48 + 48 * nJ * off : u_48, nI ? attr_48 + 48 * nI * off : attr_48,
               s.p49, s.sc3, s.sca, s.st);
        LAUNCH(c, g1_decompress_kernel, 3 * m, 3 * m, s.p49, s.p96, s.st_p, 0);
        const uint8_t *A96 = s.p96, *B96 = s.p96 + 96 * m, *U96 = s.p96 + 192 * m;
        LAUNCH(c, ac_bbs_encode_kernel, m, m, A96, B96, U96, s.e49, s.q96);
        LAUNCH(c, ac_bbs_challenge_kernel, m, m, msg_len, msg_len ? msgs + msg_len * off : msgs, s.e49, s.tr, s.sc3 + 64 * m);
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = ac_bbs_y_sum(c, m, set, pub, 0, nI, pub.g96, s.sca, s.q96))) return rc;                                      // K
        if ((rc = c12381_g1_mul_sum_batch_dev(c, m, 3, s.q96, s.sc3, nJ ? s.r96 : s.r49, nJ ? 96 : 49, 0u))) return rc;       // R
        if (nJ) {
            if ((rc = ac_bbs_y_sum(c, m, set, pub, nI, nJ, nullptr, s.sca + 32 * nI * m, s.s96))) return rc;
            if ((rc = ac_bbs_add(c, m, s.r96, s.s96, s.r49, 49))) return rc;
        }
        if ((rc = c12381_ps_verify_batch_dev(c, m, 0, pub.g2, pub.g2 + 192, nullptr, A96, B96, nullptr, s.okp))) return rc;
        LAUNCH(c, ac_bbs_verify_finish_kernel, m, m, 3 + nattr, pub.st, s.st, s.st_p, s.r49, s.e49 + 98 * m, s.okp, ok + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_bbs_verify_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                               const uint8_t* Y_49, const uint8_t* pres_243, const uint8_t* u_48, const uint8_t* attr_48, const uint8_t* msgs, uint8_t* ok) {
    ac_bbs_set set;
    int rc = bind(c) ?: ac_bbs_verify_args(nattr, nI, idx, msg_len, pk_243, Y_49, pres_243, u_48, attr_48, msgs, ok, set);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {Y_49, 49 * nattr}, {pres_243, 243 * n}, {set.nJ ? u_48 : nullptr, 48 * set.nJ * n}, {nI ? attr_48 : nullptr, 48 * nI * n},
                         {msg_len ? msgs : nullptr, msg_len * n}}, {{ok, n}}, [&](const staging& s) {
        return c12381_ac_bbs_verify_batch_dev(c, n, nattr, nI, idx, msg_len, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.out[0]);
    });
}

// ---------------------------------------------------------------- pres (pres.cpp:6-42)
// Per presentation: A's record, the attribute columns in base order, delta_j and r, alpha, -w, beta (ac_bbs_pres_prep_kernel), decode A,
// C_I = g + sum_I a_i Y_i and C_J = sum_J a_j Y_j by the fixed-base sums, C = C_I + C_J, A_ = A^r, then B_ = C^r A_^(-w) and U' = C_I^alpha A_^beta as
// ONE k = 2 product of 2 m lanes, U = U' + sum_j delta_j Y_J[j], the encodings (ac_bbs_encode_kernel), c (ac_bbs_challenge_kernel), the responses
// and the records (ac_bbs_pres_finish_kernel).
static int ac_bbs_pres_args(size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const void* pk, const void* Y, const void* attr, const void* sig,
                            const void* msgs, const void* rnd, const void* pres, const void* u, const void* status, ac_bbs_set& s) {
    int rc = ac_bbs_set_args(nattr, nI, idx, s);
    if (rc) return rc;
    return (!pk || !Y || !attr || !sig || !rnd || !pres || !status || (s.nJ && !u) || (msg_len && !msgs)) ? C12381_E_ARG : 0;
}
int c12381_ac_bbs_pres_batch_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                 const uint8_t* Y_49, const uint8_t* attr_48, const uint8_t* sig_97, const uint8_t* msgs, const uint8_t* rnd,
                                 uint8_t* pres_243, uint8_t* u_48, uint8_t* status) {
    ac_bbs_set set;
    int rc = bind(c) ?: ac_bbs_pres_args(nattr, nI, idx, msg_len, pk_243, Y_49, attr_48, sig_97, msgs, rnd, pres_243, u_48, status, set);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_BBS_CHUNK ? n : AC_BBS_CHUNK, nJ = set.nJ, nrnd = AC_BBS_PRES_RANDOM + nJ;
    if ((rc = ensure(c, c12381_ctx::WS_AC_BBS, ac_bbs_pres_layout(nullptr, ch, nattr, nJ, msg_len).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_BBS];
    const ac_bbs_public pub(d);
    if ((rc = ac_bbs_pub(c, set, pk_243, Y_49, pub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_bbs_pres_slab s = ac_bbs_pres_layout(d, m, nattr, nJ, msg_len);
        const uint8_t *attr = attr_48 + 48 * nattr * off, *sig = sig_97 + 97 * off, *rn = rnd + 32 * nrnd * off;
        LAUNCH(c, ac_bbs_pres_prep_kernel, m, m, nattr, nJ, set.ord, attr, sig, rn, s.a49, s.sca, s.scd, s.sc2, s.st);
        LAUNCH(c, g1_decompress_kernel, m, m, s.a49, s.a96, s.st_a, 0);
        // q96: the terms of the 2 m-lane product, argument-major: C | C_I, then A_ | A_ ; sc2: r | alpha, then -w | beta
        uint8_t *C = s.q96, *CI = s.q96 + 96 * m, *A_ = s.q96 + 192 * m;
        if ((rc = c12381_g1_mul_batch_dev(c, m, s.a96, s.sc2, A_, 96))) return rc;
        HIPCK(c, hipMemcpyAsync(A_ + 96 * m, A_, 96 * m, hipMemcpyDeviceToDevice, c->stream));
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = ac_bbs_y_sum(c, m, set, pub, 0, nI, pub.g96, s.sca, CI))) return rc;
        if (nJ) {
            if ((rc = ac_bbs_y_sum(c, m, set, pub, nI, nJ, nullptr, s.sca + 32 * nI * m, s.t96))) return rc;
            if ((rc = ac_bbs_add(c, m, CI, s.t96, C, 96))) return rc;
        } else {
            HIPCK(c, hipMemcpyAsync(C, CI, 96 * m, hipMemcpyDeviceToDevice, c->stream));
        }
        uint8_t *B_ = s.o96, *U = s.o96 + 96 * m;
        if ((rc = c12381_g1_mul_sum_batch_dev(c, 2 * m, 2, s.q96, s.sc2, s.o96, 96, 0u))) return rc;
        if (nJ) {
            if ((rc = ac_bbs_y_sum(c, m, set, pub, nI, nJ, nullptr, s.scd, s.t96))) return rc;
            if ((rc = ac_bbs_add(c, m, U, s.t96, U, 96))) return rc;
        }
        LAUNCH(c, ac_bbs_encode_kernel, m, m, (const uint8_t*)A_, (const uint8_t*)B_, (const uint8_t*)U, s.e49, (uint8_t*)nullptr);
        LAUNCH(c, ac_bbs_challenge_kernel, m, m, msg_len, msg_len ? msgs + msg_len * off : msgs, s.e49, s.tr, s.c32);
        LAUNCH(c, ac_bbs_pres_finish_kernel, m, m, nattr, nJ, set.ord, attr, sig, rn, s.e49, s.c32, s.st, s.st_a, pub.st, pres_243 + 243 * off,
               nJ ? u_48 + 48 * nJ * off : u_48, status + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_bbs_pres_batch(c12381_ctx* c, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243, const uint8_t* Y_49,
                             const uint8_t* attr_48, const uint8_t* sig_97, const uint8_t* msgs, const uint8_t* rnd, uint8_t* pres_243, uint8_t* u_48,
                             uint8_t* status) {
    ac_bbs_set set;
    int rc = bind(c) ?: ac_bbs_pres_args(nattr, nI, idx, msg_len, pk_243, Y_49, attr_48, sig_97, msgs, rnd, pres_243, u_48, status, set);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {Y_49, 49 * nattr}, {attr_48, 48 * nattr * n}, {sig_97, 97 * n}, {msg_len ? msgs : nullptr, msg_len * n},
                         {rnd, 32 * (AC_BBS_PRES_RANDOM + set.nJ) * n}}, {{pres_243, 243 * n}, {u_48, 48 * set.nJ * n}, {status, n}}, [&](const staging& s) {
        return c12381_ac_bbs_pres_batch_dev(c, n, nattr, nI, idx, msg_len, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.out[0], s.out[1], s.out[2]);
    });
}
