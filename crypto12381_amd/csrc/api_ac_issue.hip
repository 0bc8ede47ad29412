// The AC issuance entries of the C ABI (include/c12381_ac_issue.h): issue of the reference's examples/AC-bbs, AC-rbbs and AC-rps and AC-rps'
// user_keygen from their wire formats — everything that produces the credentials the entries of c12381_ac.h consume.  Kernels: k_ac_issue.hip (and
// k_ac_rbbs.hip's encode); the per-lane scalar work: ac_issue.hpp; the shared host pieces: host.hpp.  No exponent of one point is merged into
// another's: every `^` of the reference is one multiplication of the finished point.
#include "host.hpp"

#include "../../include/c12381_ac_issue.h"
#include "ac_issue.hpp"

using namespace c12381;
using namespace c12381_host;

static_assert(AC_ISSUE_MAX_ATTR == C12381_G1_FIXED_SUM_MAX && AC_ISSUE_MAX_ATTR == C12381_G2_FIXED_SUM_MAX, "one fixed-base table per attribute, in G1 and in G2");
constexpr size_t AC_ISSUE_CHUNK = (size_t)1 << 18;

// pk.fixed_part on the side stream: g and tilde_g, tilde_X decoded where they lie in pk_243 (the tuple parse decodes all three); the caller queues
// the used records of its key behind them and joins the side stream before its first use of any of them
static int ac_issue_fixed_part(c12381_ctx* c, const uint8_t* pk_243, const ac_rps_public& pub) {
    int rc;
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, pk_243, pub.g96, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pk_243 + 49, pub.g2, pub.st + 1, 0);
    return 0;
}

// ---------------------------------------------------------------- AC-bbs / AC-rbbs issue (issue.cpp:6-18), nsk = 1 / 2 fields of sk
// Y[0 .. nattr) decoded where they lie in Y_49 on the side stream.  Per credential: the range checks, the attribute columns, w and x + w
// (ac_issue_bbs_prep_kernel), B = g * prod Y_i^a_i as ONE fixed-base sum with the addend g, inverse(x + w) by the simultaneous inversion, A = B^inverse
// as a generic G1 column, the record and the status (ac_issue_bbs_finish_kernel).
static int ac_issue_bbs_args(size_t nattr, const void* sk, const void* pk, const void* Y, const void* attr, const void* rnd, const void* sig, const void* status) {
    return (nattr == 0 || nattr > AC_ISSUE_MAX_ATTR || !sk || !pk || !Y || !attr || !rnd || !sig || !status) ? C12381_E_ARG : 0;
}
static int ac_issue_bbs_dev(c12381_ctx* c, size_t n, size_t nattr, size_t nsk, const uint8_t* sk_48, const uint8_t* pk_243, const uint8_t* Y_49,
                            const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status) {
    int rc = bind(c) ?: ac_issue_bbs_args(nattr, sk_48, pk_243, Y_49, attr_48, rnd_32, sig_97, status);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_ISSUE_CHUNK ? n : AC_ISSUE_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_AC_ISSUE, ac_issue_bbs_layout(nullptr, ch, nattr).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_ISSUE];
    const ac_rps_public pub(d);
    if ((rc = ac_issue_fixed_part(c, pk_243, pub))) return rc;
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nattr, Y_49, pub.y96, pub.st + 3, 0);
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_issue_bbs_slab s = ac_issue_bbs_layout(d, m, nattr);
        LAUNCH(c, ac_issue_bbs_prep_kernel, m, m, nattr, nsk, sk_48, attr_48 + 48 * nattr * off, rnd_32 + 32 * off, s.sca, s.w32, s.d32, s.st, c->d_flag);
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = g1_fixed_sum_range(c, m, nattr, 0, nattr, pub.y96, pub.g96, s.sca, s.b96, 96))) return rc;                  // g * prod Y_i^a_i
        if ((rc = zp_batch_inverse(c, m, s.d32, nullptr, s.inv))) return rc;
        if ((rc = c12381_g1_mul_batch_dev(c, m, s.b96, s.inv, s.a96, 96))) return rc;                                        // A
        LAUNCH(c, ac_issue_bbs_finish_kernel, m, m, 3 + nattr, nsk, (const uint8_t*)pub.st, sk_48, (const uint8_t*)s.st, (const uint8_t*)s.a96,
               (const uint8_t*)s.w32, sig_97 + 97 * off, status + off, c->d_flag);
    }
    return 0;
}
static int ac_issue_bbs_host(c12381_ctx* c, size_t n, size_t nattr, size_t nsk, const uint8_t* sk_48, const uint8_t* pk_243, const uint8_t* Y_49,
                             const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status) {
    int rc = bind(c) ?: ac_issue_bbs_args(nattr, sk_48, pk_243, Y_49, attr_48, rnd_32, sig_97, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{sk_48, 48 * nsk}, {pk_243, 243}, {Y_49, 49 * nattr}, {attr_48, 48 * nattr * n}, {rnd_32, 32 * n}}, {{sig_97, 97 * n}, {status, n}},
                     [&](const staging& s) { return ac_issue_bbs_dev(c, n, nattr, nsk, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.out[0], s.out[1]); });
}
int c12381_ac_bbs_issue_batch_dev(c12381_ctx* c, size_t n, size_t nattr, const uint8_t* sk_48, const uint8_t* pk_243, const uint8_t* Y_49, const uint8_t* attr_48,
                                  const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status) {
    return ac_issue_bbs_dev(c, n, nattr, 1, sk_48, pk_243, Y_49, attr_48, rnd_32, sig_97, status);
}
int c12381_ac_bbs_issue_batch(c12381_ctx* c, size_t n, size_t nattr, const uint8_t* sk_48, const uint8_t* pk_243, const uint8_t* Y_49, const uint8_t* attr_48,
                              const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status) {
    return ac_issue_bbs_host(c, n, nattr, 1, sk_48, pk_243, Y_49, attr_48, rnd_32, sig_97, status);
}
// AC-rbbs: sk = (x, y), both range-checked; of the 2 nattr records of Y_49 the first nattr alone are read (the host form stages no more)
int c12381_ac_rbbs_issue_batch_dev(c12381_ctx* c, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* Y_49, const uint8_t* attr_48,
                                   const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status) {
    return ac_issue_bbs_dev(c, n, nattr, 2, sk_96, pk_243, Y_49, attr_48, rnd_32, sig_97, status);
}
int c12381_ac_rbbs_issue_batch(c12381_ctx* c, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* Y_49, const uint8_t* attr_48,
                               const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status) {
    return ac_issue_bbs_host(c, n, nattr, 2, sk_96, pk_243, Y_49, attr_48, rnd_32, sig_97, status);
}

// ---------------------------------------------------------------- AC-rps user_keygen (user_keygen.cpp:6-14)
// usk = rnd mod r as a scalar column (ac_issue_keygen_prep_kernel), upk = g^usk by g's fixed-base route straight into the caller's records, usk as
// a record and the key check (ac_issue_keygen_finish_kernel)
static int ac_issue_keygen_args(const void* pk, const void* rnd, const void* usk, const void* upk) { return (!pk || !rnd || !usk || !upk) ? C12381_E_ARG : 0; }
int c12381_ac_rps_user_keygen_batch_dev(c12381_ctx* c, size_t n, const uint8_t* pk_243, const uint8_t* rnd_32, uint8_t* usk_48, uint8_t* upk_49) {
    int rc = bind(c) ?: ac_issue_keygen_args(pk_243, rnd_32, usk_48, upk_49);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_ISSUE_CHUNK ? n : AC_ISSUE_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_AC_ISSUE, ac_issue_keygen_layout(nullptr, ch).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_ISSUE];
    const ac_rps_public pub(d);
    if ((rc = ac_issue_fixed_part(c, pk_243, pub))) return rc;
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_issue_keygen_slab s = ac_issue_keygen_layout(d, m);
        LAUNCH(c, ac_issue_keygen_prep_kernel, m, m, rnd_32 + 32 * off, s.sc);
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = c12381_g1_mul_fixed_batch_dev(c, m, pub.g96, s.sc, upk_49 + 49 * off, 49))) return rc;
        LAUNCH(c, ac_issue_keygen_finish_kernel, m, m, (const uint8_t*)pub.st, (const uint8_t*)s.sc, usk_48 + 48 * off, upk_49 + 49 * off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rps_user_keygen_batch(c12381_ctx* c, size_t n, const uint8_t* pk_243, const uint8_t* rnd_32, uint8_t* usk_48, uint8_t* upk_49) {
    int rc = bind(c) ?: ac_issue_keygen_args(pk_243, rnd_32, usk_48, upk_49);
    if (rc || n == 0) return rc;
    return host_form(c, {{pk_243, 243}, {rnd_32, 32 * n}}, {{usk_48, 48 * n}, {upk_49, 49 * n}},
                     [&](const staging& s) { return c12381_ac_rps_user_keygen_batch_dev(c, n, s.in[0], s.in[1], s.out[0], s.out[1]); });
}

// ---------------------------------------------------------------- AC-rps issue (issue.cpp:6-39)
// tilde_Y[0 .. nattr) decoded where they lie in tY_97 on the side stream.  Per credential: the range checks, the attribute columns, alpha and the
// scalars x + ym | alpha y^(nattr+1) (ac_issue_rps_prep_kernel); Z decoded straight from the caller's upk records into the second term column;
// h = g^alpha by g's fixed-base route into the first; h re-encoded; sigma as ONE k = 2 product over (h, Z); tilde_M as the G2 fixed-base sum with no
// addend; the record and the status (ac_issue_rps_finish_kernel).
static int ac_issue_rps_args(size_t nattr, const void* sk, const void* pk, const void* tY, const void* upk, const void* attr, const void* rnd, const void* sig,
                             const void* status) {
    return (nattr == 0 || nattr > AC_ISSUE_MAX_ATTR || !sk || !pk || !tY || !upk || !attr || !rnd || !sig || !status) ? C12381_E_ARG : 0;
}
int c12381_ac_rps_issue_batch_dev(c12381_ctx* c, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* tY_97, const uint8_t* upk_49,
                                  const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_195, uint8_t* status) {
    int rc = bind(c) ?: ac_issue_rps_args(nattr, sk_96, pk_243, tY_97, upk_49, attr_48, rnd_32, sig_195, status);
    if (rc || n == 0) return rc;
    const size_t ch = n < AC_ISSUE_CHUNK ? n : AC_ISSUE_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_AC_ISSUE, ac_issue_rps_layout(nullptr, ch, nattr).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_AC_ISSUE];
    const ac_rps_public pub(d);
    if ((rc = ac_issue_fixed_part(c, pk_243, pub))) return rc;
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, nattr, tY_97, pub.ty192, pub.st + 3, 0);
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const ac_issue_rps_slab s = ac_issue_rps_layout(d, m, nattr);
        uint8_t *h96 = s.q96, *z96 = s.q96 + 96 * m;
        LAUNCH(c, ac_issue_rps_prep_kernel, m, m, nattr, sk_96, attr_48 + 48 * nattr * off, rnd_32 + 32 * off, s.sca, s.al32, s.sc2, s.st, c->d_flag);
        LAUNCH(c, g1_decompress_kernel, m, m, upk_49 + 49 * off, z96, s.st_z, 0);
        if (off == 0 && (rc = join_side(c))) return rc;
        if ((rc = c12381_g1_mul_fixed_batch_dev(c, m, pub.g96, s.al32, h96, 96))) return rc;                                  // h
        LAUNCH(c, ac_rbbs_encode_kernel, m, m, (size_t)1, (const uint8_t*)h96, s.e49);
        if ((rc = c12381_g1_mul_sum_batch_dev(c, m, 2, s.q96, s.sc2, s.e49 + 49 * m, 49, 0u))) return rc;                     // sigma
        if ((rc = g2_fixed_sum_range(c, m, nattr, 0, nattr, pub.ty192, nullptr, s.sca, s.tm97, 97))) return rc;               // tilde_M
        LAUNCH(c, ac_issue_rps_finish_kernel, m, m, 3 + nattr, (const uint8_t*)pub.st, sk_96, (const uint8_t*)s.st, (const uint8_t*)s.st_z, (const uint8_t*)s.e49,
               (const uint8_t*)s.tm97, sig_195 + 195 * off, status + off, c->d_flag);
    }
    return 0;
}
int c12381_ac_rps_issue_batch(c12381_ctx* c, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* tY_97, const uint8_t* upk_49,
                              const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_195, uint8_t* status) {
    int rc = bind(c) ?: ac_issue_rps_args(nattr, sk_96, pk_243, tY_97, upk_49, attr_48, rnd_32, sig_195, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{sk_96, 96}, {pk_243, 243}, {tY_97, 97 * nattr}, {upk_49, 49 * n}, {attr_48, 48 * nattr * n}, {rnd_32, 32 * n}},
                     {{sig_195, 195 * n}, {status, n}}, [&](const staging& s) {
        return c12381_ac_rps_issue_batch_dev(c, n, nattr, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.out[0], s.out[1]);
    });
}
