// The PS entries of the C ABI (include/c12381_hip.h): batch verification on decoded columns, and verify / sign / randomnize from the wire formats with
// the aggregate verdict.  Kernels: k_ps.hip; the shared host pieces: host.hpp.
#include "host.hpp"

using namespace c12381;
using namespace c12381_host;

// ---------------------------------------------------------------- PS batch verification
// ok[j] = [ e(s1_j, X2 + sum_i m[i*n + j] Y2_i) == e(s2_j, g2) ]: the PS verification of the reference's examples/ps/src/ps.cpp:84-99
// (nmsg = 1: :26-33), evaluated as liner_pair.hpp:336-350 (two Miller values, conjugate, multiply, one final exponentiation, is_unity).
// Fast route — g2, X2 and every Y2_i elements of G2 other than infinity, nmsg + 2 <= C12381_FIXED_G2_MAX: the argument of the BBS+ path
// (bilinearity in the G2 argument holds for every curve point s1, and the cofactor part of a GLV multiple m_i s1 pairs to 1 against G2)
// turns the equation into  e(-s2, g2) * e(s1, X2) * prod_i e(m_i s1, Y2_i) == 1,  ONE K = nmsg + 2 way product over line tables.
// Generic route — anything else: W_j = X2 + sum_i m_ij Y2_i, then the pair_eq kernels.  With more messages than the product takes
// (C12381_FIXED_G2_MAX - 2 < nmsg <= C12381_G2_FIXED_SUM_MAX) W is ONE per-lane sum over the shared bases Y2 with the addend X2
// (c12381_g2_mul_fixed_sum_batch_dev: nmsg tables for keys in G2, its own generic columns otherwise; an off-twist key marks every W 0xff and
// raises the status word, and pair_eq turns a 0xff W into a 0xff lane).  Otherwise by the G2 multiplication and addition kernels per column.
// The gate over the K tables picks the route on the device: every kernel of both routes is enqueued and the other route's return at once.
static int ps_verify_args(size_t nmsg, const void* g2, const void* X2, const void* Y2, const void* s1, const void* s2, const void* m, const void* ok) {
    return (!g2 || !X2 || !s1 || !s2 || !ok || (nmsg && (!Y2 || !m))) ? C12381_E_ARG : 0;
}
// The body, on checked arguments.  X2 may be absent (host.hpp ps_verify_core: the second pairing equation of AC-rbbs, api_ac_rbbs.hip): the
// product then has the nmsg + 1 factors e(-s2, g2), e(m_i s1, Y2_i) over the tables of g2, Y2_0 .., and W is the plain sum (infinity for nmsg = 0).
int c12381_host::ps_verify_core(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                                const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, uint8_t* ok) {
    int rc;
    const size_t fixed = X2_192 ? 2 : 1;              // factors of the product that take no message scalar
    const bool fast = nmsg + fixed <= (size_t)C12381_FIXED_G2_MAX;
    const int k = (int)(nmsg + fixed);
    const int32_t *gate_generic = nullptr, *gate_fast = nullptr;
    cached t = {};
    if (fast) {
        g2_cols q = {};                               // without X2: g2, Y2_0 .. (up to FIXED_G2_MAX - 1 messages)
        if (X2_192) q = g2_key_cols(g2_192, X2_192, Y2_192, nmsg);
        else { q.p[0] = g2_192; for (size_t i = 0; i < nmsg; ++i) q.p[1 + i] = Y2_192 + 192 * i; }
        if ((rc = lines_tables_k(c, k, q, 1, t))) return rc;
        gate_generic = t.gate;                // generic kernels: skip when every table is valid
        gate_fast = t.gate + GATE_OTHER;      // fast-route kernels with a skip pointer: skip when one is not
    }
    // generic route: W = X2 + sum_i m_i Y2_i (WS_BBS_Q), each product in WS_BBS_B
    if ((rc = ensure(c, c12381_ctx::WS_BBS_Q, 192 * n))) return rc;
    uint8_t* d_w = (uint8_t*)c->ws[c12381_ctx::WS_BBS_Q];
    if (nmsg == 0 && !X2_192) {
        HIPCK(c, hipMemsetAsync(d_w, 0, 192 * n, c->stream));
    } else if (nmsg == 0) {
        LAUNCH(c, g2_bcast_kernel, 192 * n, n, X2_192, d_w, gate_generic);
    } else if (!fast && nmsg <= (size_t)C12381_G2_FIXED_SUM_MAX) {
        if ((rc = g2_fixed_sum_range(c, n, nmsg, 0, nmsg, Y2_192, X2_192, m_32, d_w, 192))) return rc;
    } else {
        if ((rc = ensure(c, c12381_ctx::WS_BBS_B, 192 * n))) return rc;
        uint8_t* d_b = (uint8_t*)c->ws[c12381_ctx::WS_BBS_B];
        for (size_t i = 0; i < nmsg; ++i) {
            const bool first_alone = i == 0 && !X2_192;       // no X2: the first product is W so far
            if ((rc = g2_mul_dev_strided(c, n, Y2_192 + 192 * i, 0, m_32 + 32 * n * i, first_alone ? d_w : d_b, 192, gate_generic))) return rc;
            if (first_alone) continue;
            LAUNCH(c, g2_add_kernel, n, n, i == 0 ? X2_192 : (const uint8_t*)d_w, (size_t)(i == 0 ? 0 : 192), (const uint8_t*)d_b, d_w, 192, c->d_flag, gate_generic);
        }
    }
    if (fast) {
        // fast route: the columns -s2 (against g2), s1 (X2), m_i s1 (Y2_i); m_i s1 by the generic G1 multiplication into WS_PROJ, then affine
        g1_cols cols = {};
        cols.p[0] = s2_96;
        if (X2_192) cols.p[1] = s1_96;
        if (nmsg) {
            const size_t stride = round_up(nmsg * n, 64);
            for (size_t i = 0; i < nmsg; ++i)
                if ((rc = g1_mul_to_proj(c, n, s1_96, m_32 + 32 * n * i, stride, 96, i * n, gate_fast))) return rc;
            if ((rc = ensure(c, c12381_ctx::WS_FQK_G1, 96 * nmsg * n))) return rc;
            uint8_t* d_m = (uint8_t*)c->ws[c12381_ctx::WS_FQK_G1];
            if ((rc = g1_finish(c, nmsg * n, (const int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, d_m, 96))) return rc;
            for (size_t i = 0; i < nmsg; ++i) cols.p[fixed + i] = d_m + 96 * n * i;
        }
        timed tm(c, 4);
        if ((rc = launch_prodk(c, n, k, cols, 1u, t, ok, true, false, gate_fast))) return rc;
    }
    timed tm(c, 4);
    return launch_pair_eq(c, n, s1_96, d_w, s2_96, g2_192, (size_t)0, ok, gate_generic);
}
int c12381_ps_verify_batch_dev(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                               const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, uint8_t* ok) {
    int rc = bind(c) ?: ps_verify_args(nmsg, g2_192, X2_192, Y2_192, s1_96, s2_96, m_32, ok);
    if (rc || n == 0) return rc;
    return ps_verify_core(c, n, nmsg, g2_192, X2_192, Y2_192, s1_96, s2_96, m_32, ok);
}
int c12381_ps_verify_batch(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                           const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, uint8_t* ok) {
    int rc = bind(c) ?: ps_verify_args(nmsg, g2_192, X2_192, Y2_192, s1_96, s2_96, m_32, ok);
    if (rc || n == 0) return rc;
    return host_form(c, {{g2_192, 192}, {X2_192, 192}, {Y2_192, 192 * nmsg}, {s1_96, 96 * n}, {s2_96, 96 * n}, {m_32, 32 * n * nmsg}}, {{ok, n}},
                     [&](const staging& s) { return c12381_ps_verify_batch_dev(c, n, nmsg, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.out[0]); });
}

// ---------------------------------------------------------------- PS from the wire formats: verify, sign, randomnize; the aggregate verdict
// What a caller of examples/ps/src/ps.cpp holds: 98-byte signatures serialize(σ1, σ2), 97-byte key points, 48-byte Zp secrets, raw message
// bytes.  WS_PS is the workspace of all four entries (none calls another).  msg_mode -> number of message scalars (ps.hpp ps_msg_scalars):
// C12381_PS_MSG_HASH one digest, nY = 1 required; C12381_PS_MSG_ENCODE ceil(msg_len / 31) units, more than nY is "message is too long".
static_assert(C12381_PS_MSG_HASH == 0 && C12381_PS_MSG_ENCODE == 1, "ps.hpp PS_MSG_HASH / PS_MSG_ENCODE");
static int ps_msg_units(int mode, size_t nY, size_t msg_len, size_t& units) {
    if (mode == C12381_PS_MSG_HASH) { units = 1; return nY == 1 ? 0 : C12381_E_ARG; }
    if (mode != C12381_PS_MSG_ENCODE) return C12381_E_ARG;
    units = (msg_len + 30) / 31;
    return units > nY ? C12381_E_ARG : 0;
}
// verify (ps.cpp:26-33, :84-99): ps_wire_prep_kernel and the 2 n square roots of the signatures on the context's stream, the 2 + units public
// points on the side stream (three launches of the G2 decompression kernel straight from the caller's pointers), c12381_ps_verify_batch_dev
// on the decoded columns, ps_wire_finish_kernel for the 0xff lanes.  Only the Y2 entries the message uses are decoded.
static int ps_wire_args(size_t nY, size_t msg_len, int mode, const void* g2, const void* X2, const void* Y2, const void* sig, const void* msgs, const void* ok,
                        size_t& units) {
    if (!g2 || !X2 || !sig || !ok || (nY && !Y2) || (msg_len && !msgs)) return C12381_E_ARG;
    return ps_msg_units(mode, nY, msg_len, units);
}
int c12381_ps_verify_wire_batch_dev(c12381_ctx* c, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* g2_97, const uint8_t* X2_97,
                                    const uint8_t* Y2_97, const uint8_t* sig_98, const uint8_t* msgs, uint8_t* ok) {
    size_t units = 0;
    int rc = bind(c) ?: ps_wire_args(nY, msg_len, msg_mode, g2_97, X2_97, Y2_97, sig_98, msgs, ok, units);
    if (rc || n == 0) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_PS, ps_wire_layout(nullptr, n, units).bytes))) return rc;
    const ps_wire_slab d = ps_wire_layout(c->ws[c12381_ctx::WS_PS], n, units);
    if ((rc = fork_side(c))) return rc;                                     // the caller's inputs are ordered on the context's stream
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, g2_97, d.p192, d.stp, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)1, X2_97, d.p192 + 192, d.stp + 1, 0);
    if (units) LAUNCH_ON(c, g2_decompress_kernel, dim3(grid_for(units)), dim3(BLOCK), c->side, units, Y2_97, d.p192 + 384, d.stp + 2, 0);
    LAUNCH(c, ps_wire_prep_kernel, n, n, msg_len, msg_mode, units, sig_98, msgs, d.s49, d.m);
    LAUNCH(c, g1_decompress_kernel, 2 * n, 2 * n, d.s49, d.s96, d.st, 0);
    if ((rc = join_side(c))) return rc;
    if ((rc = c12381_ps_verify_batch_dev(c, n, units, d.p192, d.p192 + 192, d.p192 + 384, d.s96, d.s96 + 96 * n, d.m, ok))) return rc;
    LAUNCH(c, ps_wire_finish_kernel, n, n, 2 + units, d.st, d.stp, ok, c->d_flag);
    return 0;
}
int c12381_ps_verify_wire_batch(c12381_ctx* c, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* g2_97, const uint8_t* X2_97,
                                const uint8_t* Y2_97, const uint8_t* sig_98, const uint8_t* msgs, uint8_t* ok) {
    size_t units = 0;
    int rc = bind(c) ?: ps_wire_args(nY, msg_len, msg_mode, g2_97, X2_97, Y2_97, sig_98, msgs, ok, units);
    if (rc || n == 0) return rc;
    return host_form(c, {{g2_97, 97}, {X2_97, 97}, {Y2_97, 97 * nY}, {sig_98, 98 * n}, {msg_len ? msgs : nullptr, msg_len * n}}, {{ok, n}},
                     [&](const staging& s) { return c12381_ps_verify_wire_batch_dev(c, n, nY, msg_len, msg_mode, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.out[0]); });
}
// sign (ps.cpp:17-24, :68-82).  The reference's h = random-select_in<*G1> is the default generator raised to a random scalar t
// (g1_point.hpp:355-369), so (σ1, σ2) = (G^t, (G^t)^e) = (G^t, G^(t e)), e = x + sum_i y_i m_i: G^t lies in G1, where multiply() is the plain
// multiple.  ps_sign_prep_kernel writes t_j and t_j e_j interleaved; ONE fixed-base column of 2 n lanes on G (consts.hpp, written out by
// ps_generator_kernel) with 49-byte output is the array of 98-byte signatures.  G's table has fixed-base slot PS_GEN_SLOT to itself: no
// other entry builds a table there, and sign builds none elsewhere, so it neither evicts nor loses a table to c12381_g1_mul_fixed_batch,
// BBS+ or bbs04.
static int ps_sign_args(size_t nY, size_t msg_len, int mode, const void* x, const void* y, const void* msgs, const void* t, const void* sig, size_t& units) {
    if (!x || !t || !sig || (nY && !y) || (msg_len && !msgs)) return C12381_E_ARG;
    return ps_msg_units(mode, nY, msg_len, units);
}
int c12381_ps_sign_batch_dev(c12381_ctx* c, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* x_48, const uint8_t* y_48, const uint8_t* msgs,
                             const uint8_t* t_32, uint8_t* sig_98) {
    size_t units = 0;
    int rc = bind(c) ?: ps_sign_args(nY, msg_len, msg_mode, x_48, y_48, msgs, t_32, sig_98, units);
    if (rc || n == 0) return rc;
    proj_slab w;
    if ((rc = ensure(c, c12381_ctx::WS_PS, ps_sign_layout(nullptr, n).bytes)) || (rc = proj_ws(c, 2 * n, w))) return rc;
    const ps_sign_slab d = ps_sign_layout(c->ws[c12381_ctx::WS_PS], n);
    LAUNCH_ON(c, ps_generator_kernel, dim3(1), dim3(BLOCK), c->stream, d.gen);
    LAUNCH(c, ps_sign_prep_kernel, n, n, units, msg_len, msg_mode, x_48, y_48, msgs, t_32, d.sc, d.key, c->d_flag);
    const bool fb = fixed_base_enabled();
    if (fb && (rc = g1_fixed_table(c, PS_GEN_SLOT, d.gen))) return rc;
    if ((rc = g1_fixed_column(c, 2 * n, d.gen, PS_GEN_SLOT, d.sc, w.stride, 0, fb))) return rc;
    if ((rc = g1_finish(c, 2 * n, w.p, w.stride, sig_98, 49))) return rc;
    LAUNCH(c, ps_sign_finish_kernel, n, n, (const uint8_t*)d.key, sig_98);
    return 0;
}
int c12381_ps_sign_batch(c12381_ctx* c, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* x_48, const uint8_t* y_48, const uint8_t* msgs,
                         const uint8_t* t_32, uint8_t* sig_98) {
    size_t units = 0;
    int rc = bind(c) ?: ps_sign_args(nY, msg_len, msg_mode, x_48, y_48, msgs, t_32, sig_98, units);
    if (rc || n == 0) return rc;
    return host_form(c, {{x_48, 48}, {y_48, 48 * nY}, {msg_len ? msgs : nullptr, msg_len * n}, {t_32, 32 * n}}, {{sig_98, 98 * n}},
                     [&](const staging& s) { return c12381_ps_sign_batch_dev(c, n, nY, msg_len, msg_mode, s.in[0], s.in[1], s.in[2], s.in[3], s.out[0]); });
}
// randomnize (ps.cpp:35-40): (σ1^r, σ2^r), `^` = multiply.  The 98-byte signatures ARE 2 n records of 49 bytes: decode them in place, one
// generic column of 2 n lanes (r_j for both lanes of signature j), 49-byte output straight into out_98.  A record that does not decode
// multiplies as infinity and raises nothing; ps_randomize_finish_kernel marks its signature.
static int ps_randomize_args(const void* sig, const void* r, const void* out, const void* status) { return (!sig || !r || !out || !status) ? C12381_E_ARG : 0; }
int c12381_ps_randomize_batch_dev(c12381_ctx* c, size_t n, const uint8_t* sig_98, const uint8_t* r_32, uint8_t* out_98, uint8_t* status) {
    int rc = bind(c) ?: ps_randomize_args(sig_98, r_32, out_98, status);
    if (rc || n == 0) return rc;
    const size_t stride = round_up(2 * n, 64);
    if ((rc = ensure(c, c12381_ctx::WS_PS, ps_randomize_layout(nullptr, n).bytes))) return rc;
    const ps_randomize_slab d = ps_randomize_layout(c->ws[c12381_ctx::WS_PS], n);
    LAUNCH(c, g1_decompress_kernel, 2 * n, 2 * n, sig_98, d.s96, d.st, 0);
    LAUNCH(c, ps_randomize_prep_kernel, n, n, r_32, d.sc);
    if ((rc = g1_mul_to_proj(c, 2 * n, d.s96, d.sc, stride))) return rc;
    if ((rc = g1_finish(c, 2 * n, (const int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, out_98, 49))) return rc;
    LAUNCH(c, ps_randomize_finish_kernel, n, n, (const uint8_t*)d.st, out_98, status);
    return 0;
}
int c12381_ps_randomize_batch(c12381_ctx* c, size_t n, const uint8_t* sig_98, const uint8_t* r_32, uint8_t* out_98, uint8_t* status) {
    int rc = bind(c) ?: ps_randomize_args(sig_98, r_32, out_98, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{sig_98, 98 * n}, {r_32, 32 * n}}, {{out_98, 98 * n}, {status, n}},
                     [&](const staging& s) { return c12381_ps_randomize_batch_dev(c, n, s.in[0], s.in[1], s.out[0], s.out[1]); });
}
// Aggregate verdict (optional, as BBS+'s; the reference verifies one signature per call, ps.cpp:84-99).  With caller-drawn rho_j,
//   prod_j [ e(-σ2_j, g2) e(σ1_j, X2) prod_i e(m_ij σ1_j, Y2_i) ]^rho_j
//     = e(-sum_j rho_j σ2_j, g2) * e(sum_j rho_j σ1_j, X2) * prod_i e(sum_j (rho_j m_ij) σ1_j, Y2_i):
// nmsg scalar columns rho_j m_ij (zp_op_kernel), nmsg + 2 bucket products over the signature points, one negation (the prep kernel's
// neg_mask) and ONE (nmsg + 2)-way product over the line tables of c12381_ps_verify_batch's fast route with n = 1.
// Completeness: the factor of lane j is the rho_j-th power of the product that route tests, so a batch it accepts in every lane yields 1.
// The bucket products go through multiply()'s GLV form; off the subgroup that adds cofactor points to a sum, and so does every cofactor
// component of a σ itself: all of them pair to 1 against elements of G2, which is why the keys must be in G2 (the tables' rule 1: a key
// outside G2 or at infinity leaves the gate shut and the verdict 0).  Soundness: a rejected lane has a factor f_j != 1 of prime order r, and
// prod_j f_j^rho_j = 1 fixes rho_j mod r given the others: probability at most 2^-k over k-bit uniform rho_j (k <= 254).
// all_ok = 0 settles nothing: an invalid signature, a key outside G2, or a point off the curve (the bucket products leave it out and raise
// C12381_E_POINT; ps_aggregate_finish_kernel then clears the verdict) — run c12381_ps_verify_batch.
static int ps_aggregate_args(size_t n, size_t nmsg, const void* g2, const void* X2, const void* Y2, const void* s1, const void* s2, const void* m, const void* rho,
                             const void* all_ok) {
    if (!g2 || !X2 || !all_ok || (nmsg && !Y2) || (n && (!s1 || !s2 || !rho || (nmsg && !m)))) return C12381_E_ARG;
    return nmsg + 2 > (size_t)C12381_FIXED_G2_MAX ? C12381_E_ARG : 0;
}
int c12381_ps_verify_aggregate_dev(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192, const uint8_t* s1_96,
                                   const uint8_t* s2_96, const uint8_t* m_32, const uint8_t* rho_32, uint8_t* all_ok) {
    int rc = bind(c) ?: ps_aggregate_args(n, nmsg, g2_192, X2_192, Y2_192, s1_96, s2_96, m_32, rho_32, all_ok);
    if (rc) return rc;
    if (n == 0) { HIPCK(c, hipMemsetAsync(all_ok, 1, 1, c->stream)); return 0; }
    HIPCK(c, hipMemsetAsync(all_ok, 0, 1, c->stream));
    const int k = (int)nmsg + 2;
    cached t;
    if ((rc = lines_tables_k(c, k, g2_key_cols(g2_192, X2_192, Y2_192, nmsg), 1, t))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_PS, ps_aggregate_layout(nullptr, n, (size_t)k).bytes))) return rc;
    const ps_aggregate_slab d = ps_aggregate_layout(c->ws[c12381_ctx::WS_PS], n, (size_t)k);
    g1_cols cols = {};
    for (int j = 0; j < k; ++j) cols.p[j] = d.sum + 96 * j;
    if ((rc = c12381_g1_msm_dev(c, n, s2_96, rho_32, d.sum, 96))) return rc;
    if ((rc = c12381_g1_msm_dev(c, n, s1_96, rho_32, d.sum + 96, 96))) return rc;
    for (size_t i = 0; i < nmsg; ++i) {
        LAUNCH(c, zp_op_kernel, n, 0, n, rho_32, m_32 + 32 * n * i, d.col);
        if ((rc = c12381_g1_msm_dev(c, n, s1_96, d.col, d.sum + 96 * (2 + i), 96))) return rc;
    }
    if ((rc = launch_prodk(c, 1, k, cols, 1u, t, all_ok, true, false, t.gate + GATE_OTHER))) return rc;
    LAUNCH_ON(c, ps_aggregate_finish_kernel, dim3(1), dim3(BLOCK), c->stream, all_ok, (const int*)c->d_flag);
    return 0;
}
int c12381_ps_verify_aggregate(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192, const uint8_t* s1_96,
                               const uint8_t* s2_96, const uint8_t* m_32, const uint8_t* rho_32, int* all_ok) {
    int rc = bind(c) ?: ps_aggregate_args(n, nmsg, g2_192, X2_192, Y2_192, s1_96, s2_96, m_32, rho_32, all_ok);
    if (rc) return rc;
    *all_ok = 0;
    if (n == 0) { *all_ok = 1; return 0; }
    uint8_t verdict = 0;
    rc = host_form(c, {{g2_192, 192}, {X2_192, 192}, {Y2_192, 192 * nmsg}, {s1_96, 96 * n}, {s2_96, 96 * n}, {m_32, 32 * n * nmsg}, {rho_32, 32 * n}},
                   {{&verdict, 1}}, [&](const staging& s) {      // synchronises the stream
        return c12381_ps_verify_aggregate_dev(c, n, nmsg, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.out[0]);
    });
    *all_ok = (rc == 0 && verdict == 1) ? 1 : 0;
    return rc;
}
