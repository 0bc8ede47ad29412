// The BBS+ entries of the C ABI (include/c12381_hip.h): batch verification, verification from the wire formats, the aggregate verdict and signing.
// The shared host pieces: host.hpp.
#include "host.hpp"
#include "fp.hpp"

using namespace c12381;
using namespace c12381_host;

// B_j = g1 + r_j h0 + sum_i m_ij h_i for a batch of BBS+ signatures (bbs+.cpp:51, :72): (nmsg + 1) columns of n scalar
// multiplications with ONE base each — table-driven for subgroup bases, generic otherwise — summed per lane.  Result:
// projective SoA in WS_RED0 (`red`, stride `rstride`); `stride` is the stride of the column workspace WS_PROJ.
static int bbs_message_points(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* h0_96, const uint8_t* h_96, const uint8_t* r_32,
                              const uint8_t* m_32, bool fb, int32_t*& red, size_t& rstride, size_t& stride) {
    int rc;
    const size_t cols = nmsg + 1, total = cols * n;
    proj_slab w;
    if ((rc = proj_ws(c, total, w))) return rc;
    stride = w.stride;
    for (size_t col = 0; col < cols; ++col) {
        const uint8_t* base = col == 0 ? h0_96 : h_96 + 96 * (col - 1);
        const uint8_t* sc = col == 0 ? r_32 : m_32 + 32 * n * (col - 1);
        const bool tab = fb && col < 4;                        // table slots for h0 and the first three h_i, the generic kernel beyond
        if (tab && (rc = g1_fixed_table(c, (int)col, base))) return rc;
        if ((rc = g1_fixed_column(c, n, base, (int)col, sc, stride, col * n, tab))) return rc;
    }
    rstride = round_up(n, 64);
    if ((rc = ensure(c, c12381_ctx::WS_RED0, (size_t)3 * NL * rstride * 4))) return rc;
    red = (int32_t*)c->ws[c12381_ctx::WS_RED0];
    LAUNCH(c, g1_reduce_kernel, n, total, (const int32_t*)w.p, stride, n, red, rstride);
    LAUNCH(c, g1_add_const_kernel, n, n, red, rstride, g1_96, c->d_flag);
    return 0;
}

// ---------------------------------------------------------------- BBS+ batch verification
// ok[j] = [ e(A_j, w + x_j g2) == e(g1 + r_j h0 + sum_i m_{i,j} h_i, g2) ]   — the verification equation of the
// reference's examples/bbs-plus/src/bbs+.cpp:57-73, evaluated as liner_pair.hpp:339-350 does (two Miller loops,
// one final exponentiation).  Message scalars are message-major: m[i*n + j] belongs to signature j.  All
// pointers are DEVICE pointers; the public parameters are single points.
static int bbs_verify_args(size_t nmsg, const void* g1_96, const void* g2_192, const void* h0_96, const void* h_96, const void* w_192, const void* A_96,
                           const void* x_32, const void* r_32, const void* m_32, const void* ok) {
    return (!g1_96 || !g2_192 || !h0_96 || !w_192 || !A_96 || !x_32 || !r_32 || !ok || (nmsg && (!h_96 || !m_32))) ? C12381_E_ARG : 0;
}
int c12381_bbs_plus_verify_batch_dev(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192, const uint8_t* h0_96,
                                     const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96, const uint8_t* x_32, const uint8_t* r_32,
                                     const uint8_t* m_32, uint8_t* ok) {
    int rc = bind(c) ?: bbs_verify_args(nmsg, g1_96, g2_192, h0_96, h_96, w_192, A_96, x_32, r_32, m_32, ok);
    if (rc || n == 0) return rc;
    // Q_j = w + x_j g2
    if ((rc = ensure(c, c12381_ctx::WS_BBS_Q, 192 * n))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_BBS_B, 192 * n))) return rc;
    uint8_t* d_q = (uint8_t*)c->ws[c12381_ctx::WS_BBS_Q];
    uint8_t* d_b = (uint8_t*)c->ws[c12381_ctx::WS_BBS_B];
    // Both G2 arguments of the equation are public points.  When g2 and w are elements of G2 the equation is evaluated
    // as e(A, w) * e(x A - B, g2) == 1 (bilinearity in the G2 argument holds for every point A of the curve, and the
    // cofactor part of the GLV multiple x A pairs to 1), so BOTH Miller loops run against fixed G2 points: their line
    // coefficients come from two 69-entry tables, no G2 arithmetic per signature at all.  Otherwise — the reference
    // checks nothing — the generic path below evaluates e(A, w + x g2) == e(B, g2) exactly as written.  `gate` selects:
    // every kernel of either path reads it and returns at once if it belongs to the other path.
    const bool fb = fixed_base_enabled();
    const bool fq = fb && pair_lanes() != 1;
    const int32_t *gate_fast = nullptr, *gate_generic = nullptr;      // skip_if pointers: skip when [HDR_VALID] != 0
    cached lines = {};
    if (fq) {
        if ((rc = bbs_lines_tables(c, w_192, g2_192, lines))) return rc;
        gate_generic = lines.gate;            // generic kernels: skip when the fixed-G2 path is valid
        gate_fast = lines.gate + GATE_OTHER;  // kernels that exist only for the fixed-G2 path and take a skip pointer: skip when it is not
    }
    // generic path: Q_j = w + x_j g2 (g2's multiples from its fixed-base table when it is a subgroup point)
    const int32_t* skip_g2 = nullptr;
    if (fb && !fq) {
        cached t;
        if ((rc = g2_fixed_table(c, g2_192, t))) return rc;
        skip_g2 = t.tabs;
        LAUNCH(c, g2_fixed_eval_kernel, n, n, skip_g2, x_32, w_192, d_q, 192, c->d_flag, (int32_t*)nullptr, (size_t)0);
    }
    if ((rc = g2_mul_dev_strided(c, n, g2_192, 0, x_32, d_b, 192, fq ? gate_generic : skip_g2))) return rc;
    LAUNCH(c, g2_add_kernel, n, n, w_192, (size_t)0, d_b, d_q, 192, c->d_flag, fq ? gate_generic : skip_g2);
    int32_t* red; size_t rstride, stride;
    if ((rc = bbs_message_points(c, n, nmsg, g1_96, h0_96, h_96, r_32, m_32, fb, red, rstride, stride))) return rc;
    if (fq) {
        // fixed-G2 path: red <- x A - B  (x A by the generic scalar multiplication: A differs per signature)
        if ((rc = g1_mul_to_proj(c, n, A_96, x_32, stride, 96, 0, gate_fast))) return rc;
        LAUNCH(c, g1_rsub_kernel, n, n, red, rstride, (const int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, (size_t)0, gate_generic);
    }
    if ((rc = g1_finish(c, n, red, rstride, d_b, 96))) return rc;
    timed tm(c, 4);
    if (fq && (rc = launch_prod_fixed(c, n, A_96, d_b, lines, ok, gate_generic))) return rc;
    return launch_pair_eq(c, n, A_96, d_q, d_b, g2_192, (size_t)0, ok, gate_generic);
}
int c12381_bbs_plus_verify_batch(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192, const uint8_t* h0_96,
                                 const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96, const uint8_t* x_32, const uint8_t* r_32,
                                 const uint8_t* m_32, uint8_t* ok) {
    int rc = bind(c) ?: bbs_verify_args(nmsg, g1_96, g2_192, h0_96, h_96, w_192, A_96, x_32, r_32, m_32, ok);
    if (rc || n == 0) return rc;
    return host_form(c,
                     {{g1_96, 96}, {g2_192, 192}, {h0_96, 96}, {h_96, 96 * nmsg}, {w_192, 192}, {A_96, 96 * n}, {x_32, 32 * n}, {r_32, 32 * n}, {m_32, 32 * n * nmsg}},
                     {{ok, n}},
                     [&](const staging& s) { return c12381_bbs_plus_verify_batch_dev(c, n, nmsg, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.in[7], s.in[8], s.out[0]); });
}

// ---------------------------------------------------------------- BBS+ verification from the wire formats
// The whole caller pattern of examples/bbs-plus/src/bbs+.cpp:57-73 on ONE stream: decode the public points and the signatures'
// A (g1/g2_decompress_kernel), parse x and r, encode the message bytes (bbs_wire_prep_kernel), then the
// verification pipeline above (f2).  Every message has msg_len bytes (ceil(msg_len / 31) units; more units than h entries is
// the reference's "message is too long": C12381_E_ARG).  ok[j] = 1 / 0, or 0xff where the reference would throw.
static int bbs_wire_args(size_t nh, size_t msg_len, const void* g1_g2_h0_195, const void* h_49, const void* pk_97, const void* sig_145, const void* msgs,
                         const void* ok) {
    return (!g1_g2_h0_195 || !pk_97 || !sig_145 || !ok || (nh && !h_49) || (msg_len && !msgs) || (msg_len + 30) / 31 > nh) ? C12381_E_ARG : 0;
}
int c12381_bbs_plus_verify_wire_batch_dev(c12381_ctx* c, size_t n, size_t nh, size_t msg_len, const uint8_t* g1_g2_h0_195, const uint8_t* h_49,
                                          const uint8_t* pk_97, const uint8_t* sig_145, const uint8_t* msgs, uint8_t* ok) {
    int rc = bind(c) ?: bbs_wire_args(nh, msg_len, g1_g2_h0_195, h_49, pk_97, sig_145, msgs, ok);
    if (rc || n == 0) return rc;
    const size_t nblk = (msg_len + 30) / 31, npub1 = 2 + nblk;
    if ((rc = ensure(c, c12381_ctx::WS_BBS_WIRE, bbs_wire_layout(nullptr, n, nblk).bytes))) return rc;
    const bbs_wire_slab d = bbs_wire_layout(c->ws[c12381_ctx::WS_BBS_WIRE], n, nblk);
    // The handful of public points decode on the side stream: two square-root chains of one lane each (0.4 + 0.85 ms of pure latency) beside
    // the parsing and the n square roots of the signatures' A on the context's stream, instead of in front of them.
    if ((rc = fork_side(c))) return rc;                                     // the caller's inputs are ordered on the context's stream
    LAUNCH_ON(c, bbs_wire_pub_kernel, dim3(grid_for(49 * npub1 + 2 * 97)), dim3(BLOCK), c->side, nblk, g1_g2_h0_195, h_49, pk_97, d.p49, d.p97);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(grid_for(npub1)), dim3(BLOCK), c->side, npub1, d.p49, d.p96, d.st1, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, d.p97, d.p192, d.st2, 0);
    LAUNCH(c, bbs_wire_prep_kernel, n, n, msg_len, nblk, sig_145, msgs, d.a49, d.x, d.r, d.m, d.ss);
    LAUNCH(c, g1_decompress_kernel, n, n, d.a49, d.A, d.sa, 0);
    if ((rc = join_side(c))) return rc;
    if ((rc = c12381_bbs_plus_verify_batch_dev(c, n, nblk, d.p96, d.p192, d.p96 + 96, d.p96 + 192, d.p192 + 192, d.A, d.x, d.r, d.m, ok))) return rc;
    LAUNCH(c, bbs_wire_finish_kernel, n, n, npub1, d.ss, d.sa, d.st1, d.st2, ok, c->d_flag);
    return 0;
}
int c12381_bbs_plus_verify_wire_batch(c12381_ctx* c, size_t n, size_t nh, size_t msg_len, const uint8_t* g1_g2_h0_195, const uint8_t* h_49,
                                      const uint8_t* pk_97, const uint8_t* sig_145, const uint8_t* msgs, uint8_t* ok) {
    int rc = bind(c) ?: bbs_wire_args(nh, msg_len, g1_g2_h0_195, h_49, pk_97, sig_145, msgs, ok);
    if (rc || n == 0) return rc;
    return host_form(c, {{g1_g2_h0_195, 195}, {h_49, 49 * nh}, {pk_97, 97}, {sig_145, 145 * n}, {msgs, msg_len * n}}, {{ok, n}},
                     [&](const staging& s) { return c12381_bbs_plus_verify_wire_batch_dev(c, n, nh, msg_len, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.out[0]); });
}

// ---------------------------------------------------------------- BBS+ aggregate verification (optional)
// ONE verdict for the whole batch by a random linear combination: with caller-drawn rho_j,
//   prod_j [ e(A_j, w) e(x_j A_j - B_j, g2) ]^rho_j
//     = e( sum_j rho_j A_j, w ) * e( sum_j (rho_j x_j) A_j - (sum_j rho_j) g1 - (sum_j rho_j r_j) h0 - sum_i (sum_j rho_j m_ij) h_i, g2 )
// — the per-signature point arithmetic collapses into inner products mod r, two bucket products over the A_j and one
// product of two pairings.  all_ok = 1 iff g2, w are elements of G2 and the combined product is 1; every signature the
// per-signature entry accepts contributes a factor 1 (cofactor components of any argument pair to 1 against G2), so
// a batch of valid signatures always yields 1, and a batch containing an invalid one yields 1 with probability at most
// 2^-k over k-bit uniform rho_j.  all_ok = 0 settles nothing: the caller then runs the per-signature entry.
// The reference has no such mode (it verifies one signature at a time, bbs+.cpp:57-73); the booleans of
// c12381_bbs_plus_verify_batch stay the parity surface.
static int bbs_aggregate_args(size_t n, size_t nmsg, const void* g1_96, const void* g2_192, const void* h0_96, const void* h_96, const void* w_192,
                              const void* A_96, const void* x_32, const void* r_32, const void* m_32, const void* rho_32, const void* all_ok) {
    if (!g1_96 || !g2_192 || !h0_96 || !w_192 || !all_ok || (n && (!A_96 || !x_32 || !r_32 || !rho_32)) || (nmsg && (!h_96 || (n && !m_32)))) return C12381_E_ARG;
    return n + nmsg + 2 > MSM_MAX_TERMS ? C12381_E_ARG : 0;          // split the batch: one bucket product per call
}
int c12381_bbs_plus_verify_aggregate_dev(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192, const uint8_t* h0_96,
                                         const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96, const uint8_t* x_32, const uint8_t* r_32,
                                         const uint8_t* m_32, const uint8_t* rho_32, uint8_t* all_ok) {
    int rc = bind(c) ?: bbs_aggregate_args(n, nmsg, g1_96, g2_192, h0_96, h_96, w_192, A_96, x_32, r_32, m_32, rho_32, all_ok);
    if (rc) return rc;
    const size_t terms = n + nmsg + 2;
    if (n == 0) { HIPCK(c, hipMemsetAsync(all_ok, 1, 1, c->stream)); return 0; }
    HIPCK(c, hipMemsetAsync(all_ok, 0, 1, c->stream));
    cached lines;
    if ((rc = bbs_lines_tables(c, w_192, g2_192, lines))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_BBS_B, bbs_aggregate_layout(nullptr, terms).bytes))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_BBS_Q, 32 * terms))) return rc;
    const bbs_aggregate_slab d = bbs_aggregate_layout(c->ws[c12381_ctx::WS_BBS_B], terms);
    uint8_t* pts = d.pts;                                        // A_1 .. A_n, g1, h0, h_1 .. h_nmsg
    uint8_t* sc = (uint8_t*)c->ws[c12381_ctx::WS_BBS_Q];         // rho_j x_j | -sum rho_j, -sum rho_j r_j, -sum_j rho_j m_ij
    uint8_t *tail = sc + 32 * n, *p1 = d.p12, *p2 = p1 + 96;
    LAUNCH(c, zp_op_kernel, n, 0, n, rho_32, x_32, sc);
    {   // tail[y] = sum_j rho_j * (1 | r_j | m_{y-2,j}): all nmsg + 2 inner products as columns of the same fold stages
        const size_t cols = nmsg + 2;
        const uint8_t* cur_a = rho_32;
        size_t cur_n = n, col_stride = 0;
        int slot = c12381_ctx::WS_RED0, first = 1;
        for (;;) {
            const size_t T = (cur_n + 63) / 64;
            uint8_t* dst = tail;
            if (T > 1) {
                if ((rc = ensure(c, slot, round_up(32 * T * cols, 256)))) return rc;
                dst = (uint8_t*)c->ws[slot];
            }
            LAUNCH_ON(c, zp_fold_cols_kernel, dim3(grid_for(T), (unsigned)cols), dim3(BLOCK), c->stream, cur_n, cur_a, col_stride, r_32, m_32, first, T, dst);
            if (T == 1) break;
            cur_a = dst; col_stride = 32 * T; cur_n = T; first = 0;
            slot = other_red(slot);
        }
    }
    LAUNCH(c, zp_op_kernel, nmsg + 2, 3, nmsg + 2, (const uint8_t*)tail, (const uint8_t*)nullptr, tail);
    HIPCK(c, hipMemcpyAsync(pts, A_96, 96 * n, hipMemcpyDeviceToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(pts + 96 * n, g1_96, 96, hipMemcpyDeviceToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(pts + 96 * (n + 1), h0_96, 96, hipMemcpyDeviceToDevice, c->stream));
    if (nmsg) HIPCK(c, hipMemcpyAsync(pts + 96 * (n + 2), h_96, 96 * nmsg, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = c12381_g1_msm_dev(c, n, A_96, rho_32, p1, 96))) return rc;
    if ((rc = c12381_g1_msm_dev(c, terms, pts, sc, p2, 96))) return rc;
    return launch_prod_fixed(c, 1, p1, p2, lines, all_ok, lines.gate);
}
int c12381_bbs_plus_verify_aggregate(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192, const uint8_t* h0_96,
                                     const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96, const uint8_t* x_32, const uint8_t* r_32,
                                     const uint8_t* m_32, const uint8_t* rho_32, int* all_ok) {
    int rc = bind(c) ?: bbs_aggregate_args(n, nmsg, g1_96, g2_192, h0_96, h_96, w_192, A_96, x_32, r_32, m_32, rho_32, all_ok);
    if (rc) return rc;
    *all_ok = 0;
    if (n == 0) { *all_ok = 1; return 0; }
    uint8_t verdict = 0;
    rc = host_form(c, {{g1_96, 96}, {g2_192, 192}, {h0_96, 96}, {h_96, 96 * nmsg}, {w_192, 192}, {A_96, 96 * n}, {x_32, 32 * n}, {r_32, 32 * n},
                       {m_32, 32 * n * nmsg}, {rho_32, 32 * n}}, {{&verdict, 1}}, [&](const staging& s) {      // synchronises the stream
        return c12381_bbs_plus_verify_aggregate_dev(c, n, nmsg, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.in[7], s.in[8], s.in[9], s.out[0]);
    });
    *all_ok = (rc == 0 && verdict == 1) ? 1 : 0;
    return rc;
}

// BBS+ signing for a batch (bbs+.cpp:38-55): A_j = (g1 * h0^r_j * prod_i h_i^m_ij)^(1/(gamma + x_j)).  x_j, r_j are the
// caller's random scalars (the reference draws them inside sign()); inverse(0) = 0 gives the point at infinity, as there.
static int bbs_sign_args(size_t nmsg, const void* g1_96, const void* h0_96, const void* h_96, const void* gamma_32, const void* x_32, const void* r_32,
                         const void* m_32, const void* A_out96) {
    return (!g1_96 || !h0_96 || !gamma_32 || !x_32 || !r_32 || !A_out96 || (nmsg && (!h_96 || !m_32))) ? C12381_E_ARG : 0;
}
int c12381_bbs_plus_sign_batch_dev(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* h0_96, const uint8_t* h_96,
                                   const uint8_t* gamma_32, const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, uint8_t* A_out96) {
    int rc = bind(c) ?: bbs_sign_args(nmsg, g1_96, h0_96, h_96, gamma_32, x_32, r_32, m_32, A_out96);
    if (rc || n == 0) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_BBS_B, 192 * n))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_BBS_Q, 192 * n))) return rc;
    uint8_t* d_b = (uint8_t*)c->ws[c12381_ctx::WS_BBS_B];         // B_j affine
    uint8_t* d_e = (uint8_t*)c->ws[c12381_ctx::WS_BBS_Q];         // 1 / (gamma + x_j)
    int32_t* red; size_t rstride, stride;
    if ((rc = bbs_message_points(c, n, nmsg, g1_96, h0_96, h_96, r_32, m_32, fixed_base_enabled(), red, rstride, stride))) return rc;
    if ((rc = g1_finish(c, n, red, rstride, d_b, 96))) return rc;
    if ((rc = zp_batch_inverse(c, n, x_32, gamma_32, d_e))) return rc;
    return c12381_g1_mul_batch_dev(c, n, d_b, d_e, A_out96, 96);
}
int c12381_bbs_plus_sign_batch(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* h0_96, const uint8_t* h_96,
                               const uint8_t* gamma_32, const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, uint8_t* A_out96) {
    int rc = bind(c) ?: bbs_sign_args(nmsg, g1_96, h0_96, h_96, gamma_32, x_32, r_32, m_32, A_out96);
    if (rc || n == 0) return rc;
    return host_form(c, {{g1_96, 96}, {h0_96, 96}, {h_96, 96 * nmsg}, {gamma_32, 32}, {x_32, 32 * n}, {r_32, 32 * n}, {m_32, 32 * n * nmsg}}, {{A_out96, 96 * n}},
                     [&](const staging& s) { return c12381_bbs_plus_sign_batch_dev(c, n, nmsg, s.in[0], s.in[1], s.in[2], s.in[3], s.in[4], s.in[5], s.in[6], s.out[0]); });
}
