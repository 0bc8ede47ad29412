// The SHA3-512 entry and the bbs04 group-signature entries of the C ABI (include/c12381_hip.h): verify, open, sign, issue.  Kernels: k_bbs04.hip;
// the shared host pieces: host.hpp.
#include "host.hpp"

using namespace c12381;
using namespace c12381_host;

// ---------------------------------------------------------------- SHA3-512 (k_bbs04.hip, sha3.hpp)
// out[i] = SHA3-512 of the i-th len-byte message: hash_state's SHA3_init(64) / SHA3_process / SHA3_hash (set.hpp:317-392), one lane per message
static int sha3_args(size_t len, const void* msgs, const void* out) { return (!out || (len && !msgs)) ? C12381_E_ARG : 0; }
static int launch_sha3(c12381_ctx* c, size_t n, size_t len, const uint8_t* msgs, uint8_t* out) {
    LAUNCH(c, sha3_512_kernel, n, n, len, msgs, out);
    return 0;
}
int c12381_sha3_512_batch_dev(c12381_ctx* c, size_t n, size_t len, const uint8_t* msgs, uint8_t* out64) {
    int rc = bind(c) ?: sha3_args(len, msgs, out64);
    if (rc || n == 0) return rc;
    return launch_sha3(c, n, len, msgs, out64);
}
int c12381_sha3_512_batch(c12381_ctx* c, size_t n, size_t len, const uint8_t* msgs, uint8_t* out64) {
    int rc = bind(c) ?: sha3_args(len, msgs, out64);
    if (rc || n == 0) return rc;
    return host_form(c, {{len ? msgs : nullptr, len * n}}, {{out64, 64 * n}}, [&](const staging& s) { return launch_sha3(c, n, len, s.in[0], s.out[0]); });
}

// ---------------------------------------------------------------- bbs04 group signatures (examples/bbs04/src/bbs.cpp)
// verify (:61-78), per signature: decode T1..T3 and range-check the six Zp fields (bbs04_prep_kernel), thirteen scalar multiplications by
// the G1 kernels — six variable-base in one launch, seven against u, v, h, g1 through their fixed-base tables (generic kernel when a base
// is not a subgroup point) — complete additions (bbs04_combine_kernel), affine conversion, R3 by the k = 2 fixed-G2 product, the
// transcript, SHA3-512 mod r against c (bbs04_check_kernel).  Batches run in chunks of BBS04_CHUNK signatures.  WS_BBS04 holds
// BBS04_PUB_BYTES of decoded public points and, per signature of a chunk, bbs04_sig_bytes(msg_len) bytes (T records, 13 scalar columns,
// statuses, R and P points, GT value, transcript); the shared scalar-multiplication workspaces hold 13 projective points per signature.
constexpr size_t BBS04_CHUNK = (size_t)1 << 18;
// The public block and the three slabs behind it: host_layouts.hpp (bbs04_public, bbs04_layout, bbs04_sign_layout, bbs04_issue_layout).
// the public points on the side stream (two short square-root chains beside the per-signature work on the context's stream); the caller
// joins the side stream before its first use of them
static int bbs04_pub(c12381_ctx* c, const uint8_t* gpk, const bbs04_public& pub) {
    int rc;
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, bbs04_pub_kernel, dim3(grid_for(4 * 49 + 2 * 97)), dim3(BLOCK), c->side, gpk, pub.wire_g1, pub.wire_g2);
    LAUNCH_ON(c, g1_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)4, pub.wire_g1, pub.g1, pub.st, 0);
    LAUNCH_ON(c, g2_decompress_kernel, dim3(1), dim3(BLOCK), c->side, (size_t)2, pub.wire_g2, pub.g2_w, pub.st + 4, 0);
    return 0;
}
static int bbs04_verify_args(size_t msg_len, const void* gpk, const void* sig, const void* msgs, const void* ok) {
    return (!gpk || !sig || !ok || (msg_len && !msgs)) ? C12381_E_ARG : 0;
}
int c12381_bbs04_verify_batch_dev(c12381_ctx* c, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* sig_435, const uint8_t* msgs,
                                  uint8_t* ok) {
    int rc = bind(c) ?: bbs04_verify_args(msg_len, gpk_390, sig_435, msgs, ok);
    if (rc || n == 0) return rc;
    const size_t ch = n < BBS04_CHUNK ? n : BBS04_CHUNK, L = msg_len + 919;
    if ((rc = ensure(c, c12381_ctx::WS_BBS04, bbs04_layout(nullptr, ch, msg_len).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_BBS04];
    const bbs04_public pub(d);
    if ((rc = bbs04_pub(c, gpk_390, pub))) return rc;
    const bool fb = fixed_base_enabled();
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const bbs04_slab s = bbs04_layout(d, m, msg_len);
        LAUNCH(c, bbs04_prep_kernel, m, m, sig_435 + 435 * off, s.t49, s.sc, s.c32, s.st);
        LAUNCH(c, g1_decompress_kernel, 3 * m, 3 * m, s.t49, s.t96, s.st_t, 0);
        // variable bases T1, T2, T3, T1, T2, T3 against scalar columns 0-5: one launch of 6 m lanes
        HIPCK(c, hipMemcpyAsync(s.t96 + 3 * 96 * m, s.t96, 3 * 96 * m, hipMemcpyDeviceToDevice, c->stream));
        if (off == 0 && (rc = join_side(c))) return rc;
        proj_slab w;
        if ((rc = proj_ws(c, 13 * m, w))) return rc;
        if ((rc = g1_mul_to_proj(c, 6 * m, s.t96, s.sc, w.stride))) return rc;
        // fixed bases: columns 6-12 (u, v, u, v, h, g1, h); table slots u -> 0, v -> 1, h -> 2, g1 -> 3
        const uint8_t* tab[4] = {pub.u, pub.v, pub.h, pub.g1};
        const int slot[7] = {0, 1, 0, 1, 2, 3, 2};
        if (fb)
            for (int t = 0; t < 4; ++t)
                if ((rc = g1_fixed_table(c, t, tab[t]))) return rc;
        for (size_t col = 6; col < 13; ++col)
            if ((rc = g1_fixed_column(c, m, tab[slot[col - 6]], slot[col - 6], s.sc + 32 * col * m, w.stride, col * m, fb))) return rc;
        LAUNCH(c, bbs04_combine_kernel, m, m, w.p, w.stride);
        if ((rc = g1_finish(c, 4 * m, w.p, w.stride, s.r49, 49))) return rc;
        if ((rc = g1_finish(c, 2 * m, w.p + 4 * m, w.stride, s.p96, 96))) return rc;
        if ((rc = c12381_pair_product_fixed_g2_batch_dev(c, m, 2, s.p96, pub.g2_w, s.gt, 0u))) return rc;
        const size_t bytes = m * L;
        LAUNCH(c, bbs04_transcript_kernel, bytes, m, msg_len, msg_len ? msgs + msg_len * off : msgs, s.t49, s.t96, s.r49, s.gt, s.tr);
        LAUNCH(c, bbs04_check_kernel, m, m, L, s.tr, s.c32, s.st, s.st_t, pub.st, ok + off, c->d_flag);
    }
    return 0;
}
int c12381_bbs04_verify_batch(c12381_ctx* c, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* sig_435, const uint8_t* msgs, uint8_t* ok) {
    int rc = bind(c) ?: bbs04_verify_args(msg_len, gpk_390, sig_435, msgs, ok);
    if (rc || n == 0) return rc;
    return host_form(c, {{gpk_390, 390}, {sig_435, 435 * n}, {msg_len ? msgs : nullptr, msg_len * n}}, {{ok, n}},
                     [&](const staging& s) { return c12381_bbs04_verify_batch_dev(c, n, msg_len, s.in[0], s.in[1], s.in[2], s.out[0]); });
}
// open (:80-86): a = T3 - (T1^xi1 + T2^xi2), `^` = PAIR_G1mul by the generic G1 kernel (both columns in one launch of 2 m lanes)
static int bbs04_open_args(const void* gmsk, const void* sig, const void* out, const void* status) { return (!gmsk || !sig || !out || !status) ? C12381_E_ARG : 0; }
int c12381_bbs04_open_batch_dev(c12381_ctx* c, size_t n, const uint8_t* gmsk_96, const uint8_t* sig_435, uint8_t* out49, uint8_t* status) {
    int rc = bind(c) ?: bbs04_open_args(gmsk_96, sig_435, out49, status);
    if (rc || n == 0) return rc;
    const size_t ch = n < BBS04_CHUNK ? n : BBS04_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_BBS04, bbs04_layout(nullptr, ch, 0).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_BBS04];
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const bbs04_slab s = bbs04_layout(d, m, 0);
        LAUNCH(c, bbs04_open_prep_kernel, m, m, gmsk_96, sig_435 + 435 * off, s.t49, s.sc, s.st, c->d_flag);
        LAUNCH(c, g1_decompress_kernel, 3 * m, 3 * m, s.t49, s.t96, s.st_t, 0);
        proj_slab w;
        if ((rc = proj_ws(c, 2 * m, w))) return rc;
        if ((rc = g1_mul_to_proj(c, 2 * m, s.t96, s.sc, w.stride))) return rc;
        LAUNCH(c, bbs04_open_combine_kernel, m, m, w.p, w.stride, (const uint8_t*)s.t96 + 2 * 96 * m);
        if ((rc = g1_finish(c, m, w.p, w.stride, out49 + 49 * off, 49))) return rc;
        LAUNCH(c, bbs04_open_status_kernel, m, m, s.st, s.st_t, status + off);
    }
    return 0;
}
int c12381_bbs04_open_batch(c12381_ctx* c, size_t n, const uint8_t* gmsk_96, const uint8_t* sig_435, uint8_t* out49, uint8_t* status) {
    int rc = bind(c) ?: bbs04_open_args(gmsk_96, sig_435, out49, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{gmsk_96, 96}, {sig_435, 435 * n}}, {{out49, 49 * n}, {status, n}},
                     [&](const staging& s) { return c12381_bbs04_open_batch_dev(c, n, s.in[0], s.in[1], s.out[0], s.out[1]); });
}

// sign (:32-59), per signature: decode A, reduce the seven random scalars and write the scalar columns (bbs04_sign_prep_kernel,
// bbs04_sign.hpp).  Phase 1: u^alpha, v^beta, h^(alpha + beta) through the fixed-base tables (generic kernel when a base is not a subgroup
// point), T3 = A + h^(alpha + beta), T1..T3 as 49-byte records (wire, transcript) and 96-byte records (bases of phase 2).  Phase 2: T1^rx,
// T2^rx, T3^rx in one variable-base launch of 3 m lanes, six fixed-base columns, the additions (bbs04_sign_combine_kernel), R3 by the
// k = 2 fixed-G2 product, verify's transcript kernel, then c and the responses (bbs04_sign_finish_kernel).  Table slots as in verify
// (u -> 0, v -> 1, h -> 2, g1 -> 3), so signing and verifying under one gpk share the tables.  WS_BBS04 holds, behind BBS04_PUB_BYTES and
// per signature of a chunk, bbs04_sign_layout's 2848 + msg_len bytes; the scalar-multiplication workspace holds 9 projective points.
static int bbs04_sign_args(size_t msg_len, const void* gpk, const void* gsk, const void* msgs, const void* rnd, const void* sig, const void* status) {
    return (!gpk || !gsk || !rnd || !sig || !status || (msg_len && !msgs)) ? C12381_E_ARG : 0;
}
int c12381_bbs04_sign_batch_dev(c12381_ctx* c, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* gsk_97, const uint8_t* msgs,
                                const uint8_t* rnd_224, uint8_t* sig_435, uint8_t* status) {
    int rc = bind(c) ?: bbs04_sign_args(msg_len, gpk_390, gsk_97, msgs, rnd_224, sig_435, status);
    if (rc || n == 0) return rc;
    const size_t ch = n < BBS04_CHUNK ? n : BBS04_CHUNK, L = msg_len + 919;
    if ((rc = ensure(c, c12381_ctx::WS_BBS04, bbs04_sign_layout(nullptr, ch, msg_len).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_BBS04];
    const bbs04_public pub(d);
    if ((rc = bbs04_pub(c, gpk_390, pub))) return rc;
    const bool fb = fixed_base_enabled();
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        const bbs04_sign_slab s = bbs04_sign_layout(d, m, msg_len);
        const uint8_t *gsk = gsk_97 + 97 * off, *rnd = rnd_224 + 224 * off;
        LAUNCH(c, bbs04_sign_prep_kernel, m, m, gsk, rnd, s.a49, s.sc);
        LAUNCH(c, g1_decompress_kernel, m, m, s.a49, s.a96, s.st_a, 0);
        if (off == 0 && (rc = join_side(c))) return rc;
        proj_slab w;
        if ((rc = proj_ws(c, 9 * m, w))) return rc;
        const uint8_t* tab[3] = {pub.u, pub.v, pub.h};
        if (fb)
            for (int t = 0; t < 3; ++t)
                if ((rc = g1_fixed_table(c, t, tab[t]))) return rc;
        // phase 1: scalar columns 0-2 -> T1, T2, T3
        for (size_t k = 0; k < 3; ++k)
            if ((rc = g1_fixed_column(c, m, tab[k], (int)k, s.sc + 32 * k * m, w.stride, k * m, fb))) return rc;
        LAUNCH(c, bbs04_sign_t3_kernel, m, m, w.p, w.stride, (const uint8_t*)s.a96);
        if ((rc = g1_finish(c, 3 * m, w.p, w.stride, s.t49, 49))) return rc;
        if ((rc = g1_finish(c, 3 * m, w.p, w.stride, s.t96, 96))) return rc;
        // phase 2: T1, T2, T3 against scalar columns 3-5 (r_x) in one launch of 3 m lanes, then columns 6-11 (u, v, u, v, h, h)
        if ((rc = g1_mul_to_proj(c, 3 * m, s.t96, s.sc + 32 * 3 * m, w.stride))) return rc;
        const int slot2[6] = {0, 1, 0, 1, 2, 2};
        for (size_t k = 0; k < 6; ++k)
            if ((rc = g1_fixed_column(c, m, tab[slot2[k]], slot2[k], s.sc + 32 * (6 + k) * m, w.stride, (3 + k) * m, fb))) return rc;
        LAUNCH(c, bbs04_sign_combine_kernel, m, m, w.p, w.stride);
        if ((rc = g1_finish(c, 4 * m, w.p, w.stride, s.r49, 49))) return rc;
        if ((rc = g1_finish(c, 2 * m, w.p + 4 * m, w.stride, s.p96, 96))) return rc;
        if ((rc = c12381_pair_product_fixed_g2_batch_dev(c, m, 2, s.p96, pub.g2_w, s.gt, 0u))) return rc;
        LAUNCH(c, bbs04_transcript_kernel, m * L, m, msg_len, msg_len ? msgs + msg_len * off : msgs, s.t49, s.t96, s.r49, s.gt, s.tr);
        LAUNCH(c, bbs04_sign_finish_kernel, m, m, L, s.tr, gsk, rnd, s.t49, s.st_a, pub.st, sig_435 + 435 * off, status + off, c->d_flag);
    }
    return 0;
}
int c12381_bbs04_sign_batch(c12381_ctx* c, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* gsk_97, const uint8_t* msgs,
                            const uint8_t* rnd_224, uint8_t* sig_435, uint8_t* status) {
    int rc = bind(c) ?: bbs04_sign_args(msg_len, gpk_390, gsk_97, msgs, rnd_224, sig_435, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{gpk_390, 390}, {gsk_97, 97 * n}, {msg_len ? msgs : nullptr, msg_len * n}, {rnd_224, 224 * n}}, {{sig_435, 435 * n}, {status, n}},
                     [&](const staging& s) { return c12381_bbs04_sign_batch_dev(c, n, msg_len, s.in[0], s.in[1], s.in[2], s.in[3], s.out[0], s.out[1]); });
}
// key_gen's issuance (:17-23): gsk_i = serialize(g1^inverse(gamma + x_i), x_i) — the simultaneous inversion of c12381_zp_op_batch, g1's
// fixed-base table (slot 3, as in verify; the generic kernel when g1 is not a subgroup point), 49-byte records, bbs04_issue_pack_kernel.
// WS_BBS04: the public block, then 32 + 49 bytes per key of a chunk.
static int bbs04_issue_args(const void* gpk, const void* gamma, const void* x, const void* gsk) { return (!gpk || !gamma || !x || !gsk) ? C12381_E_ARG : 0; }
int c12381_bbs04_issue_batch_dev(c12381_ctx* c, size_t n, const uint8_t* gpk_390, const uint8_t* gamma_32, const uint8_t* x_32, uint8_t* gsk_97) {
    int rc = bind(c) ?: bbs04_issue_args(gpk_390, gamma_32, x_32, gsk_97);
    if (rc || n == 0) return rc;
    const size_t ch = n < BBS04_CHUNK ? n : BBS04_CHUNK;
    if ((rc = ensure(c, c12381_ctx::WS_BBS04, bbs04_issue_layout(nullptr, ch).bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_BBS04];
    const bbs04_issue_slab s = bbs04_issue_layout(d, ch);
    const bbs04_public pub(d);
    if ((rc = bbs04_pub(c, gpk_390, pub))) return rc;
    const bool fb = fixed_base_enabled();
    for (size_t off = 0; off < n; off += ch) {
        const size_t m = n - off < ch ? n - off : ch;
        if ((rc = zp_batch_inverse(c, m, x_32 + 32 * off, gamma_32, s.inv))) return rc;
        if (off == 0 && (rc = join_side(c))) return rc;
        proj_slab w;
        if ((rc = proj_ws(c, m, w))) return rc;
        if (fb && (rc = g1_fixed_table(c, 3, pub.g1))) return rc;
        if ((rc = g1_fixed_column(c, m, pub.g1, 3, s.inv, w.stride, 0, fb))) return rc;
        if ((rc = g1_finish(c, m, w.p, w.stride, s.a49, 49))) return rc;
        LAUNCH(c, bbs04_issue_pack_kernel, m, m, s.a49, x_32 + 32 * off, pub.st, gsk_97 + 97 * off, c->d_flag);
    }
    return 0;
}
int c12381_bbs04_issue_batch(c12381_ctx* c, size_t n, const uint8_t* gpk_390, const uint8_t* gamma_32, const uint8_t* x_32, uint8_t* gsk_97) {
    int rc = bind(c) ?: bbs04_issue_args(gpk_390, gamma_32, x_32, gsk_97);
    if (rc || n == 0) return rc;
    return host_form(c, {{gpk_390, 390}, {gamma_32, 32}, {x_32, 32 * n}}, {{gsk_97, 97 * n}},
                     [&](const staging& s) { return c12381_bbs04_issue_batch_dev(c, n, s.in[0], s.in[1], s.in[2], s.out[0]); });
}
