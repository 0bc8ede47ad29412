// Slab layouts of the protocol entries: which fields an entry keeps in its workspace and how many bytes each holds.  Nothing of HIP in here,
// so that a CPU program can carve every layout and write it end to end (tests/host_sim/host_layouts.cpp).
// An entry calls its layout function twice: with a null base for the size it hands to ensure(), then with the workspace.  The byte counts are
// the ones the entry's kernels write; a field a kernel indexes as one array (the public points g1, h0, h_1 ...; both halves of s96) is one field.
#pragma once
#include <cstddef>
#include <cstdint>

namespace c12381_host __attribute__((visibility("hidden"))) {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Fields taken in order from `base + start`, each rounded to 256 bytes; `bytes` is the size so far (base = nullptr: sizing only)
struct carver {
    uint8_t* base; size_t bytes;
    explicit carver(void* base_, size_t start = 0) : base((uint8_t*)base_), bytes(start) {}
    uint8_t* take(size_t n) { uint8_t* p = base ? base + bytes : nullptr; bytes = round_up(bytes + n, 256); return p; }
};

// ---------------------------------------------------------------- BBS+ (WS_BBS_WIRE; the aggregate: WS_BBS_B)
// wire: the public points as they arrive (p49: g1, h0, h_1 ..; p97: g2, w), decoded (p96, p192) with their statuses, then per signature
// A as it arrives and decoded, x, r, the nblk message scalars (message-major), the parse status and the decoding status of A
struct bbs_wire_slab { uint8_t *p49, *p97, *p96, *p192, *st1, *st2, *a49, *A, *x, *r, *m, *ss, *sa; size_t bytes; };
inline bbs_wire_slab bbs_wire_layout(void* base, size_t n, size_t nblk) {
    const size_t npub1 = 2 + nblk;
    carver f(base);
    bbs_wire_slab s;
    s.p49 = f.take(49 * npub1); s.p97 = f.take(2 * 97); s.p96 = f.take(96 * npub1); s.p192 = f.take(2 * 192); s.st1 = f.take(npub1); s.st2 = f.take(2);
    s.a49 = f.take(49 * n); s.A = f.take(96 * n); s.x = f.take(32 * n); s.r = f.take(32 * n); s.m = f.take(32 * n * nblk); s.ss = f.take(n); s.sa = f.take(n);
    s.bytes = f.bytes;
    return s;
}
// aggregate: the terms of the second bucket product A_1 .. A_n, g1, h0, h_1 .. h_nmsg, then its two results P1, P2
struct bbs_aggregate_slab { uint8_t *pts, *p12; size_t bytes; };
inline bbs_aggregate_slab bbs_aggregate_layout(void* base, size_t terms) {
    carver f(base);
    bbs_aggregate_slab s;
    s.pts = f.take(96 * terms); s.p12 = f.take(2 * 96);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- PS (WS_PS: verify, sign, randomize and the aggregate; none calls another)
// verify: npub = 2 + units public points g2, X2, Y2_0 .. decoded and their statuses; per signature both 49-byte records (σ1 column, σ2 column),
// both decoded, `units` message scalars, both decoding statuses
struct ps_wire_slab { uint8_t *p192, *stp, *s49, *s96, *m, *st; size_t bytes; };
inline ps_wire_slab ps_wire_layout(void* base, size_t n, size_t units) {
    const size_t npub = 2 + units;
    carver f(base);
    ps_wire_slab s;
    s.p192 = f.take(192 * npub); s.stp = f.take(npub); s.s49 = f.take(98 * n); s.s96 = f.take(192 * n); s.m = f.take(32 * n * units); s.st = f.take(2 * n);
    s.bytes = f.bytes;
    return s;
}
// sign: the generator record, the key's status byte, the interleaved scalars t_j, t_j e_j
struct ps_sign_slab { uint8_t *gen, *key, *sc; size_t bytes; };
inline ps_sign_slab ps_sign_layout(void* base, size_t n) {
    carver f(base);
    ps_sign_slab s;
    s.gen = f.take(96); s.key = f.take(1); s.sc = f.take(64 * n);
    s.bytes = f.bytes;
    return s;
}
// randomize: the 2 n decoded records, r_j twice per signature, the 2 n decoding statuses
struct ps_randomize_slab { uint8_t *s96, *sc, *st; size_t bytes; };
inline ps_randomize_slab ps_randomize_layout(void* base, size_t n) {
    carver f(base);
    ps_randomize_slab s;
    s.s96 = f.take(192 * n); s.sc = f.take(64 * n); s.st = f.take(2 * n);
    s.bytes = f.bytes;
    return s;
}
// aggregate: the k = nmsg + 2 sums, and one scalar column rewritten per message (stream order)
struct ps_aggregate_slab { uint8_t *sum, *col; size_t bytes; };
inline ps_aggregate_slab ps_aggregate_layout(void* base, size_t n, size_t k) {
    carver f(base);
    ps_aggregate_slab s;
    s.sum = f.take(96 * k); s.col = f.take(32 * n);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- bbs04 (WS_BBS04): every slab starts behind the public block
constexpr size_t BBS04_PUB_BYTES = 2048;
// the public block: gpk's points as they arrive, decoded, and the six status bytes of the decoding
struct bbs04_public {
    uint8_t *wire_g1, *wire_g2;          // 4 x 49 B (g1, h, u, v), 2 x 97 B (g2, w)
    uint8_t *g1, *h, *u, *v;             // 96 B each, contiguous from g1
    uint8_t *g2_w;                       // g2, w: 192 B each
    uint8_t* st;                         // 4 G1 statuses, 2 G2 statuses
    explicit bbs04_public(uint8_t* d)
        : wire_g1(d), wire_g2(d + 256), g1(d + 512), h(g1 + 96), u(g1 + 192), v(g1 + 288), g2_w(d + 1024), st(d + 1536) {}
};
// verify and open, per signature of a chunk: T records, 13 scalar columns, statuses, R and P points, GT value, transcript
struct bbs04_slab { uint8_t *t49, *t96, *sc, *c32, *st, *st_t, *r49, *p96, *gt, *tr; size_t bytes; };
inline bbs04_slab bbs04_layout(void* base, size_t m, size_t msg_len) {
    carver f(base, BBS04_PUB_BYTES);
    bbs04_slab s;
    s.t49 = f.take(3 * 49 * m); s.t96 = f.take(6 * 96 * m); s.sc = f.take(13 * 32 * m); s.c32 = f.take(32 * m); s.st = f.take(m); s.st_t = f.take(3 * m);
    s.r49 = f.take(4 * 49 * m); s.p96 = f.take(2 * 96 * m); s.gt = f.take(576 * m); s.tr = f.take((msg_len + 919) * m);
    s.bytes = f.bytes;
    return s;
}
struct bbs04_sign_slab { uint8_t *a49, *a96, *st_a, *sc, *t49, *t96, *r49, *p96, *gt, *tr; size_t bytes; };
inline bbs04_sign_slab bbs04_sign_layout(void* base, size_t m, size_t msg_len) {
    carver f(base, BBS04_PUB_BYTES);
    bbs04_sign_slab s;
    s.a49 = f.take(49 * m); s.a96 = f.take(96 * m); s.st_a = f.take(m); s.sc = f.take(12 * 32 * m); s.t49 = f.take(3 * 49 * m); s.t96 = f.take(3 * 96 * m);
    s.r49 = f.take(4 * 49 * m); s.p96 = f.take(2 * 96 * m); s.gt = f.take(576 * m); s.tr = f.take((msg_len + 919) * m);
    s.bytes = f.bytes;
    return s;
}
// issue: 32 + 49 bytes per key of a chunk
struct bbs04_issue_slab { uint8_t *inv, *a49; size_t bytes; };
inline bbs04_issue_slab bbs04_issue_layout(void* base, size_t m) {
    carver f(base, BBS04_PUB_BYTES);
    bbs04_issue_slab s;
    s.inv = f.take(32 * m); s.a49 = f.take(49 * m);
    s.bytes = f.bytes;
    return s;
}

}  // namespace c12381_host
