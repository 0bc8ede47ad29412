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

// ---------------------------------------------------------------- AC-bbs (WS_AC_BBS): both slabs start behind the public block
constexpr size_t AC_BBS_PUB_BYTES = 8192;
// the public block: pk.Y gathered into base order (the disclosed attributes' Y in the caller's order, then the hidden ones ascending) as it
// arrives and decoded, g and tilde_g, tilde_X decoded (straight from pk.fixed_part), and the 3 + nattr status bytes: g, tilde_g, tilde_X, Y ..
struct ac_bbs_public {
    uint8_t *y49, *g96, *y96, *g2, *st;  // 32 x 49 B; 96 B; 32 x 96 B; 2 x 192 B; 3 + 32 B
    explicit ac_bbs_public(uint8_t* d) : y49(d), g96(d + 1792), y96(d + 2048), g2(d + 5120), st(d + 5632) {}
};
// verify, per presentation of a chunk: A_, B_, U as they arrive (columns) and decoded, their statuses, the re-encoded A_, B_, U, the terms K, A_, -B_
// of the k = 3 product and its scalars s, t, c, the nattr fixed-base columns (a_I .., u_J ..), the parse status, the transcript, the product R, the
// sum over Y_J, R + sum compressed, the pairing verdict: 1359 + 32 nattr + msg_len bytes
struct ac_bbs_verify_slab { uint8_t *p49, *p96, *st_p, *e49, *q96, *sc3, *sca, *st, *tr, *r96, *s96, *r49, *okp; size_t bytes; };
inline ac_bbs_verify_slab ac_bbs_verify_layout(void* base, size_t m, size_t nattr, size_t msg_len) {
    carver f(base, AC_BBS_PUB_BYTES);
    ac_bbs_verify_slab s;
    s.p49 = f.take(3 * 49 * m); s.p96 = f.take(3 * 96 * m); s.st_p = f.take(3 * m); s.e49 = f.take(3 * 49 * m); s.q96 = f.take(3 * 96 * m);
    s.sc3 = f.take(3 * 32 * m); s.sca = f.take(32 * nattr * m); s.st = f.take(m); s.tr = f.take((msg_len + 147) * m); s.r96 = f.take(96 * m);
    s.s96 = f.take(96 * m); s.r49 = f.take(49 * m); s.okp = f.take(m);
    s.bytes = f.bytes;
    return s;
}
// pres, per presentation of a chunk: A as it arrives and decoded, its status and the parse status, the nattr attribute columns in base order, the
// nJ columns delta_j, the scalars r, alpha, -w, beta (the columns of A^r and of the 2 m-lane k = 2 product), its points C, C_I, A_, A_, a sum
// over Y_J, the products B_, U, the encoded A_, B_, U, c, the transcript: 1273 + 32 (nattr + nJ) + msg_len bytes
struct ac_bbs_pres_slab { uint8_t *a49, *a96, *st_a, *st, *sca, *scd, *sc2, *q96, *t96, *o96, *e49, *c32, *tr; size_t bytes; };
inline ac_bbs_pres_slab ac_bbs_pres_layout(void* base, size_t m, size_t nattr, size_t nJ, size_t msg_len) {
    carver f(base, AC_BBS_PUB_BYTES);
    ac_bbs_pres_slab s;
    s.a49 = f.take(49 * m); s.a96 = f.take(96 * m); s.st_a = f.take(m); s.st = f.take(m); s.sca = f.take(32 * nattr * m); s.scd = f.take(32 * nJ * m);
    s.sc2 = f.take(4 * 32 * m); s.q96 = f.take(4 * 96 * m); s.t96 = f.take(96 * m); s.o96 = f.take(2 * 96 * m); s.e49 = f.take(3 * 49 * m);
    s.c32 = f.take(32 * m); s.tr = f.take((msg_len + 147) * m);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- AC-rbbs (WS_AC_RBBS): the verify and redact slabs start behind the public block
constexpr size_t AC_RBBS_PUB_BYTES = 18432;
// the public block.  verify: the used records of pk.Y and pk.tilde_Y (in the order of idx) as they arrive (y49, ty97) and decoded (y96, ty192);
// redact: all 2 nattr records of pk.Y decoded (y96) and the base list gathered from them (l96).  Both: g and tilde_g, tilde_X decoded straight
// from pk.fixed_part, and the status bytes g, tilde_g, tilde_X, then the Y (and, behind them, the tilde_Y) that the entry decodes
struct ac_rbbs_public {
    uint8_t *y49, *ty97, *g96, *y96, *l96, *g2, *ty192, *st;  // 32 x 49 B; 32 x 97 B; 96 B; 32 x 96 B; 32 x 96 B; 2 x 192 B; 32 x 192 B; 3 + 64 B
    explicit ac_rbbs_public(uint8_t* d)
        : y49(d), ty97(d + 1792), g96(d + 5120), y96(d + 5376), l96(d + 8448), g2(d + 11520), ty192(d + 12032), st(d + 18176) {}
};
// verify, per presentation of a chunk: A_, B_, U, C_J_, D_ as they arrive (columns) and decoded, their statuses, the re-encoded five, the terms K, A_,
// -B_ of the k = 3 product and its scalars s, t, c, the nI columns a_I and the nI columns q_I, the parse status, the transcript, C_J_ + B_, the
// product compressed, both pairing verdicts: 1752 + 64 nI + msg_len bytes
struct ac_rbbs_verify_slab { uint8_t *p49, *p96, *st_p, *e49, *q96, *sc3, *sca, *q32, *st, *tr, *s96, *r49, *ok1, *ok3; size_t bytes; };
inline ac_rbbs_verify_slab ac_rbbs_verify_layout(void* base, size_t m, size_t nI, size_t msg_len) {
    carver f(base, AC_RBBS_PUB_BYTES);
    ac_rbbs_verify_slab s;
    s.p49 = f.take(5 * 49 * m); s.p96 = f.take(5 * 96 * m); s.st_p = f.take(5 * m); s.e49 = f.take(5 * 49 * m); s.q96 = f.take(3 * 96 * m);
    s.sc3 = f.take(3 * 32 * m); s.sca = f.take(32 * nI * m); s.q32 = f.take(32 * nI * m); s.st = f.take(m); s.tr = f.take((msg_len + 245) * m);
    s.s96 = f.take(96 * m); s.r49 = f.take(49 * m); s.ok1 = f.take(m); s.ok3 = f.take(m);
    s.bytes = f.bytes;
    return s;
}
// pres (no key: the slab starts at the workspace), per presentation: C_I, A, B, C_J, D as they arrive and decoded, their statuses and the parse
// status, r four times, alpha and beta, the terms C_I, A_ of the k = 2 product, the points A_, B_, C_J_, D_, U and their encodings, c, the
// transcript: 2117 + msg_len bytes
struct ac_rbbs_pres_slab { uint8_t *p49, *p96, *st_p, *st, *scr, *sc2, *t96, *o96, *e49, *c32, *tr; size_t bytes; };
inline ac_rbbs_pres_slab ac_rbbs_pres_layout(void* base, size_t m, size_t msg_len) {
    carver f(base);
    ac_rbbs_pres_slab s;
    s.p49 = f.take(5 * 49 * m); s.p96 = f.take(5 * 96 * m); s.st_p = f.take(5 * m); s.st = f.take(m); s.scr = f.take(4 * 32 * m); s.sc2 = f.take(2 * 32 * m);
    s.t96 = f.take(2 * 96 * m); s.o96 = f.take(5 * 96 * m); s.e49 = f.take(5 * 49 * m); s.c32 = f.take(32 * m); s.tr = f.take((msg_len + 245) * m);
    s.bytes = f.bytes;
    return s;
}
// redact, per credential: A as it arrives and decoded, its status and the parse status, the nattr attribute columns, -w, the disclosed fields in
// the order of idx, the nI columns q_I, the nD exponent columns of D, A^(-w), the points C_I, C_J, B, D: 659 + 32 nattr + 80 nI + 32 nD bytes
struct ac_rbbs_redact_slab { uint8_t *a49, *a96, *st_a, *st, *sca, *scw, *aI48, *q32, *scd, *t96, *o96; size_t bytes; };
inline ac_rbbs_redact_slab ac_rbbs_redact_layout(void* base, size_t m, size_t nattr, size_t nI, size_t nD) {
    carver f(base, AC_RBBS_PUB_BYTES);
    ac_rbbs_redact_slab s;
    s.a49 = f.take(49 * m); s.a96 = f.take(96 * m); s.st_a = f.take(m); s.st = f.take(m); s.sca = f.take(32 * nattr * m); s.scw = f.take(32 * m);
    s.aI48 = f.take(48 * nI * m); s.q32 = f.take(32 * nI * m); s.scd = f.take(32 * nD * m); s.t96 = f.take(96 * m); s.o96 = f.take(4 * 96 * m);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- AC-rps (WS_AC_RPS): every slab starts behind the public block
constexpr size_t AC_RPS_PUB_BYTES = 22016;
// the public block.  verify: the nI + 1 used records of pk.Y (the base list) and of pk.tilde_Y (the disclosed ones in the order of idx, then
// tilde_Y[nattr]) as they arrive (y49, ty97) and decoded (l96, ty192); redact: the nI used records of pk.tilde_Y likewise; pres: all 2 nattr + 1
// records of pk.Y decoded (y96) and the base list gathered from them (l96).  verify and pres: g and tilde_g, tilde_X decoded straight from
// pk.fixed_part.  st: the status bytes of what the entry decodes — g, tilde_g, tilde_X, then the Y (and, behind them, the tilde_Y); redact: the tilde_Y
struct ac_rps_public {
    uint8_t *y49, *ty97, *g96, *y96, *l96, *g2, *ty192, *st;  // 32 x 49 B; 33 x 97 B; 96 B; 65 x 96 B; 32 x 96 B; 2 x 192 B; 32 x 192 B; 3 + 65 B
    explicit ac_rps_public(uint8_t* d)
        : y49(d), ty97(d + 1792), g96(d + 5120), y96(d + 5376), l96(d + 11776), g2(d + 14848), ty192(d + 15360), st(d + 21504) {}
};
// verify, per presentation of a chunk: sigma1_, C, sigma3_, sigma2_ (columns, in that order) and tilde_sigma_ as they arrive; S and the four decoded
// (S in front: S | sigma1_ and sigma1_ | C and sigma3_ | sigma2_ are each the point columns of one launch); tilde_sigma_ decoded and W behind it; the
// G2 sum; the five decoding statuses, the parse statuses of c0, s0 and of the disclosed values; the scalars s0, c0; the nI columns a_I; the hashed
// prefix; the nI + 1 columns q; the encodings sigma1_, C, C0, sigma2_; the Schnorr transcript and its hash; five Miller values, e(C, tilde_Y[nattr])'s,
// two conjugates; both verdicts: 6632 + 120 nI bytes
struct ac_rps_verify_slab { uint8_t *p49, *p97, *a96, *q192, *w192, *st_p, *st, *st_a, *sc2, *sca, *pre, *q32, *e49, *tr, *c32, *gt, *ge, *gh, *okp; size_t bytes; };
inline ac_rps_verify_slab ac_rps_verify_layout(void* base, size_t m, size_t nI) {
    carver f(base, AC_RPS_PUB_BYTES);
    ac_rps_verify_slab s;
    s.p49 = f.take(4 * 49 * m); s.p97 = f.take(97 * m); s.a96 = f.take(5 * 96 * m); s.q192 = f.take(2 * 192 * m); s.w192 = f.take(192 * m);
    s.st_p = f.take(5 * m); s.st = f.take(m); s.st_a = f.take(m); s.sc2 = f.take(2 * 32 * m); s.sca = f.take(32 * nI * m);
    s.pre = f.take((195 + 56 * nI) * m + 4); s.q32 = f.take(32 * (nI + 1) * m); s.e49 = f.take(4 * 49 * m); s.tr = f.take(147 * m + 4); s.c32 = f.take(32 * m);
    s.gt = f.take(5 * 576 * m); s.ge = f.take(576 * m); s.gh = f.take(2 * 576 * m); s.okp = f.take(2 * m);
    s.bytes = f.bytes;
    return s;
}
// pres, per presentation: h, sigma and tilde_M, tilde_H as they arrive; h, sigma decoded and sigma1_ behind them; sigma1_ twice; tilde_M, tilde_H
// decoded; tilde_g^t; the four decoding statuses and the parse status; the scalars r | r, t | z, rho | t; the hashed prefix; the nI + 1 columns q;
// the `total` columns of sigma3_'s sum; the encodings sigma2_, sigma1_, C, C0 and sigma3_, tilde_sigma_; the Schnorr transcript and its hash:
// 2293 + 88 nI + 32 total bytes
struct ac_rps_pres_slab { uint8_t *p49, *p97, *a96, *b96, *m192, *t192, *st_p, *st, *scr, *sc2, *scz, *sct, *pre, *q32, *sc3, *e49, *s3_49, *ts97, *tr, *c32; size_t bytes; };
inline ac_rps_pres_slab ac_rps_pres_layout(void* base, size_t m, size_t nI, size_t total) {
    carver f(base, AC_RPS_PUB_BYTES);
    ac_rps_pres_slab s;
    s.p49 = f.take(2 * 49 * m); s.p97 = f.take(2 * 97 * m); s.a96 = f.take(3 * 96 * m); s.b96 = f.take(2 * 96 * m); s.m192 = f.take(2 * 192 * m);
    s.t192 = f.take(192 * m); s.st_p = f.take(4 * m); s.st = f.take(m); s.scr = f.take(32 * m); s.sc2 = f.take(2 * 32 * m); s.scz = f.take(2 * 32 * m);
    s.sct = f.take(32 * m); s.pre = f.take((195 + 56 * nI) * m + 4); s.q32 = f.take(32 * (nI + 1) * m); s.sc3 = f.take(32 * total * m);
    s.e49 = f.take(4 * 49 * m); s.s3_49 = f.take(49 * m); s.ts97 = f.take(97 * m); s.tr = f.take(147 * m + 4); s.c32 = f.take(32 * m);
    s.bytes = f.bytes;
    return s;
}
// redact, per credential: h, sigma and tilde_M as they arrive; h, sigma decoded (for their statuses alone) and tilde_M decoded; the three decoding
// statuses and the parse status; the nI columns a_I; the G2 sum; tilde_H encoded: 872 + 32 nI bytes
struct ac_rps_redact_slab { uint8_t *p49, *p97, *a96, *m192, *st_p, *st, *sca, *w192, *h97; size_t bytes; };
inline ac_rps_redact_slab ac_rps_redact_layout(void* base, size_t m, size_t nI) {
    carver f(base, AC_RPS_PUB_BYTES);
    ac_rps_redact_slab s;
    s.p49 = f.take(2 * 49 * m); s.p97 = f.take(97 * m); s.a96 = f.take(2 * 96 * m); s.m192 = f.take(192 * m); s.st_p = f.take(3 * m); s.st = f.take(m);
    s.sca = f.take(32 * nI * m); s.w192 = f.take(192 * m); s.h97 = f.take(97 * m);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- MHAC-bbs (WS_MHAC_BBS): both slabs start behind the public block
// The public block is ac_bbs_public's, read as: y49 / y96 the used h records gathered into the entry's base list (up to 32 positions) as they arrive
// and decoded, g96 = g1 of pp (decoded, not used), g2 = g2 of pp and w of pk (pres: g2 alone), st = the statuses g1, g2, w (pres: 1), then the list's
constexpr size_t MHAC_BBS_PUB_BYTES = AC_BBS_PUB_BYTES;
// verify, per presentation of a chunk: B_, C_rev, A_ as they arrive (columns) and decoded — the terms of the k = 3 product —, their statuses, its
// scalars -ch, zr, ze, the nb columns z .., zhp .. of the verify list, ch, the parse status, the product, the sum over the list, U compressed, the
// pairing verdict, the transcript of nrp revealed values: 956 + 32 nb + 48 nrp bytes
struct mhac_bbs_verify_slab { uint8_t *p49, *p96, *st_p, *sc3, *sca, *c32, *st, *r96, *s96, *u49, *okp, *tr; size_t bytes; };
inline mhac_bbs_verify_slab mhac_bbs_verify_layout(void* base, size_t m, size_t nb, size_t nrp) {
    carver f(base, MHAC_BBS_PUB_BYTES);
    mhac_bbs_verify_slab s;
    s.p49 = f.take(3 * 49 * m); s.p96 = f.take(3 * 96 * m); s.st_p = f.take(3 * m); s.sc3 = f.take(3 * 32 * m); s.sca = f.take(32 * nb * m);
    s.c32 = f.take(32 * m); s.st = f.take(m); s.r96 = f.take(96 * m); s.s96 = f.take(96 * m); s.u49 = f.take(49 * m); s.okp = f.take(m);
    s.tr = f.take((147 + 48 * nrp) * m + 4);
    s.bytes = f.bytes;
    return s;
}
// pres, per presentation of a chunk: C_pub, D, A, C_rev as they arrive (columns) and decoded (C_pub * D replaces D: C_pub * D | A is the 2 m-lane G1
// column), their statuses and the parse status, r twice, the t + 1 columns alpha, gamma .., the `total` exponent columns of the pres list, the
// column's output B_ | A_, the five term columns C_rev, A_ x 4 of the k-way products, the running U and one further point, the transcript:
// 1692 + 32 (t + total) + 48 nrp bytes
struct mhac_bbs_pres_slab { uint8_t *p49, *p96, *st_p, *st, *scr, *scu, *sch, *o96, *q96, *u96, *v96, *tr; size_t bytes; };
inline mhac_bbs_pres_slab mhac_bbs_pres_layout(void* base, size_t m, size_t t, size_t total, size_t nrp) {
    carver f(base, MHAC_BBS_PUB_BYTES);
    mhac_bbs_pres_slab s;
    s.p49 = f.take(4 * 49 * m); s.p96 = f.take(4 * 96 * m); s.st_p = f.take(4 * m); s.st = f.take(m); s.scr = f.take(2 * 32 * m);
    s.scu = f.take(32 * (t + 1) * m); s.sch = f.take(32 * total * m); s.o96 = f.take(2 * 96 * m); s.q96 = f.take(5 * 96 * m); s.u96 = f.take(96 * m);
    s.v96 = f.take(96 * m); s.tr = f.take((147 + 48 * nrp) * m + 4);
    s.bytes = f.bytes;
    return s;
}
// The issuance entries (api_mhac_iss.hip).  attr and iss run k credentials of a chunk as k x nparties lanes (credential-major, the layout of
// their per-party outputs); a chunk holds mhac_iss_chunk(nparties) credentials, so no launch exceeds 2^18 lanes.
inline size_t mhac_iss_chunk(size_t nparties) { const size_t k = ((size_t)1 << 18) / nparties; return k ? k : 1; }
// attr, per credential: the nPrv share columns of its nparties lanes: 32 nPrv nparties bytes
struct mhac_iss_attr_slab { uint8_t* sc; size_t bytes; };
inline mhac_iss_attr_slab mhac_iss_attr_layout(void* base, size_t k, size_t nparties, size_t nPrv) {
    carver f(base, MHAC_BBS_PUB_BYTES);
    mhac_iss_attr_slab s;
    s.sc = f.take(32 * nPrv * nparties * k);
    s.bytes = f.bytes;
    return s;
}
// iss: gamma as 32 bytes and its range status in front (64 bytes for the chunk); per credential the nparties records of C decoded and their
// statuses, the parse status, e, inverse(gamma + e), the t columns lambda, the nPub public columns, the nparties scalars -e_share, the t term columns
// C[0] .. C[t-1] of the products, the product (then C_a), the public sum, A, A once per party, and A^(-e_share) (then D):
// 353 + 321 nparties + 128 t + 32 nPub bytes
struct mhac_iss_iss_slab { uint8_t *gam, *c96, *st_c, *st, *e32, *inv, *scl, *scp, *nes, *q96, *u96, *v96, *a96, *r96, *w96; size_t bytes; };
inline mhac_iss_iss_slab mhac_iss_iss_layout(void* base, size_t k, size_t nparties, size_t t, size_t nPub) {
    const size_t L = k * nparties;
    carver f(base, MHAC_BBS_PUB_BYTES);
    mhac_iss_iss_slab s;
    s.gam = f.take(64); s.c96 = f.take(96 * L); s.st_c = f.take(L); s.st = f.take(k); s.e32 = f.take(32 * k); s.inv = f.take(32 * k);
    s.scl = f.take(32 * t * k); s.scp = f.take(32 * nPub * k); s.nes = f.take(32 * L); s.q96 = f.take(96 * t * k); s.u96 = f.take(96 * k);
    s.v96 = f.take(96 * k); s.a96 = f.take(96 * k); s.r96 = f.take(96 * L); s.w96 = f.take(96 * L);
    s.bytes = f.bytes;
    return s;
}
// group (no key: the slab starts at the workspace), per presentation: the t records of S as they arrive (columns) and decoded, their statuses, the t
// columns lambda, the running product and one further point: 192 + 178 t bytes
struct mhac_iss_group_slab { uint8_t *p49, *p96, *st_p, *sc, *u96, *v96; size_t bytes; };
inline mhac_iss_group_slab mhac_iss_group_layout(void* base, size_t m, size_t t) {
    carver f(base);
    mhac_iss_group_slab s;
    s.p49 = f.take(49 * t * m); s.p96 = f.take(96 * t * m); s.st_p = f.take(t * m); s.sc = f.take(32 * t * m); s.u96 = f.take(96 * m); s.v96 = f.take(96 * m);
    s.bytes = f.bytes;
    return s;
}
// type, per presentation: the parse status, the nPub columns of the type list, C_rev, the sum over the hidden public positions, C_pub:
// 289 + 32 nPub bytes
struct mhac_iss_type_slab { uint8_t *st, *sca, *r96, *v96, *p96; size_t bytes; };
inline mhac_iss_type_slab mhac_iss_type_layout(void* base, size_t m, size_t nPub) {
    carver f(base, MHAC_BBS_PUB_BYTES);
    mhac_iss_type_slab s;
    s.st = f.take(m); s.sca = f.take(32 * nPub * m); s.r96 = f.take(96 * m); s.v96 = f.take(96 * m); s.p96 = f.take(96 * m);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- AC issuance (WS_AC_ISSUE, api_ac_issue.hip): every slab starts behind the public block
// The public block is ac_rps_public's, read as: g96 = g and g2 = tilde_g, tilde_X decoded straight from pk.fixed_part; y96 = Y[0 .. nattr) of pk.Y
// (AC-bbs / AC-rbbs) and ty192 = tilde_Y[0 .. nattr) of pk.tilde_Y (AC-rps), decoded where they lie in the key, in attribute order; st = the
// statuses g, tilde_g, tilde_X, then the nattr used records (user_keygen: the first three alone)
constexpr size_t AC_ISSUE_PUB_BYTES = AC_RPS_PUB_BYTES;
// AC-bbs / AC-rbbs issue, per credential of a chunk: the nattr attribute columns, w, x + w, its inverse, the parse status, the sum g * prod Y_i^a_i, A:
// 289 + 32 nattr bytes
struct ac_issue_bbs_slab { uint8_t *sca, *w32, *d32, *inv, *st, *b96, *a96; size_t bytes; };
inline ac_issue_bbs_slab ac_issue_bbs_layout(void* base, size_t m, size_t nattr) {
    carver f(base, AC_ISSUE_PUB_BYTES);
    ac_issue_bbs_slab s;
    s.sca = f.take(32 * nattr * m); s.w32 = f.take(32 * m); s.d32 = f.take(32 * m); s.inv = f.take(32 * m); s.st = f.take(m); s.b96 = f.take(96 * m);
    s.a96 = f.take(96 * m);
    s.bytes = f.bytes;
    return s;
}
// AC-rps user_keygen, per key pair: usk as the scalar of g: 32 bytes
struct ac_issue_keygen_slab { uint8_t* sc; size_t bytes; };
inline ac_issue_keygen_slab ac_issue_keygen_layout(void* base, size_t m) {
    carver f(base, AC_ISSUE_PUB_BYTES);
    ac_issue_keygen_slab s;
    s.sc = f.take(32 * m);
    s.bytes = f.bytes;
    return s;
}
// AC-rps issue, per credential: the nattr attribute columns, alpha, the scalars x + ym | alpha y^(nattr+1) of the k = 2 product, the parse status, upk's
// decoding status, the terms h | Z of the product, the encodings h | sigma, tilde_M encoded: 485 + 32 nattr bytes
struct ac_issue_rps_slab { uint8_t *sca, *al32, *sc2, *st, *st_z, *q96, *e49, *tm97; size_t bytes; };
inline ac_issue_rps_slab ac_issue_rps_layout(void* base, size_t m, size_t nattr) {
    carver f(base, AC_ISSUE_PUB_BYTES);
    ac_issue_rps_slab s;
    s.sca = f.take(32 * nattr * m); s.al32 = f.take(32 * m); s.sc2 = f.take(2 * 32 * m); s.st = f.take(m); s.st_z = f.take(m); s.q96 = f.take(2 * 96 * m);
    s.e49 = f.take(2 * 49 * m); s.tm97 = f.take(97 * m);
    s.bytes = f.bytes;
    return s;
}

// ---------------------------------------------------------------- pairing work queue (WS_PAIR_ST; the GT power: WS_POW_ST)
// The figures of the queue kernels (api_pair.hip asserts them against kernels.hpp): 21 pairings per wavefront group, 4 wavefronts per
// workgroup, a grid that fills the machine at 2 wavefronts per SIMD, and a queued group's state block in the tagged / the fenced form.
constexpr size_t QUEUE_GROUP_ELEMS = 21, QUEUE_WAVES_PER_BLOCK = 4, PAIR_QUEUE_WAVES = 2048;
constexpr size_t QUEUE_BLOCK_TAGGED = (size_t)168 * 64 * 8, QUEUE_BLOCK_FENCED = (size_t)42 * 1024;
// THE split of the hybrid schedule, evaluated here (the kernels take ndirect as an argument; gt3_pow_queue_kernel alone keeps a transcription,
// k_pair3.hip gt_pow_direct_groups, which has to stay this text): how many of `ngroups`
// groups the `nwaves` wavefronts of the grid run whole, ahead of the queue; the rest goes through the queue in tasks.
// Groups left to the tenth-length queue tasks at the end of a launch.  Measured on MI355X (profiles/r02_ab_queued_groups.txt):
// 2^16 pairings (3121 groups, 2048 resident wavefronts): 2048 queued 21.8 ms, 1024 queued 19.4 ms, 512 queued 20.1 ms;
// 2^18 BBS+ verifications (12484 groups): 2048 queued 82.0 ms, 1024 queued 82.4 ms, 512 queued 88.9 ms, 256 queued 97.3 ms —
// the more whole groups a wavefront runs, the further apart the wavefronts finish: a third of the groups, between half a
// grid and two grids (re-measured with the normalised line tables: 12484 groups, 2048 queued 83.2 ms, 4096 80.5, 6144 80.4, all 82.1).
// A batch that fits the grid is queued whole (the queue forced on for a small batch: tests of the queue path).
// override_groups > 0 (tuning runs, C12381_QUEUE_GROUPS in an experiments build): that many groups go through the queue.
inline size_t queue_direct_groups(size_t ngroups, size_t nwaves, int override_groups) {
    if (ngroups <= nwaves) return 0;
    size_t queued = ngroups / 3;
    if (queued < nwaves / 2) queued = nwaves / 2;
    if (queued > 2 * nwaves) queued = 2 * nwaves;
    if (override_groups > 0) queued = (size_t)override_groups < ngroups ? (size_t)override_groups : ngroups;
    return ngroups - queued;
}
// [flags: one word per group][task counter][whole-group counter][pad to 256 B][one state block per QUEUED group] — whole groups keep
// their state in registers and the LDS slot; 2^18 BBS+ verifications: 4096 blocks (344 MB) instead of 12484 (1.0 GB).  `blocks`
// workgroups = `nwaves` wavefronts are launched; groups [0, ndirect) run whole, queued group ndirect + j owns block j of `state`.
struct pair_queue_slab { uint8_t *flags, *counter, *state; unsigned blocks; size_t nwaves, ndirect, nq, bytes; };
inline pair_queue_slab pair_queue_layout(void* base, size_t n, bool tagged, int override_groups) {
    const size_t groups = (n + QUEUE_GROUP_ELEMS - 1) / QUEUE_GROUP_ELEMS;
    const size_t waves = groups < PAIR_QUEUE_WAVES ? groups : PAIR_QUEUE_WAVES;
    carver f(base);
    pair_queue_slab s;
    s.flags = f.take((groups + 2) * 4);
    s.counter = s.flags ? s.flags + groups * 4 : nullptr;
    s.blocks = (unsigned)((waves + QUEUE_WAVES_PER_BLOCK - 1) / QUEUE_WAVES_PER_BLOCK);
    s.nwaves = (size_t)s.blocks * QUEUE_WAVES_PER_BLOCK;
    s.ndirect = queue_direct_groups(groups, s.nwaves, override_groups);
    s.nq = groups - s.ndirect;
    s.state = f.take(s.nq * (tagged ? QUEUE_BLOCK_TAGGED : QUEUE_BLOCK_FENCED));
    s.bytes = f.bytes;
    return s;
}

}  // namespace c12381_host
