// The pairing entries of the C ABI (include/c12381_hip.h): pairings, pair_eq, products, the forms against fixed G2 points with their line tables,
// the work-queue setup and its diagnostic stamps, Miller loops and GT operations.  Kernels: k_pair3.hip, k_pairk.hip, k_g2gt.hip; the shared
// host pieces: host.hpp.
#include "host.hpp"
#include "pairing3.hpp"

using namespace c12381;
using namespace c12381_host;

// Line tables (host.hpp "device-built tables"): one Q (pair_fixed_g2), BBS+'s w and g2 (rule 1), the k points of a product.  bbs04's product
// (rule 0) and BBS+ have a workspace each, so neither evicts the other's tables.
static_assert(FIXED_G2_MAX <= TABLE_ARRAY_MAX, "table_points holds the points of the largest array");
constexpr size_t FQ_TAB_DWORDS = table_dwords(FQ_TABLE_DWORDS);
constexpr table_array TA_FQ_P = {c12381_ctx::WS_FQ_P, 1, FQ_TAB_DWORDS, 0, 192};
constexpr table_array TA_FQ_WG = {c12381_ctx::WS_FQ_W, 2, FQ_TAB_DWORDS, GATE_DWORDS, 192};
constexpr table_array TA_FQ_K = {c12381_ctx::WS_FQ_K, FIXED_G2_MAX, FQ_TAB_DWORDS, GATE_DWORDS, 192};
// the tables of the k points q.p[j] in array `a` and, where the array has one, the gate over the k
static int lines_tables(c12381_ctx* c, const table_array& a, int k, const g2_cols& q, int rule, cached& t) {
    table_points pts = {};
    for (int j = 0; j < k; ++j) pts.p[j] = q.p[j];
    int rc = cached_tables(c, a, k, pts, t, [&](const cached& b) {
        LAUNCH_ON(c, g2_lines_tables_kernel, dim3(1), dim3(BLOCK), c->stream, k, q, b.tabs, b.stride, rule);
        return 0;
    });
    if (rc || !a.gate) return rc;
    LAUNCH_ON(c, gate_all_kernel, dim3(1), dim3(BLOCK), c->stream, t.gate, (const int32_t*)t.tabs, t.stride, k);
    return 0;
}
int c12381_host::lines_tables_k(c12381_ctx* c, int k, const g2_cols& q, int rule, cached& t) { return lines_tables(c, TA_FQ_K, k, q, rule, t); }
g2_cols c12381_host::g2_key_cols(const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192, size_t nmsg) {
    g2_cols q = {};
    q.p[0] = g2_192; q.p[1] = X2_192;
    for (size_t i = 0; i < nmsg; ++i) q.p[2 + i] = Y2_192 + 192 * i;
    return q;
}
// the rule of the entry points whose product is followed by the final exponentiation: C12381_FQ_RAW=1 keeps their records raw (A/B switch)
static int fq_rule(int need_g2) {
    static const int raw = [] { const char* e = tuning_env("C12381_FQ_RAW"); return (e && e[0] == '1') ? 2 : 0; }();
    return need_g2 | raw;
}
int c12381_host::bbs_lines_tables(c12381_ctx* c, const uint8_t* w_192, const uint8_t* g2_192, cached& t) {
    g2_cols q = {};
    q.p[0] = w_192; q.p[1] = g2_192;
    return lines_tables(c, TA_FQ_WG, 2, q, fq_rule(1), t);
}
// ---------------------------------------------------------------- pairing
// C12381_PAIR_LANES=1 selects the one-lane-per-pairing kernels (kept for A/B measurements); default is 3.
#ifdef C12381_EXPERIMENTS
int c12381_host::pair_lanes() {
    static const int v = [] { const char* e = tuning_env("C12381_PAIR_LANES"); return (e && e[0] == '1') ? 1 : 3; }();
    return v;
}
#else
int c12381_host::pair_lanes() { return 3; }
#endif
static unsigned grid_tri(size_t n) {
    const size_t waves = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
    return (unsigned)((waves * 64 + BLOCK - 1) / BLOCK);
}
// Work-queue variant (k_pair3.hip): used when the batch is more than one machine-filling round of wavefronts, where the
// plain grid would end in a mostly idle round (PAIR_QUEUE_WAVES, host_layouts.hpp: the resident wavefronts at 2 per SIMD).
// C12381_PAIR_QUEUE=0 / 1 forces it off / on (A/B measurements, tests).
static int pair_queue_mode() {
    static const int v = [] { const char* e = tuning_env("C12381_PAIR_QUEUE"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    return v;
}
// bound of the hand-over spin in the queue kernels (pair_queue.hpp queue_wait_rlx / queue_wait): 2^20 sleeps of 4096 cycles, about two
// seconds — three orders of magnitude beyond a task.  C12381_PAIR_SPIN_LIMIT overrides it; a negative value makes every
// wait fail (tests of the poison path).
static int pair_spin_limit() {
    static const int v = [] { const char* e = tuning_env("C12381_PAIR_SPIN_LIMIT"); return e ? std::atoi(e) : (1 << 20); }();
    return v;
}
// Diagnostic: C12381_PAIR_STAMPS=<file> makes every task of pair3_queue_kernel record its claim / start / end times (s_memtime)
// into a device buffer that c12381_sync() writes to the file — per-phase durations and hand-over waits (tools/queue_phase_times.py).
static const char* pair_stamps_path() {
    static const char* p = tuning_env("C12381_PAIR_STAMPS");
    return p;
}
static unsigned long long* pair_stamps(c12381_ctx* c, size_t n) {
    if (!pair_stamps_path()) return nullptr;
    const size_t tasks = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE * 16;      // ten per group (room for up to 14), one more for its whole-group stamp
    if (c->stamps_tasks < tasks) {
        (void)hipStreamSynchronize(c->stream);              // a kernel of this context may still be writing the old buffer
        if (c->stamps) (void)hipFree(c->stamps);
        if (hipMalloc((void**)&c->stamps, tasks * 32 + c12381_ctx::STAMP_WAVES * 96) != hipSuccess) { c->stamps = nullptr; c->stamps_tasks = 0; return nullptr; }
        c->stamps_tasks = tasks;
    }
    (void)hipMemsetAsync(c->stamps, 0, c->stamps_tasks * 32 + c12381_ctx::STAMP_WAVES * 96, c->stream);
    return c->stamps;
}
// the per-wavefront region behind the per-task stamps (null when the diagnostic is off)
static unsigned long long* pair_wave_stats(c12381_ctx* c, size_t n) {
    unsigned long long* s = pair_stamps(c, n);
    return s ? s + c->stamps_tasks * 4 : nullptr;
}
void c12381_host::pair_stamps_dump(c12381_ctx* c) {
    if (!pair_stamps_path() || !c->stamps) return;
    std::vector<unsigned long long> h(c->stamps_tasks * 4 + c12381_ctx::STAMP_WAVES * 12);
    if (hipMemcpy(h.data(), c->stamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    if (FILE* f = std::fopen(pair_stamps_path(), "wb")) { std::fwrite(h.data(), 8, h.size(), f); std::fclose(f); }
}
static bool pair_use_queue(size_t n) {
    const int m = pair_queue_mode();
    if (m >= 0) return m == 1;
    return (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE > PAIR_QUEUE_WAVES;
}
// The queue of one launch: the slab (host_layouts.hpp pair_queue_layout — the split rule lives there and is evaluated here; the kernels take
// ndirect as an argument, all but gt3_pow_queue_kernel, which keeps a transcription of the rule: k_pair3.hip) and, for the tagged form, this launch's epoch.
// tagged (every kernel but the GT power): blocks of PAIR_QUEUE_STATE_BYTES in 8-byte tagged words, `epoch` = this launch's tag base.  The slab
// then only ever holds tagged words or zeros (zeroed when it is allocated and when the 28-bit epoch wraps), so a word of an earlier launch —
// at whatever offset that launch's group count put it — can never carry the tag of this one.  The GT power keeps the fenced 16-byte rows in a
// slab of its own.
static_assert(QUEUE_GROUP_ELEMS == TRI_PER_WAVE && QUEUE_WAVES_PER_BLOCK * 64 == BLOCK && QUEUE_BLOCK_TAGGED == PAIR_QUEUE_STATE_BYTES &&
              QUEUE_BLOCK_FENCED == (size_t)PAIR_QUEUE_STATE_ROWS * 1024, "host_layouts.hpp: the queue's figures are those of kernels.hpp");
struct pair_queue : pair_queue_slab {           // the layout's values as they are, plus the epoch; the kernels' pointer types
    unsigned int epoch;
    uint4* st() const { return (uint4*)state; }
    unsigned int* fl() const { return (unsigned int*)flags; }
    unsigned int* ct() const { return (unsigned int*)counter; }
};
static int pair_queue_setup(c12381_ctx* c, size_t n, pair_queue& pq, bool tagged = true) {
    const int slot = tagged ? c12381_ctx::WS_PAIR_ST : c12381_ctx::WS_POW_ST;
    const size_t bytes = pair_queue_layout(nullptr, n, tagged, g_queue_groups_host).bytes;          // sizing pass, then the workspace (host_layouts.hpp)
    bool fresh = c->ws_bytes[slot] < bytes;
    int rc;
    if ((rc = ensure(c, slot, bytes))) return rc;
    static_cast<pair_queue_slab&>(pq) = pair_queue_layout(c->ws[slot], n, tagged, g_queue_groups_host);
    pq.epoch = 0;
    if (tagged) {
        c->queue_epoch = (c->queue_epoch + 1u) & 0x0fffffffu;
        if (c->queue_epoch == 0) { c->queue_epoch = 1; fresh = true; }
        if (fresh) HIPCK(c, hipMemsetAsync(c->ws[slot], 0, c->ws_bytes[slot], c->stream));
        pq.epoch = c->queue_epoch;
    }
    HIPCK(c, hipMemsetAsync(pq.flags, 0, (size_t)(pq.counter - pq.flags) + 8, c->stream));       // flags and both counters
    return 0;
}
static int launch_pair(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt) {
#ifdef C12381_EXPERIMENTS
    if (pair_lanes() == 1) { LAUNCH(c, pair_kernel, n, n, g1, g2, gt, c->d_flag); return 0; }
#endif
    if (pair_use_queue(n)) {
        pair_queue pq; int rc;
        if ((rc = pair_queue_setup(c, n, pq))) return rc;
        unsigned long long* const stp = pair_stamps(c, n);
        LAUNCH_ON(c, pair3_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, g1, g2, gt, c->d_flag, pq.st(), pq.fl(), pq.ct(), pq.ndirect,
                  pair_spin_limit(), pq.epoch, stp,
                  stp ? stp + c->stamps_tasks * 4 : nullptr);
    } else LAUNCH_ON(c, pair3_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, n, g1, g2, gt, c->d_flag);
    return 0;
}
int c12381_host::launch_pair_eq(c12381_ctx* c, size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, size_t b2_stride,
                                uint8_t* ok, const int32_t* skip_if) {
#ifdef C12381_EXPERIMENTS
    if (pair_lanes() == 1) { LAUNCH(c, pair_eq_kernel, n, n, a1, a2, b1, b2, b2_stride, ok, c->d_flag); return 0; }
#endif
    if (pair_use_queue(n)) {
        pair_queue pq; int rc;
        if ((rc = pair_queue_setup(c, n, pq))) return rc;
        LAUNCH_ON(c, pair3_eq_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, a1, a2, b1, b2, b2_stride, ok, c->d_flag, pq.st(), pq.fl(), pq.ct(),
                  skip_if, pq.ndirect, pair_spin_limit(),
                  pq.epoch);
    } else LAUNCH_ON(c, pair3_eq_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, n, a1, a2, b1, b2, b2_stride, ok, c->d_flag, skip_if);
    return 0;
}
// (also the check of c12381_pair_fixed_g2_batch and c12381_miller_batch, with flags 0)
static int pair_args(const void* g1, const void* g2, const void* gt, unsigned flags) {
    return (!g1 || !g2 || !gt || (flags & ~(unsigned)C12381_F_COMPRESSED_IN)) ? C12381_E_ARG : 0;
}
int c12381_pair_batch_dev(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt) {
    int rc = bind(c) ?: pair_args(g1, g2, gt, 0u);
    if (rc || n == 0) return rc;
    if (pair_lanes() != 1 && pair_use_queue(n)) {            // workspace and its reset stay outside the timed bracket
        pair_queue pq;
        if ((rc = pair_queue_setup(c, n, pq))) return rc;
        timed tm(c, 3);
        unsigned long long* const stp = pair_stamps(c, n);
        LAUNCH_ON(c, pair3_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, g1, g2, gt, c->d_flag, pq.st(), pq.fl(), pq.ct(), pq.ndirect,
                  pair_spin_limit(), pq.epoch, stp,
                  stp ? stp + c->stamps_tasks * 4 : nullptr);
        return 0;
    }
    timed tm(c, 3);
    return launch_pair(c, n, g1, g2, gt);
}
// C12381_F_COMPRESSED_IN: g1 = n x 49, g2 = n x 97 bytes.  The pairing kernels read their inputs once per queue task (up to five times),
// so the decoding runs as its own two kernels into a workspace (288 B per pairing, against ~280 ns of arithmetic); a rejected
// encoding becomes an off-curve record there and surfaces exactly like an invalid 96 / 192-byte input: 0xff lane, C12381_E_POINT.
int c12381_pair_batch_flags_dev(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, unsigned flags) {
    int rc = bind(c) ?: pair_args(g1, g2, gt, flags);
    if (rc || n == 0) return rc;
    if (!(flags & C12381_F_COMPRESSED_IN)) return c12381_pair_batch_dev(c, n, g1, g2, gt);
    if ((rc = ensure(c, c12381_ctx::WS_DEC1, 96 * n))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_DEC2, 192 * n))) return rc;
    uint8_t *d1 = (uint8_t*)c->ws[c12381_ctx::WS_DEC1], *d2 = (uint8_t*)c->ws[c12381_ctx::WS_DEC2];
    LAUNCH(c, g1_decompress_kernel, n, n, g1, d1, (uint8_t*)nullptr, 1);
    LAUNCH(c, g2_decompress_kernel, n, n, g2, d2, (uint8_t*)nullptr, 1);
    return c12381_pair_batch_dev(c, n, d1, d2, gt);
}
int c12381_pair_batch_flags(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, unsigned flags) {
    int rc = bind(c) ?: pair_args(g1, g2, gt, flags);
    if (rc || n == 0) return rc;
    const bool comp = (flags & C12381_F_COMPRESSED_IN) != 0;
    return host_form(c, {{g1, (comp ? 49 : 96) * n}, {g2, (comp ? 97 : 192) * n}}, {{gt, 576 * n}},
                     [&](const staging& s) { return c12381_pair_batch_flags_dev(c, n, s.in[0], s.in[1], s.out[0], flags); });
}
int c12381_pair_batch(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt) { return c12381_pair_batch_flags(c, n, g1, g2, gt, 0u); }
// Product of k pairings per element with shared squarings (pair3_prod_kernel)
static int pair_product_args(int k, const void* g1s, const void* g2s, const void* gt, unsigned flags) {
    return (!g1s || !g2s || !gt || k < 1 || k > MAX_PROD || (flags & ~(unsigned)C12381_F_MILLER_ONLY)) ? C12381_E_ARG : 0;
}
int c12381_pair_product_batch_dev(c12381_ctx* c, size_t n, int k, const uint8_t* g1s, const uint8_t* g2s, uint8_t* gt, unsigned flags) {
    int rc = bind(c) ?: pair_product_args(k, g1s, g2s, gt, flags);
    if (rc || n == 0) return rc;
    timed tm(c, 3);
    LAUNCH_ON(c, pair3_prod_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, n, k, g1s, g2s, gt, c->d_flag, (flags & C12381_F_MILLER_ONLY) ? 1 : 0);
    return 0;
}
int c12381_pair_product_batch(c12381_ctx* c, size_t n, int k, const uint8_t* g1s, const uint8_t* g2s, uint8_t* gt, unsigned flags) {
    int rc = bind(c) ?: pair_product_args(k, g1s, g2s, gt, flags);
    if (rc || n == 0) return rc;
    return host_form(c, {{g1s, 96 * n * (size_t)k}, {g2s, 192 * n * (size_t)k}}, {{gt, 576 * n}},
                     [&](const staging& s) { return c12381_pair_product_batch_dev(c, n, k, s.in[0], s.in[1], s.out[0], flags); });
}
// gt[i] = e(P_i, Q) with ONE G2 argument for the batch: the 69 line-coefficient triples of Q are computed once (and kept
// until Q changes), every element then runs the table-driven Miller loop.  Same field elements as the running-point loop,
// so the GT bytes equal c12381_pair_batch on n copies of Q for every Q, infinity included.
int c12381_pair_fixed_g2_batch_dev(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2_192, uint8_t* gt) {
    int rc = bind(c) ?: pair_args(g1, g2_192, gt, 0u);
    if (rc || n == 0) return rc;
    g2_cols q = {};
    q.p[0] = g2_192;
    cached t;
    if ((rc = lines_tables(c, TA_FQ_P, 1, q, fq_rule(0), t))) return rc;
    pair_queue pq;
    if ((rc = pair_queue_setup(c, n, pq))) return rc;
    timed tm(c, 3);
    LAUNCH_ON(c, pair3_fixed_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, g1, (const int32_t*)t.tabs, gt, c->d_flag, pq.st(), pq.fl(), pq.ct(),
              pq.ndirect, pair_spin_limit(), pq.epoch);
    return 0;
}
int c12381_pair_fixed_g2_batch(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2_192, uint8_t* gt) {
    int rc = bind(c) ?: pair_args(g1, g2_192, gt, 0u);
    if (rc || n == 0) return rc;
    return host_form(c, {{g1, 96 * n}, {g2_192, 192}}, {{gt, 576 * n}},
                     [&](const staging& s) { return c12381_pair_fixed_g2_batch_dev(c, n, s.in[0], s.in[1], s.out[0]); });
}
// ---------------------------------------------------------------- K-way products against fixed G2 points (k_pairk.hip)
static_assert(C12381_FIXED_G2_MAX == FIXED_G2_MAX, "public and device bound of k");
int c12381_host::launch_prodk(c12381_ctx* c, size_t n, int k, const g1_cols& cols, uint32_t neg_mask, const cached& t, uint8_t* out, bool eq, bool miller_only,
                              const int32_t* prep_skip) {
    const int32_t *gate = t.gate, *lines = t.tabs + HDR_DWORDS;
    const size_t rec_bytes = round_up((size_t)k * n * FQK_PT_DWORDS * 4, 256);
    int rc;
    if ((rc = ensure(c, c12381_ctx::WS_FQK_PTS, rec_bytes + round_up(n * 4, 256)))) return rc;
    int32_t* pts = (int32_t*)c->ws[c12381_ctx::WS_FQK_PTS];
    uint32_t* mask = (uint32_t*)((uint8_t*)pts + rec_bytes);
    LAUNCH(c, pairk_prep_kernel, n, n, k, cols, neg_mask, pts, mask, prep_skip);
    pair_queue pq;
    if ((rc = pair_queue_setup(c, n, pq))) return rc;
    if (eq)
        LAUNCH_ON(c, pair3_prodk_fixed_eq_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, k, (const int32_t*)pts, (const uint32_t*)mask, lines, t.stride, out,
                  c->d_flag, pq.st(), pq.fl(), pq.ct(), gate, pq.ndirect, pair_spin_limit(), pq.epoch);
    else
        LAUNCH_ON(c, pair3_prodk_fixed_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, k, (const int32_t*)pts, (const uint32_t*)mask, lines, t.stride, out,
                  c->d_flag, pq.st(), pq.fl(), pq.ct(), gate, pq.ndirect, miller_only ? 1 : 0, pair_spin_limit(), pq.epoch);
    return 0;
}
int c12381_host::launch_prod_fixed(c12381_ctx* c, size_t n, const uint8_t* a_96, const uint8_t* b_96, const cached& lines, uint8_t* ok, const int32_t* gate) {
    pair_queue pq; int rc;
    if ((rc = pair_queue_setup(c, n, pq))) return rc;
    LAUNCH_ON(c, pair3_prod_fixed_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, a_96, b_96, (const int32_t*)lines.tabs + HDR_DWORDS,
              (const int32_t*)lines.tabs + lines.stride + HDR_DWORDS, ok, c->d_flag, pq.st(), pq.fl(), pq.ct(), gate, pq.ndirect, pair_spin_limit(), pq.epoch);
    return 0;
}
// gt[i] = prod_{j < k} e(g1s[j * n + i], g2s[j]): the k line tables are built with need_g2 = 0 (exact for every point of the twist, infinity
// included), raw under C12381_F_MILLER_ONLY (the Miller value itself is the output).
static int pair_product_fixed_args(int k, const void* g1s, const void* g2s, const void* gt, unsigned flags) {
    return (!g1s || !g2s || !gt || k < 1 || k > C12381_FIXED_G2_MAX || (flags & ~(unsigned)C12381_F_MILLER_ONLY)) ? C12381_E_ARG : 0;
}
int c12381_pair_product_fixed_g2_batch_dev(c12381_ctx* c, size_t n, int k, const uint8_t* g1s, const uint8_t* g2s, uint8_t* gt, unsigned flags) {
    int rc = bind(c) ?: pair_product_fixed_args(k, g1s, g2s, gt, flags);
    if (rc || n == 0) return rc;
    const bool miller_only = (flags & C12381_F_MILLER_ONLY) != 0;
    g1_cols cols = {};
    g2_cols q = {};
    for (int j = 0; j < k; ++j) { cols.p[j] = g1s + (size_t)96 * n * j; q.p[j] = g2s + (size_t)192 * j; }
    cached t;
    if ((rc = lines_tables(c, TA_FQ_K, k, q, miller_only ? 2 : 0, t))) return rc;
    timed tm(c, 3);
    return launch_prodk(c, n, k, cols, 0u, t, gt, false, miller_only, nullptr);
}
int c12381_pair_product_fixed_g2_batch(c12381_ctx* c, size_t n, int k, const uint8_t* g1s, const uint8_t* g2s, uint8_t* gt, unsigned flags) {
    int rc = bind(c) ?: pair_product_fixed_args(k, g1s, g2s, gt, flags);
    if (rc || n == 0) return rc;
    return host_form(c, {{g1s, 96 * n * (size_t)k}, {g2s, 192 * (size_t)k}}, {{gt, 576 * n}},
                     [&](const staging& s) { return c12381_pair_product_fixed_g2_batch_dev(c, n, k, s.in[0], s.in[1], s.out[0], flags); });
}
static int pair_eq_args(const void* a1, const void* a2, const void* b1, const void* b2, const void* ok) { return (!a1 || !a2 || !b1 || !b2 || !ok) ? C12381_E_ARG : 0; }
int c12381_pair_eq_batch_dev(c12381_ctx* c, size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, uint8_t* ok) {
    int rc = bind(c) ?: pair_eq_args(a1, a2, b1, b2, ok);
    if (rc || n == 0) return rc;
    timed tm(c, 4);
    return launch_pair_eq(c, n, a1, a2, b1, b2, (size_t)192, ok);
}
int c12381_pair_eq_batch(c12381_ctx* c, size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, uint8_t* ok) {
    int rc = bind(c) ?: pair_eq_args(a1, a2, b1, b2, ok);
    if (rc || n == 0) return rc;
    return host_form(c, {{a1, 96 * n}, {a2, 192 * n}, {b1, 96 * n}, {b2, 192 * n}}, {{ok, n}},
                     [&](const staging& s) { return c12381_pair_eq_batch_dev(c, n, s.in[0], s.in[1], s.in[2], s.in[3], s.out[0]); });
}
static int launch_miller(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out) {
#ifdef C12381_EXPERIMENTS
    if (pair_lanes() == 1) { LAUNCH(c, miller_kernel, n, n, g1, g2, out, c->d_flag); return 0; }
#endif
    if (pair_use_queue(n)) {              // more than one machine round of wavefront tasks: quarter-loop tasks from the work queue
        pair_queue pq; int rc;
        if ((rc = pair_queue_setup(c, n, pq))) return rc;
        LAUNCH_ON(c, miller3_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, g1, g2, out, c->d_flag, pq.st(), pq.fl(), pq.ct(), pq.ndirect,
                  pair_spin_limit(), pq.epoch, pair_wave_stats(c, n));
    } else LAUNCH_ON(c, miller3_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, n, g1, g2, out, c->d_flag);
    return 0;
}
static int launch_gt_op(c12381_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
#ifdef C12381_EXPERIMENTS
    if (pair_lanes() == 1) { LAUNCH(c, gt_op_kernel, n, op, n, a, b, out); return 0; }
#endif
    if (op == 3 && pair_use_queue(n)) {   // final exponentiations alone, more than one machine round: its six steps as queue tasks
        pair_queue pq; int rc;
        if ((rc = pair_queue_setup(c, n, pq))) return rc;
        LAUNCH_ON(c, fexp3_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, a, out, c->d_flag, pq.st(), pq.fl(), pq.ct(), pq.ndirect,
                  pair_spin_limit(), pq.epoch, pair_wave_stats(c, n));
    } else if (op == 2 && pair_use_queue(n)) {
        // the power, more than one machine round: five tasks per queued group (k_pair3.hip gt3_pow_queue_kernel); one table per wavefront of the
        // grid and one per queued group (at most 2048 + 4096 tables of 224 KB)
        pair_queue pq; int rc;
        if ((rc = pair_queue_setup(c, n, pq, false))) return rc;
        const size_t tables = pq.nwaves + pq.nq;
        // the rule queues at most 2 x the grid: 6144 tables = 1.4 GB, held until c12381_trim / c12381_destroy; a tuning override beyond that is refused
        if (tables > 3 * PAIR_QUEUE_WAVES) { std::snprintf(c->err, sizeof c->err, "GT power: %zu tables exceed the workspace budget (queued-groups override too large)", tables); return C12381_E_ARG; }
        if ((rc = ensure(c, c12381_ctx::WS_GT_POW, tables * GT_POW_TAB_BYTES_PER_WAVE))) return rc;
        LAUNCH_ON(c, gt3_pow_queue_kernel, dim3(pq.blocks), dim3(BLOCK), c->stream, n, a, b, out, c->d_flag, (uint4*)c->ws[c12381_ctx::WS_GT_POW], pq.st(),
                  pq.fl(), pq.ct(),
                  pair_spin_limit());        // this kernel evaluates the split itself (k_pair3.hip gt_pow_direct_groups): the same rule, the same override
    } else if (op == 2) {
        // the power in one plain launch: at most PAIR_QUEUE_WAVES wavefronts get here (longer batches took the queue above), each with its table
        // of x^0 .. x^15 behind it (224 KB per wavefront).  Only an experiments run with the queue forced off can be longer: it runs the
        // reference's digit sequence without tables.
        const size_t waves = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
        uint4* tab = nullptr;
        if (waves <= PAIR_QUEUE_WAVES) {
            int rc;
            if ((rc = ensure(c, c12381_ctx::WS_GT_POW, waves * GT_POW_TAB_BYTES_PER_WAVE))) return rc;
            tab = (uint4*)c->ws[c12381_ctx::WS_GT_POW];
        }
        LAUNCH_ON(c, gt3_op_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, op, n, a, b, out, tab);
    } else LAUNCH_ON(c, gt3_op_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, op, n, a, b, out, (uint4*)nullptr);
    return 0;
}
static int launch_gt_is_unity(c12381_ctx* c, size_t n, const uint8_t* a, uint8_t* out) {
#ifdef C12381_EXPERIMENTS
    if (pair_lanes() == 1) { LAUNCH(c, gt_is_unity_kernel, n, n, a, out); return 0; }
#endif
    LAUNCH_ON(c, gt3_is_unity_kernel, dim3(grid_tri(n)), dim3(BLOCK), c->stream, n, a, out);
    return 0;
}
int c12381_miller_batch_dev(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out576) {
    int rc = bind(c) ?: pair_args(g1, g2, out576, 0u);
    if (rc || n == 0) return rc;
    timed tm(c, 6);
    return launch_miller(c, n, g1, g2, out576);
}
int c12381_miller_batch(c12381_ctx* c, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out576) {
    int rc = bind(c) ?: pair_args(g1, g2, out576, 0u);
    if (rc || n == 0) return rc;
    return host_form(c, {{g1, 96 * n}, {g2, 192 * n}}, {{out576, 576 * n}},
                     [&](const staging& s) { return c12381_miller_batch_dev(c, n, s.in[0], s.in[1], s.out[0]); });
}
static int gt_op_args(int op, const void* a, const void* b, const void* out) {
    return (op < 0 || op > 3 || !a || !out || ((op == 0 || op == 2) && !b)) ? C12381_E_ARG : 0;
}
int c12381_gt_op_batch_dev(c12381_ctx* c, int op, size_t n, const uint8_t* a576, const uint8_t* b, uint8_t* out576) {
    int rc = bind(c) ?: gt_op_args(op, a576, b, out576);
    if (rc || n == 0) return rc;
    timed tm(c, 7);
    return launch_gt_op(c, op, n, a576, b, out576);
}
int c12381_gt_op_batch(c12381_ctx* c, int op, size_t n, const uint8_t* a576, const uint8_t* b, uint8_t* out576) {
    int rc = bind(c) ?: gt_op_args(op, a576, b, out576);
    if (rc || n == 0) return rc;
    const size_t bb = op == 0 ? 576 * n : (op == 2 ? 32 * n : 0);
    return host_form(c, {{a576, 576 * n}, {bb ? b : nullptr, bb}}, {{out576, 576 * n}},
                     [&](const staging& s) { return c12381_gt_op_batch_dev(c, op, n, s.in[0], s.in[1], s.out[0]); });
}
int c12381_fexp_batch(c12381_ctx* c, size_t n, const uint8_t* in576, uint8_t* out576) { return c12381_gt_op_batch(c, 3, n, in576, nullptr, out576); }
int c12381_fexp_batch_dev(c12381_ctx* c, size_t n, const uint8_t* in576, uint8_t* out576) { return c12381_gt_op_batch_dev(c, 3, n, in576, nullptr, out576); }
static int gt_is_unity_args(const void* a, const void* out) { return (!a || !out) ? C12381_E_ARG : 0; }
int c12381_gt_is_unity_batch_dev(c12381_ctx* c, size_t n, const uint8_t* a576, uint8_t* out) {
    int rc = bind(c) ?: gt_is_unity_args(a576, out);
    if (rc || n == 0) return rc;
    return launch_gt_is_unity(c, n, a576, out);
}
int c12381_gt_is_unity_batch(c12381_ctx* c, size_t n, const uint8_t* a576, uint8_t* out) {
    int rc = bind(c) ?: gt_is_unity_args(a576, out);
    if (rc || n == 0) return rc;
    return host_form(c, {{a576, 576 * n}}, {{out, n}}, [&](const staging& s) { return c12381_gt_is_unity_batch_dev(c, n, s.in[0], s.out[0]); });
}
