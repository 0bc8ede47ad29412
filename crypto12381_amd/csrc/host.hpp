// Host side shared by the units behind the C ABI (c12381_hip.hip, api_pair.hip, api_ps.hip, api_bbs.hip, api_bbs04.hip, api_ac_bbs.hip, api_ac_rbbs.hip, api_ac_rps.hip, api_mhac_bbs.hip, api_mhac_iss.hip, api_ac_issue.hip): the context and its
// workspaces, and the idioms every entry point is written in — launch, slab (host_layouts.hpp), host form.  Everything in namespace c12381_host
// has external linkage and hidden visibility: the units call each other's helpers, the library exports the C ABI alone.  The comment at each
// declaration names the unit that defines it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/c12381_hip.h"
#include "host_layouts.hpp"
#include "kernels.hpp"

struct c12381_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t side = nullptr;           // rare fix-up passes run here, overlapped with the next chunk on `stream`
    hipEvent_t ev_side = nullptr;
    std::vector<hipEvent_t> ev_chunk;     // one per chunk of a scalar-mul batch (main -> side dependencies)
    std::vector<hipStream_t> sort_streams; // further streams for the segment sorts of the bucket product (created on first use)
    std::vector<hipEvent_t> sort_events;
    char err[256] = {0};
    // WS_STAGE holds the caller's buffers of a host form (stage / unstage).  No _dev path uses it and no _dev path calls a host form
    // (host forms are synchronous), so a host form's slab is never overwritten while the call still needs it.
    enum { WS_TAB, WS_PROJ, WS_PREF, WS_STAGE, WS_RED0, WS_RED1, WS_BBS_Q, WS_BBS_B, WS_BBS_WIRE,
           WS_PAIR_ST, WS_POW_ST, WS_FQ_W, WS_FQ_P, WS_FB_G2, WS_FB_G1_0, WS_FB_G1_1, WS_FB_G1_2, WS_FB_G1_3, WS_FB_G1_4, WS_MSM_PTS, WS_MSM_K0, WS_MSM_K1, WS_MSM_V0, WS_MSM_V1, WS_MSM_TMP, WS_MSM_RNG, WS_MSM_BK, WS_MSM_ORD, WS_MSM_OVF, WS_DEC1, WS_DEC2, WS_GT_POW,
           WS_FQ_K, WS_FQK_PTS, WS_FQK_G1, WS_BBS04, WS_FB_G1_SUM, WS_FB_G2_SUM, WS_PS, WS_AC_BBS, WS_AC_RBBS, WS_AC_RPS, WS_MHAC_BBS, WS_AC_ISSUE, WS_COUNT };
    void* ws[WS_COUNT] = {nullptr};
    size_t ws_bytes[WS_COUNT] = {0};
    int* d_flag = nullptr;
    int* h_flag = nullptr;          // pinned
    // optional per-kernel timing (HIP events on the context's stream), see c12381_profile()
    bool profiling = false;
    struct ev_pair { hipEvent_t a, b; int kind; };
    std::vector<ev_pair> events;
    // diagnostic (experiments builds, C12381_PAIR_STAMPS): per-task time stamps of the last queue pairing launch, on this context's device
    unsigned long long* stamps = nullptr;
    size_t stamps_tasks = 0;
    // ... followed by 12 words per wavefront of the grid (pair_queue.hpp queue_wave_stats) for the last queue launch of pairings, Miller loops or
    // final exponentiations; c12381_sync() writes both regions to the file
    static constexpr size_t STAMP_WAVES = 4096;
    // launch counter of the work-queue kernels whose state travels in tagged words (pair_queue.hpp stw_store): 28 bits, never 0
    uint32_t queue_epoch = 0;
};

namespace c12381_host __attribute__((visibility("hidden"))) {
using namespace c12381;

// Tuning and diagnostic switches exist only in builds with -DC12381_EXPERIMENTS (crypto12381_amd/lib/libc12381_hip_exp.so: tools/, A/B
// runs, tests/test_gpu_variants.py).  The default library reads NO environment variable and contains neither the superseded
// one-lane pairing kernels nor the forced-failure hooks: a stray variable in a caller's environment cannot select another path.
// tuning_env is getenv in an experiments build and null otherwise (c12381_hip.hip, one of the two host units that look at the define).
const char* tuning_env(const char* name);
extern int g_queue_groups_host;                 // experiments builds: C12381_QUEUE_GROUPS (c12381_hip.hip): the override of the queue's split, api_pair.hip pair_queue_setup; a device copy for gt3_pow_queue_kernel alone
extern const size_t MSM_MAX_TERMS;              // terms per bucket-method pass (c12381_hip.hip)
bool fixed_base_enabled();                      // C12381_FIXED_BASE=0 switches the table-driven routes off (c12381_hip.hip)
int pair_lanes();                               // 3; C12381_PAIR_LANES=1: the one-lane-per-pairing kernels (api_pair.hip)

inline int fail(c12381_ctx* c, hipError_t e, const char* what) {
    std::snprintf(c->err, sizeof c->err, "%s: %s", what, hipGetErrorString(e));
    return C12381_E_HIP;
}
#define HIPCK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((c), e_, #call); } while (0)

// c12381_hip.hip.  Every entry begins `int rc = bind(c) ?: x_args(...); if (rc || n == 0) return rc;` — the argument condition of an entry is
// written once, in its x_args function, and both forms of the entry check it before anything else (a ?: b is a when a is not 0).
int bind(c12381_ctx* c);
int ensure(c12381_ctx* c, int slot, size_t bytes);
inline unsigned grid_for(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }
inline int other_red(int slot) { return slot == c12381_ctx::WS_RED0 ? c12381_ctx::WS_RED1 : c12381_ctx::WS_RED0; }      // the ping-pong of the reduction slots
inline bool g1_fmt(int fmt) { return fmt == 49 || fmt == 96; }
inline bool g2_fmt(int fmt) { return fmt == 97 || fmt == 192; }

// Launch.  LAUNCH: one thread per lane in blocks of BLOCK on the context's stream; LAUNCH_ON: the sites that differ (side stream, 2-D grid,
// 64-thread blocks, a grid counted in blocks for the queue kernels).  Like HIPCK, both return from the calling function when the launch failed.
#define LAUNCH_ON(c, kernel, grid, block, stream, ...) \
    do { hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__); HIPCK(c, hipGetLastError()); } while (0)
#define LAUNCH(c, kernel, lanes, ...) LAUNCH_ON(c, kernel, dim3(grid_for(lanes)), dim3(BLOCK), (c)->stream, __VA_ARGS__)

// HIP-event bracket around a dominant-kernel launch (kind: 0 = g1_mul_kernel, 1 = g1_finish_kernel, ...)
struct timed {
    c12381_ctx* c; int idx = -1;
    timed(c12381_ctx* c_, int kind) : c(c_) {
        if (!c->profiling) return;
        c12381_ctx::ev_pair p; p.kind = kind;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
        (void)hipEventRecord(p.a, c->stream);
        c->events.push_back(p); idx = (int)c->events.size() - 1;
    }
    ~timed() { if (idx >= 0) (void)hipEventRecord(c->events[idx].b, c->stream); }
};

// Host form.  The caller's inputs and outputs, (host pointer, bytes) each, laid out in WS_STAGE at 256-byte-aligned offsets.  stage() copies
// every non-empty input in and hands back the device pointers (a null host pointer stays null); unstage() copies the outputs back after
// the _dev call and ends with read_flag.  Up to 12 inputs and 5 outputs.  host_form: stage, the entry's _dev form on s.in[] / s.out[], unstage.
struct host_buf { const void* p; size_t bytes; };
struct staging {
    const uint8_t* in[12] = {};
    uint8_t* out[5] = {};
    host_buf host_out[5] = {};
    size_t nout = 0;
};
int stage(c12381_ctx* c, staging& s, std::initializer_list<host_buf> ins, std::initializer_list<host_buf> outs);       // c12381_hip.hip
int unstage(c12381_ctx* c, const staging& s);
int read_flag(c12381_ctx* c);
template <class Dev>
int host_form(c12381_ctx* c, std::initializer_list<host_buf> ins, std::initializer_list<host_buf> outs, Dev dev) {
    staging s;
    int rc;
    if ((rc = stage(c, s, ins, outs)) || (rc = dev(s))) return rc;
    return unstage(c, s);
}

// ---------------------------------------------------------------- c12381_hip.hip: G1, G2, Zp pieces the protocol units are built from
// WS_PROJ for `lanes` projective points of G1 (3 NL dwords each; g2: 6 NL) as an SoA of stride round_up(lanes, 64)
struct proj_slab { size_t stride; int32_t* p; };
int proj_ws(c12381_ctx* c, size_t lanes, proj_slab& w, bool g2 = false);
int g1_mul_to_proj(c12381_ctx* c, size_t n, const uint8_t* d_pts, const uint8_t* d_sc, size_t stride, size_t pt_stride = 96, size_t proj_off = 0,
                   const int32_t* skip_if = nullptr, bool in_g1 = false);
int g1_finish(c12381_ctx* c, size_t n, const int32_t* proj, size_t stride, uint8_t* d_out, int fmt);
int g2_mul_dev_strided(c12381_ctx* c, size_t n, const uint8_t* pts, size_t pt_stride, const uint8_t* sc, uint8_t* out, int fmt, const int32_t* skip_if = nullptr,
                       bool finish = false, bool in_g2 = false, size_t proj_stride = 0, size_t proj_off = 0);
int g2_finish(c12381_ctx* c, size_t n, uint8_t* d_out, int fmt, size_t proj_stride = 0);
int zp_batch_inverse(c12381_ctx* c, size_t n, const uint8_t* x, const uint8_t* gamma, uint8_t* out);
using reduce_fn = void (*)(size_t, const int32_t*, size_t, size_t, int32_t*, size_t);
int tree_sum(c12381_ctx* c, reduce_fn reduce, size_t words, size_t n, const int32_t*& cur, size_t& stride);
// fork_side: what is queued on the side stream from here on starts after everything queued on the context's stream so far (ev_chunk[0]).
// join_side: the context's stream waits for what the side stream has been given (ev_side).  Every call that forks joins before it returns.
int fork_side(c12381_ctx* c);
int join_side(c12381_ctx* c);

// ---------------------------------------------------------------- device-built tables, kept across calls
// A table array: `count` tables `stride` dwords apart behind `gate` dwords (0 or GATE_DWORDS) in workspace `slot`, each a header and its entries
// built from one point of `point_bytes` bytes (fixed-base multiples, line coefficients: the header words are listed in k_fixed.hip).  A single
// table is an array of one.  cached_tables makes the first k tables current for the points pts.p[0 .. k): it grows the workspace and zeroes
// it when it grew, so that every table in it misses on first use, launches fixed_cache_check_kernel — the "same point as last time?"
// comparison runs on the device — and then the caller's build kernel, whose workgroups return at once where the cached table is current.
// k = 0 only provides the workspace.  Everything is queued on the stream, nothing waits for the host; a table lives until another point
// takes its place or c12381_trim frees the workspace.
struct table_array { int slot, count; size_t stride, gate; int point_bytes; };
struct cached { int32_t *gate, *tabs; int stride; };
constexpr size_t GATE_DWORDS = 128;
constexpr size_t table_dwords(size_t entries) { return (HDR_DWORDS + entries + 63) / 64 * 64; }
template <class Build>
int cached_tables(c12381_ctx* c, const table_array& a, int k, const table_points& pts, cached& t, Build build) {
    if (k < 0 || k > a.count || a.count > TABLE_ARRAY_MAX) return C12381_E_ARG;
    const size_t bytes = (a.gate + (size_t)a.count * a.stride) * 4;
    int rc;
    if (c->ws_bytes[a.slot] < bytes) {
        if ((rc = ensure(c, a.slot, bytes))) return rc;
        HIPCK(c, hipMemsetAsync(c->ws[a.slot], 0, bytes, c->stream));      // no magic yet: first use of every table is a miss
    }
    t.gate = (int32_t*)c->ws[a.slot];
    t.tabs = t.gate + a.gate;
    t.stride = (int)a.stride;
    if (k == 0) return 0;
    LAUNCH_ON(c, fixed_cache_check_kernel, dim3((unsigned)k), dim3(64), c->stream, pts, a.point_bytes, t.tabs, t.stride);
    return build(t);
}
// G1 multiples (c12381_hip.hip): the four slots that g1_mul_fixed (0), the BBS+ columns (h0, h_1, h_2, h_3) and bbs04 (u, v, h, g1) share, and
// slot 4 (PS_GEN_SLOT) for the default generator under PS sign alone.  g1_fixed_table makes the table of `slot` current for base96;
// g1_fixed_column: m products of one public base into proj[col_off, col_off + m) of WS_PROJ (stride `stride`), from that table where the base is a
// subgroup point, by the generic kernel otherwise — each of the two launches returns at once when the other one serves the column.  fb = false:
// the generic kernel alone.  g2_fixed_table: the one slot of g2_mul_fixed and BBS+.
constexpr int PS_GEN_SLOT = 4;
int g1_fixed_table(c12381_ctx* c, int slot, const uint8_t* base96);
int g2_fixed_table(c12381_ctx* c, const uint8_t* base192, cached& t);
int g1_fixed_column(c12381_ctx* c, size_t m, const uint8_t* base, int slot, const uint8_t* sc, size_t stride, size_t col_off, bool fb);
// The per-lane sum of c12381_g1_mul_fixed_sum_batch_dev over bases [first, first + nb) of a list of `total` (c12381_hip.hip): the tables of ALL
// `total` bases are made current at their positions, so sums over different parts of one key evict nothing.  sc: the nb columns of the range.
// Arguments are the caller's to check (1 <= nb, first + nb <= total <= C12381_G1_FIXED_SUM_MAX, n > 0).
int g1_fixed_sum_range(c12381_ctx* c, size_t n, size_t total, size_t first, size_t nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* sc,
                       uint8_t* out, int fmt);
// the same over G2 bases and the tables of c12381_g2_mul_fixed_sum_batch_dev (1 <= nb, first + nb <= total <= C12381_G2_FIXED_SUM_MAX)
int g2_fixed_sum_range(c12381_ctx* c, size_t n, size_t total, size_t first, size_t nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* sc,
                       uint8_t* out, int fmt);

// ---------------------------------------------------------------- api_ps.hip, api_ac_bbs.hip: pieces the credential units share
// The body of c12381_ps_verify_batch_dev on checked arguments (n > 0) with an X2 that may be ABSENT (null):
// ok[j] = [ e(s1_j, sum_i m[i*n + j] Y2_i) == e(s2_j, g2) ], the product of the fast route then has nmsg + 1 factors.
int ps_verify_core(c12381_ctx* c, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192, const uint8_t* s1_96,
                   const uint8_t* s2_96, const uint8_t* m_32, uint8_t* ok);
// out[j] = a96[j] + b96[j], one complete addition per lane (api_ac_bbs.hip)
int ac_bbs_add(c12381_ctx* c, size_t m, const uint8_t* a96, const uint8_t* b96, uint8_t* out, int fmt);

// ---------------------------------------------------------------- api_pair.hip: line tables and the pairing launches the protocols share
// Line tables of the k points q.p[j] (coefficients of a fixed G2 argument of the Miller loop, pairing3.hpp) and the gate over the k, in the
// array of the K-way products (TA_FQ_K).  rule: bit 0 need_g2, bit 1 raw records (k_pairk.hip g2_lines_tables_kernel); a table is also rebuilt
// when its rule changes.  g2_key_cols: the columns g2, X2, Y2_0 .. of a PS key.
int lines_tables_k(c12381_ctx* c, int k, const g2_cols& q, int rule, cached& t);
g2_cols g2_key_cols(const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192, size_t nmsg);
// BBS+'s two line tables — w and g2, both have to be elements of G2 — and the gate over them; verification and the aggregate form share them
int bbs_lines_tables(c12381_ctx* c, const uint8_t* w_192, const uint8_t* g2_192, cached& t);
int launch_pair_eq(c12381_ctx* c, size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, size_t b2_stride, uint8_t* ok,
                   const int32_t* skip_if = nullptr);
// The prep kernel (G1 columns -> records, skipped when prep_skip says so) and the K-way queue kernel: GT output (eq = false; gate[HDR_VALID]
// = 0 poisons every lane) or the boolean (eq = true; runs only when gate[HDR_VALID] != 0).
int launch_prodk(c12381_ctx* c, size_t n, int k, const g1_cols& cols, uint32_t neg_mask, const cached& t, uint8_t* out, bool eq, bool miller_only,
                 const int32_t* prep_skip);
// ok[j] = [ e(a_j, w) e(b_j, g2) == 1 ] over BBS+'s two line tables (bbs_lines_tables), runs only when gate[HDR_VALID] != 0
int launch_prod_fixed(c12381_ctx* c, size_t n, const uint8_t* a_96, const uint8_t* b_96, const cached& lines, uint8_t* ok, const int32_t* gate);
void pair_stamps_dump(c12381_ctx* c);

}  // namespace c12381_host
