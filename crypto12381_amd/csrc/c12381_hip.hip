// Context, workspaces and the core of the C ABI of the batched BLS12-381 backend for MI355X (gfx950): context life cycle, streams, profile, Fp, G1,
// G2, MSM, fixed-base tables and per-lane sums, decoding, hash-to-G1 and Zp entries, and the definitions of the helpers host.hpp declares for the
// protocol units (api_pair.hip, api_ps.hip, api_bbs.hip, api_bbs04.hip).  Public interface and reference citations: include/c12381_hip.h.
// Kernels: kernels.hpp (k_*.hip).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <new>
#include <thread>

#include "host.hpp"
#include "fp.hpp"
#include "g1.hpp"
#include "g2.hpp"
#include "msm.hpp"
#include "fixed_base.hpp"
#ifdef C12381_EXPERIMENTS
#include "fp_raw_ops.hpp"
#endif

using namespace c12381;
using namespace c12381_host;

namespace {
// the unsorted value of entry x of a window segment, as the bucket product's sort reads it through its input iterator (msm_entry_value)
struct msm_value_fn { uint32_t n; __host__ __device__ uint32_t operator()(uint32_t x) const { return msm_entry_value(x, n); } };
}  // namespace

namespace c12381_host __attribute__((visibility("hidden"))) {
#ifdef C12381_EXPERIMENTS
const char* tuning_env(const char* name) { return std::getenv(name); }
#else
const char* tuning_env(const char*) { return nullptr; }
#endif
int g_queue_groups_host = 0;
constexpr int FLAG_WORDS = 4;                    // device status words (read_flag)
// elements per scalar-mul launch, in machine rounds (one round = the lanes resident at the kernel's occupancy: 256 CUs x 4 SIMDs x
// 64 lanes x waves per SIMD).  EIGHT rounds per launch, not one: a SIMD serves its oldest wavefront first and the younger one only
// fills its stalls (csrc/microbench/issue_mix.hip), so in a launch of exactly the resident size the older workgroup of each CU runs at
// full speed, leaves, and the younger one then runs ALONE with every wait for its table records exposed (SQ_WAIT_ANY 12 % per
// wavefront: + 6 % on the launch).  With more rounds per launch the dispatcher puts a new workgroup beside the one that is left, and only
// the last round runs alone: G1 26.8 -> 25.8-26.1 ms per 2^20, G2 8.04 -> 7.66 ms per 2^17 (profiles/r03_ab_chunk_rounds.txt).
// Table slabs: 2816 B per lane — 2.95 GB for a full G1 launch of 2^20 points, 2.95 GB for a full G2 launch of 2^19 (two lanes per point);
// smaller batches allocate for their own size.
constexpr size_t CHUNK_ROUNDS = 8;
constexpr size_t G1_CHUNK = (size_t)65536 * G1_OCC * CHUNK_ROUNDS;
constexpr size_t G2_CHUNK = (size_t)32768 * G2H_OCC * CHUNK_ROUNDS;
// C12381_MSM_MAX_TERMS lowers the bound (2 * n * windows sort items < 2^31) so that tests reach the multi-part path with small inputs
const size_t MSM_MAX_TERMS = [] {
    const char* e = tuning_env("C12381_MSM_MAX_TERMS");
    const size_t v = e ? (size_t)std::strtoull(e, nullptr, 10) : 0;
    return v >= 64 && v < ((size_t)1 << 26) ? v : (size_t)1 << 26;
}();

int ensure(c12381_ctx* c, int slot, size_t bytes) {
    if (c->ws_bytes[slot] >= bytes) return 0;
    if (c->ws[slot]) { HIPCK(c, hipFree(c->ws[slot])); c->ws[slot] = nullptr; c->ws_bytes[slot] = 0; }
    hipError_t e = hipMalloc(&c->ws[slot], bytes);
    if (e != hipSuccess) { std::snprintf(c->err, sizeof c->err, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return C12381_E_NOMEM; }
    c->ws_bytes[slot] = bytes;
    return 0;
}
int bind(c12381_ctx* c) {
    if (!c) return C12381_E_ARG;
    HIPCK(c, hipSetDevice(c->device));
    return 0;
}
int proj_ws(c12381_ctx* c, size_t lanes, proj_slab& w, bool g2) {
    w.stride = round_up(lanes, 64);
    const int rc = ensure(c, c12381_ctx::WS_PROJ, (size_t)(g2 ? 6 : 3) * NL * w.stride * 4);
    w.p = (int32_t*)c->ws[c12381_ctx::WS_PROJ];
    return rc;
}

// scalar multiplication of n elements into the projective SoA workspace (stride = padded n)
// (results land at proj[proj_off + i]; pt_stride 96 = per-lane points, 0 = one broadcast point)
// in_g1: the caller asserts every point lies in G1 (C12381_F_IN_SUBGROUP): the [r]phi(P) terms of scalars below x^2 are then
// the point at infinity and the kernel skips them — a membership test as long as a scalar multiplication per such lane
int g1_mul_to_proj(c12381_ctx* c, size_t n, const uint8_t* d_pts, const uint8_t* d_sc, size_t stride, size_t pt_stride, size_t proj_off,
                   const int32_t* skip_if, bool in_g1) {
    const size_t chunk = n < G1_CHUNK ? round_up(n, 64) : G1_CHUNK;
    int rc;
    if ((rc = ensure(c, c12381_ctx::WS_TAB, (size_t)G1_TAB_DWORDS * chunk * 4))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_PROJ, (size_t)3 * NL * stride * 4))) return rc;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = n - off < chunk ? n - off : chunk;
        timed tm(c, 0);
        // small_term: the reference's [r]phi(P) for scalars below x^2, inside the kernel (k_g1.hip); in_g1 callers have none to add
        LAUNCH(c, g1_mul_kernel, m, m, d_pts + pt_stride * off, pt_stride, d_sc + 32 * off, (int32_t*)c->ws[c12381_ctx::WS_TAB], (int32_t*)c->ws[c12381_ctx::WS_PROJ],
               stride, proj_off + off, c->d_flag, skip_if, in_g1 ? 0 : 1);
    }
    return 0;
}
// Lanes of the simultaneous inversion (g1_finish_kernel / g2_finish_kernel: lane t converts elements t, t + T, ...): one lane per element up
// to one machine round of single wavefronts (65 536 lanes), then up to FINISH_M elements per lane.  The kernels are latency-bound — an
// inversion is a chain of 28 K dependent instructions whatever the number of lanes running it — so idle SIMDs are cheaper than long lanes:
// 2^18 G2 elements at 16 per lane took 0.50 ms (a quarter wavefront per SIMD, 16 x 15 products behind each inversion).
static size_t finish_lanes(size_t n) {
    size_t per = (n + 65535) / 65536;
    if (per > (size_t)FINISH_M) per = FINISH_M;
    if (per < 1) per = 1;
    const size_t T = round_up((n + per - 1) / per, 64);
    return T > n ? n : T;
}
int g1_finish(c12381_ctx* c, size_t n, const int32_t* proj, size_t stride, uint8_t* d_out, int fmt) {
    int rc;
    if ((rc = ensure(c, c12381_ctx::WS_PREF, (size_t)NL * stride * 4))) return rc;
    const size_t T = finish_lanes(n);
    timed tm(c, 1);
    LAUNCH(c, g1_finish_kernel, T, n, proj, stride, (int32_t*)c->ws[c12381_ctx::WS_PREF], d_out, fmt, T);
    return 0;
}
// Status words raised by the kernels since the last read: [0] an input point was not on the curve (its outputs are 0xff),
// [1] a library-internal failure (a work-queue hand-over timed out: the affected outputs are 0xff as well), [2] a device-side argument
// check failed (bbs04 open: a gmsk scalar >= r, its status bytes are 0xff; PS sign: x or a used y_i >= r, its signatures are 0xff).  Every host
// entry point ends here, so a word raised by an earlier asynchronous _dev call is reported by the next host call or
// c12381_sync() on the same context, whichever comes first — _dev callers separate logical operations with c12381_sync().
int read_flag(c12381_ctx* c) {
    HIPCK(c, hipMemcpyAsync(c->h_flag, c->d_flag, FLAG_WORDS * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemsetAsync(c->d_flag, 0, FLAG_WORDS * sizeof(int), c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (c->h_flag[1]) {
        std::snprintf(c->err, sizeof c->err, "internal: a pairing work-queue hand-over timed out; the affected outputs are 0xff");
        return C12381_E_INTERNAL;
    }
    if (c->h_flag[2]) {
        std::snprintf(c->err, sizeof c->err, "a secret scalar is not below r (bbs04 open: gmsk; PS sign: x, y; MHAC-bbs iss: sk; AC issue: sk)");
        return C12381_E_ARG;
    }
    return c->h_flag[0] ? C12381_E_POINT : 0;
}
int stage(c12381_ctx* c, staging& s, std::initializer_list<host_buf> ins, std::initializer_list<host_buf> outs) {
    size_t bytes = 0;
    for (const host_buf& b : ins) bytes += b.p ? round_up(b.bytes, 256) : 0;
    for (const host_buf& b : outs) bytes += round_up(b.bytes, 256);
    int rc;
    if ((rc = ensure(c, c12381_ctx::WS_STAGE, bytes))) return rc;
    uint8_t* d = (uint8_t*)c->ws[c12381_ctx::WS_STAGE];
    size_t i = 0;
    for (const host_buf& b : ins) {
        s.in[i++] = b.p ? d : nullptr;
        if (!b.p) continue;
        if (b.bytes) HIPCK(c, hipMemcpyAsync(d, b.p, b.bytes, hipMemcpyHostToDevice, c->stream));
        d += round_up(b.bytes, 256);
    }
    for (const host_buf& b : outs) {
        s.out[s.nout] = d; s.host_out[s.nout++] = b;
        d += round_up(b.bytes, 256);
    }
    return 0;
}
int unstage(c12381_ctx* c, const staging& s) {
    for (size_t i = 0; i < s.nout; ++i)
        if (s.host_out[i].bytes) HIPCK(c, hipMemcpyAsync(const_cast<void*>(s.host_out[i].p), s.out[i], s.host_out[i].bytes, hipMemcpyDeviceToHost, c->stream));
    return read_flag(c);
}
// Projective tree sum of the n elements at `cur` (SoA with stride `stride`, `words` dwords per element: 3 NL for G1, 6 NL for G2) by the
// reduce kernel, ping-pong between WS_RED0 and WS_RED1: levels of round_up(n / 32, 64) elements above 4096, of 64 above 64, then 1.
// cur / stride end at the single projective result.
int tree_sum(c12381_ctx* c, reduce_fn reduce, size_t words, size_t n, const int32_t*& cur, size_t& stride) {
    int slot = c12381_ctx::WS_RED0, rc;
    for (size_t cur_n = n; cur_n > 1;) {
        const size_t m = cur_n > 4096 ? round_up(cur_n / 32, 64) : (cur_n > 64 ? 64 : 1);
        const size_t m_stride = round_up(m, 64);
        if ((rc = ensure(c, slot, words * m_stride * 4))) return rc;
        LAUNCH(c, reduce, m, cur_n, cur, stride, m, (int32_t*)c->ws[slot], m_stride);
        cur = (const int32_t*)c->ws[slot]; cur_n = m; stride = m_stride;
        slot = other_red(slot);
    }
    return 0;
}
int fork_side(c12381_ctx* c) {
    if (c->ev_chunk.empty()) {
        hipEvent_t e;
        HIPCK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->ev_chunk.push_back(e);
    }
    HIPCK(c, hipEventRecord(c->ev_chunk[0], c->stream));
    HIPCK(c, hipStreamWaitEvent(c->side, c->ev_chunk[0], 0));
    return 0;
}
int join_side(c12381_ctx* c) {
    HIPCK(c, hipEventRecord(c->ev_side, c->side));
    HIPCK(c, hipStreamWaitEvent(c->stream, c->ev_side, 0));
    return 0;
}
// Fixed-base table arrays (host.hpp "device-built tables"): the G1 slots, the slot of g2_mul_fixed, BBS+ and bbs04, and the nb tables of the
// per-lane sums in G1 and in G2
static_assert(FB_HEADER_DWORDS == HDR_DWORDS, "every table: header in front of the entries");
static_assert(G1_FIXED_SUM_MAX <= TABLE_ARRAY_MAX && G2_FIXED_SUM_MAX <= TABLE_ARRAY_MAX, "table_points holds the points of the largest array");
constexpr size_t FB_G1_ENTRIES = (size_t)FB_G1_WINDOWS * FB_ENTRIES, FB_G2_ENTRIES = (size_t)FB_G2_WINDOWS * FB_ENTRIES;
constexpr table_array fb_g1_slot(int i) { return {c12381_ctx::WS_FB_G1_0 + i, 1, table_dwords(FB_G1_ENTRIES * FB_G1_DWORDS), 0, 96}; }
static_assert(c12381_ctx::WS_FB_G1_0 + PS_GEN_SLOT == c12381_ctx::WS_FB_G1_4, "the fixed-base slots are consecutive workspaces");
constexpr table_array TA_FB_G1_SUM = {c12381_ctx::WS_FB_G1_SUM, G1_FIXED_SUM_MAX, table_dwords(FB_G1_ENTRIES * FB_G1_DWORDS), GATE_DWORDS, 96};
constexpr table_array TA_FB_G2 = {c12381_ctx::WS_FB_G2, 1, table_dwords(FB_G2_ENTRIES * FB_G2_DWORDS), 0, 192};
constexpr table_array TA_FB_G2_SUM = {c12381_ctx::WS_FB_G2_SUM, G2_FIXED_SUM_MAX, table_dwords(FB_G2_ENTRIES * FB_G2_DWORDS), GATE_DWORDS, 192};
// the fixed-base tables of nb points of G (fixed_base.hpp: fb_g1, fb_g2) POINT_BYTES apart
struct host_g1 : fb_g1 { static constexpr auto tables_kernel = g1_fixed_tables_kernel; };
struct host_g2 : fb_g2 { static constexpr auto tables_kernel = g2_fixed_tables_kernel; };
template <class G>
int fixed_tables(c12381_ctx* c, const table_array& a, int nb, const uint8_t* bases, cached& t) {
    table_points pts = {};
    for (int i = 0; i < nb; ++i) pts.p[i] = bases + G::POINT_BYTES * i;
    return cached_tables(c, a, nb, pts, t, [&](const cached& b) {
        LAUNCH_ON(c, G::tables_kernel, dim3(grid_for((size_t)G::WINDOWS * FB_ENTRIES), (unsigned)nb), dim3(BLOCK), c->stream, bases, b.tabs, b.stride);
        return 0;
    });
}
int g1_fixed_table(c12381_ctx* c, int slot, const uint8_t* base96) {
    cached t;
    return fixed_tables<host_g1>(c, fb_g1_slot(slot), 1, base96, t);
}
int g2_fixed_table(c12381_ctx* c, const uint8_t* base192, cached& t) { return fixed_tables<host_g2>(c, TA_FB_G2, 1, base192, t); }
bool fixed_base_enabled() {
    static const bool on = [] { const char* e = tuning_env("C12381_FIXED_BASE"); return !(e && e[0] == '0'); }();
    return on;
}
int g1_fixed_column(c12381_ctx* c, size_t m, const uint8_t* base, int slot, const uint8_t* sc, size_t stride, size_t col_off, bool fb) {
    const int32_t* skip = nullptr;
    if (fb) {
        skip = (const int32_t*)c->ws[c12381_ctx::WS_FB_G1_0 + slot];
        LAUNCH(c, g1_fixed_eval_kernel, m, m, skip, sc, (int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, col_off);
    }
    return g1_mul_to_proj(c, m, base, sc, stride, 0, col_off, skip);
}
// window width: msm_window_bits(n), or C12381_MSM_C = 4..16 (tuning runs)
static int msm_c(size_t n) {
    static const int forced = [] { const char* e = tuning_env("C12381_MSM_C"); const int v = e ? std::atoi(e) : 0; return v >= 4 && v <= 16 ? v : 0; }();
    return forced ? forced : msm_window_bits(n);
}
constexpr int MSM_SORT_STREAMS = 2;      // streams the window segments are sorted on (>= 2: the context's and its side stream; three or four measure the same, profiles/r04_ab_msm_front2.txt)
static_assert(MSM_SORT_STREAMS >= 2 && MSM_SORT_STREAMS <= 8, "MSM_SORT_STREAMS");
// Bucket-method MSM (msm.hpp): prep -> radix sort -> bucket sums -> window reduction -> Horner -> affine.
int g1_msm_pippenger(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, int in_fmt = 96) {
    const int cb = msm_c(n), W = msm_windows(cb);
    // nbk digit buckets + ONE more (index nbk, key W << cb): the points whose scalar is below x^2 (msm.hpp)
    const size_t E = msm_entries(n, W), nb = (size_t)1 << cb, nbk = nb * W, nbx = nbk + 1;
    int rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_PTS, (size_t)2 * n * MSM_PT_STRIDE * 4))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_K0, E * 4))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_K1, E * 4))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_V0, E * 4))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_V1, E * 4))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_RNG, (nbx + 1) * 8))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_MSM_BK, nbx * G1_ENT_DWORDS * 4))) return rc;
    int32_t* pts2 = (int32_t*)c->ws[c12381_ctx::WS_MSM_PTS];
    uint32_t *k0 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_K0], *k1 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_K1];
    uint32_t *v0 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_V0], *v1 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_V1];
    uint32_t* lo = (uint32_t*)c->ws[c12381_ctx::WS_MSM_RNG];
    uint32_t* hi = lo + nbx + 1;
    int32_t* bk = (int32_t*)c->ws[c12381_ctx::WS_MSM_BK];
    // Sort by digit inside every window segment (msm_prep_one lays the entries out window by window): bits [0, cb) only — two
    // 8-bit passes for cb = 16.  rocPRIM's radix sort is called directly.  From 2^15 terms on: once per segment, on 16-BIT keys (the digit
    // alone: the window is the position) and with the unsorted values supplied by an iterator (msm_entry_value: they are positional too) —
    // round 4: 6 instead of 8 bytes read and written per entry and pass, no value array written by the preparation.  Below that: one
    // call over all entries with the window bits in 32-bit keys (a handful of launches instead of 3 per segment).
    const bool per_window = n >= ((size_t)1 << 15) && cb <= 16;
    if (per_window) {
        uint16_t *q0 = (uint16_t*)k0, *q1 = (uint16_t*)k1;
        LAUNCH(c, msm_prep16_kernel, n, n, pts, in_fmt, sc, cb, W, pts2, q0, c->d_flag);
        auto vin = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), msm_value_fn{(uint32_t)n});
        size_t tmp_bytes = 0, tb = 0;
        HIPCK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, q0, q1, vin, v1, 2 * n, 0, cb, c->stream));
        HIPCK(c, rocprim::radix_sort_pairs(nullptr, tb, q0, q1, vin, v1, n, 0, 1, c->stream));
        if (tb > tmp_bytes) tmp_bytes = tb;
        // The segments are sorted alternately on the context's stream and on the side stream (own temporary storage each): one sort is
        // six small launches around two passes that reach 1.7 TB/s, two at a time fill the gaps and the memory system better.
        const size_t tmp_half = round_up(tmp_bytes + 256, 256);
        if ((rc = ensure(c, c12381_ctx::WS_MSM_TMP, MSM_SORT_STREAMS * tmp_half))) return rc;
        uint8_t* tmp = (uint8_t*)c->ws[c12381_ctx::WS_MSM_TMP];
        while ((int)c->sort_streams.size() < MSM_SORT_STREAMS - 2) {       // beyond the context's stream and its side stream
            hipStream_t st; hipEvent_t e;
            HIPCK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            c->sort_streams.push_back(st);
            HIPCK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c->sort_events.push_back(e);
        }
        auto sort_stream = [&](int k) { return k == 0 ? c->stream : (k == 1 ? c->side : c->sort_streams[(size_t)k - 2]); };
        if ((rc = fork_side(c))) return rc;                                // the keys are written
        for (int k = 2; k < MSM_SORT_STREAMS; ++k) HIPCK(c, hipStreamWaitEvent(sort_stream(k), c->ev_chunk[0], 0));
        for (int w = 0; w <= W; ++w) {                                     // segment W: the small-scalar entries, one key bit
            const size_t off = (size_t)2 * w * n;
            size_t sz = tmp_bytes;
            const int k = w % MSM_SORT_STREAMS;
            HIPCK(c, rocprim::radix_sort_pairs(tmp + (size_t)k * tmp_half, sz, q0 + off, q1 + off, vin, v1 + off, w < W ? 2 * n : n, 0, w < W ? cb : 1, sort_stream(k)));
        }
        if ((rc = join_side(c))) return rc;
        for (int k = 2; k < MSM_SORT_STREAMS; ++k) {
            HIPCK(c, hipEventRecord(c->sort_events[(size_t)k - 2], sort_stream(k)));
            HIPCK(c, hipStreamWaitEvent(c->stream, c->sort_events[(size_t)k - 2], 0));
        }
        HIPCK(c, hipMemsetAsync(lo, 0, (nbx + 1) * 8, c->stream));
        LAUNCH_ON(c, msm_ranges16_kernel, dim3(grid_for((2 * n + MSM_RANGES_PER_THREAD - 1) / MSM_RANGES_PER_THREAD), W + 1), dim3(BLOCK), c->stream, n,
                  (const uint16_t*)q1, cb, W, lo, hi);
    } else {
        LAUNCH(c, msm_prep_kernel, n, n, pts, in_fmt, sc, cb, W, pts2, k0, v0, c->d_flag);
        size_t tmp_bytes = 0;
        int end_bit = cb;
        while ((1 << (end_bit - cb)) <= W) ++end_bit;              // keys < (W + 1) << cb
        HIPCK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, k0, k1, v0, v1, E, 0, end_bit, c->stream));
        if ((rc = ensure(c, c12381_ctx::WS_MSM_TMP, tmp_bytes + 256))) return rc;
        size_t sz = tmp_bytes;
        HIPCK(c, rocprim::radix_sort_pairs(c->ws[c12381_ctx::WS_MSM_TMP], sz, k0, k1, v0, v1, E, 0, end_bit, c->stream));
        HIPCK(c, hipMemsetAsync(lo, 0, (nbx + 1) * 8, c->stream));
        LAUNCH(c, msm_ranges_kernel, E, E, k1, cb, W, lo, hi);
    }
    // buckets in order of decreasing run length (k0 / v0 are free again after the first sort; the sorted size keys go
    // to k1, which the ranges kernel has finished with)
    const size_t key_cap = E > nbx ? E : nbx;
    if (key_cap > E) {
        if ((rc = ensure(c, c12381_ctx::WS_MSM_K0, key_cap * 4))) return rc;
        if ((rc = ensure(c, c12381_ctx::WS_MSM_K1, key_cap * 4))) return rc;
        if ((rc = ensure(c, c12381_ctx::WS_MSM_V0, key_cap * 4))) return rc;
        k0 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_K0]; k1 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_K1]; v0 = (uint32_t*)c->ws[c12381_ctx::WS_MSM_V0];
    }
    if ((rc = ensure(c, c12381_ctx::WS_MSM_ORD, nbx * 4))) return rc;
    uint32_t* order = (uint32_t*)c->ws[c12381_ctx::WS_MSM_ORD];
    // overflow bookkeeping for runs longer than MSM_RUN_CAP (k_g1.hip): counters | segment list | cut-bucket list | partial sums
    const uint32_t run_cap = msm_run_cap(n, cb);
    const size_t ovf_cap = E / (run_cap / 2) + 1;
    const size_t o_seg = 256, o_big = o_seg + round_up(ovf_cap * 8, 256), o_part = o_big + round_up(ovf_cap * 16, 256);
    if ((rc = ensure(c, c12381_ctx::WS_MSM_OVF, o_part + ovf_cap * G1_ENT_DWORDS * 4))) return rc;
    uint8_t* ovf = (uint8_t*)c->ws[c12381_ctx::WS_MSM_OVF];
    uint32_t* ovf_cnt = (uint32_t*)ovf;
    uint2* ovf_seg = (uint2*)(ovf + o_seg);
    uint4* ovf_big = (uint4*)(ovf + o_big);
    int32_t* ovf_part = (int32_t*)(ovf + o_part);
    HIPCK(c, hipMemsetAsync(ovf_cnt, 0, 16, c->stream));
    // The small-scalar bucket (index nbk) and the [r]phi(S) it owes, on the side stream while this one goes on to the bucket sums: ranges and
    // sorted values are final here.  ovf_cnt[2] = "term written"; longer buckets are left to the bucket kernel and msm_small_term_kernel.
    int32_t* small_term = (int32_t*)(ovf + 64);
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, msm_small_early_kernel, dim3(1), dim3(64), c->side, (const uint32_t*)lo, (const uint32_t*)hi, (uint32_t)nbk, MSM_SMALL_EARLY_MAX,
              (const uint32_t*)v1, (const int32_t*)pts2, small_term, ovf_cnt + 2);
    LAUNCH(c, msm_sizes_kernel, nbx, nbx, lo, hi, k0, v0, run_cap, ovf_cnt, ovf_seg, ovf_big, MSM_SMALL_EARLY_MAX);
    {   // run-length keys are below 2^bits(cap): one or two passes instead of four
        int kb = 1;
        while (((uint32_t)1 << kb) <= run_cap) ++kb;
        size_t tmp2 = 0;
        HIPCK(c, rocprim::radix_sort_pairs(nullptr, tmp2, k0, k1, v0, order, nbx, 0, kb, c->stream));
        if ((rc = ensure(c, c12381_ctx::WS_MSM_TMP, tmp2 + 256))) return rc;
        HIPCK(c, rocprim::radix_sort_pairs(c->ws[c12381_ctx::WS_MSM_TMP], tmp2, k0, k1, v0, order, nbx, 0, kb, c->stream));
    }
    {
        timed tm(c, 5);
        LAUNCH(c, msm_bucket_kernel, nbx, nbx, lo, hi, v1, pts2, bk, order, run_cap, MSM_SMALL_EARLY_MAX);
    }
    // uniform scalars register no overflow segment: both grids leave after reading the counters
    LAUNCH(c, msm_overflow_kernel, ovf_cap, (const uint32_t*)ovf_cnt, (const uint2*)ovf_seg, lo, hi, v1, pts2, ovf_part, run_cap);
    LAUNCH_ON(c, msm_overflow_combine_kernel, dim3(ovf_cap < 4096 ? (unsigned)((ovf_cap + 3) / 4) : 1024u), dim3(BLOCK), c->stream, (const uint32_t*)ovf_cnt,
              (const uint4*)ovf_big, (const int32_t*)ovf_part, bk);
    // a small-scalar bucket too long for the early kernel: its term from the bucket sum, on the side stream beside the window reductions
    // (returns at once when the early kernel has written the term)
    if ((rc = fork_side(c))) return rc;
    LAUNCH_ON(c, msm_small_term_kernel, dim3(1), dim3(64), c->side, (const int32_t*)(bk + nbk * G1_ENT_DWORDS), small_term, (const uint32_t*)(ovf_cnt + 2));
    const uint32_t chunks = (uint32_t)((nb + MSM_CHUNK - 1) / MSM_CHUNK);
    size_t cur_n = (size_t)W * chunks, cur_stride = round_up(cur_n, 64);
    if ((rc = ensure(c, c12381_ctx::WS_RED0, (size_t)3 * NL * cur_stride * 4))) return rc;
    LAUNCH(c, msm_wreduce_kernel, cur_n, W, (uint32_t)nb, chunks, bk, (int32_t*)c->ws[c12381_ctx::WS_RED0], cur_stride);
    // per-window sums: element index = chunk * W + w; every level folds 64 points of a window per wavefront
    const int32_t* cur = (const int32_t*)c->ws[c12381_ctx::WS_RED0];
    int slot = c12381_ctx::WS_RED1;
    while (cur_n > (size_t)W) {
        const size_t groups = cur_n / W, out_groups = (groups + 63) / 64;
        const size_t m = (size_t)W * out_groups, m_stride = round_up(m, 64);
        if ((rc = ensure(c, slot, (size_t)3 * NL * m_stride * 4))) return rc;
        LAUNCH(c, g1_wave_reduce_kernel, m * 64, groups, W, cur, cur_stride, (int32_t*)c->ws[slot], m_stride);
        cur = (const int32_t*)c->ws[slot]; cur_n = m; cur_stride = m_stride;
        slot = other_red(slot);
    }
    proj_slab w;
    if ((rc = proj_ws(c, 1, w))) return rc;
    if ((rc = join_side(c))) return rc;                                    // the small-scalar term is written
    LAUNCH_ON(c, msm_horner_kernel, dim3(1), dim3(64), c->stream, cur, cur_stride, W, cb, w.p, w.stride, (const int32_t*)small_term);
    return g1_finish(c, 1, w.p, w.stride, out, fmt);
}
// C12381_MSM=naive forces the n-scalar-muls + tree-sum path (A/B measurements); default: buckets from 2 terms on (both
// paths equal the reference's chain of multiply() calls for every input; the bucket path is the faster one at every size)
static bool msm_use_buckets(size_t n) {
    static const int mode = [] { const char* e = tuning_env("C12381_MSM"); return e ? (e[0] == 'n' ? 1 : (e[0] == 'b' ? 2 : 0)) : 0; }();
    if (mode == 1) return false;
    return n >= 2;
}
}  // namespace c12381_host

int c12381_version(void) { return (0 << 16) | 6; }

int c12381_create(int device, c12381_ctx** out) {
    if (!out) return C12381_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return C12381_E_HIP;
    c12381_ctx* c = new (std::nothrow) c12381_ctx;
    if (!c) return C12381_E_NOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return C12381_E_HIP; }
    c->own_stream = true;
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming) != hipSuccess) { c12381_destroy(c); return C12381_E_HIP; }
    if (hipMalloc((void**)&c->d_flag, FLAG_WORDS * sizeof(int)) != hipSuccess || hipHostMalloc((void**)&c->h_flag, FLAG_WORDS * sizeof(int)) != hipSuccess ||
        hipMemset(c->d_flag, 0, FLAG_WORDS * sizeof(int)) != hipSuccess) { c12381_destroy(c); return C12381_E_HIP; }
    if (const char* e = tuning_env("C12381_QUEUE_GROUPS")) { g_queue_groups_host = std::atoi(e); set_queue_groups_override(g_queue_groups_host); }      // tuning runs only; the device copy: gt3_pow_queue_kernel
    *out = c;
    return 0;
}

void c12381_destroy(c12381_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->events) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (int i = 0; i < c12381_ctx::WS_COUNT; ++i) if (c->ws[i]) (void)hipFree(c->ws[i]);
    if (c->stamps) (void)hipFree(c->stamps);
    if (c->d_flag) (void)hipFree(c->d_flag);
    if (c->h_flag) (void)hipHostFree(c->h_flag);
    for (hipStream_t st : c->sort_streams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipEvent_t e : c->sort_events) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->side) (void)hipStreamDestroy(c->side);
    for (hipEvent_t e : c->ev_chunk) (void)hipEventDestroy(e);
    if (c->ev_side) (void)hipEventDestroy(c->ev_side);
    delete c;
}

const char* c12381_last_error(const c12381_ctx* c) { return c ? c->err : "null context"; }

// Workspaces grow to the largest call a context has served and stay (a GT power of 2^16 elements leaves 1.4 GB of tables, 2^18 BBS+ verifications
// a 344 MB state slab, a 2^20 scalar multiplication its 2.95 GB table slab): a long-lived context that has finished with the large batches hands
// them back here; the next call allocates what it needs again.
int c12381_trim(c12381_ctx* c) {
    int rc = bind(c); if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (c->side) HIPCK(c, hipStreamSynchronize(c->side));
    for (hipStream_t st : c->sort_streams) HIPCK(c, hipStreamSynchronize(st));
    for (int i = 0; i < c12381_ctx::WS_COUNT; ++i) {
        if (!c->ws[i]) continue;
        // cached tables whose headers say "valid" live in some of these slots: freeing them only costs a rebuild on the next call that needs them
        HIPCK(c, hipFree(c->ws[i]));
        c->ws[i] = nullptr; c->ws_bytes[i] = 0;
    }
    return 0;
}

int c12381_set_stream(c12381_ctx* c, void* hip_stream) {
    int rc = bind(c); if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream) { HIPCK(c, hipStreamDestroy(c->stream)); c->own_stream = false; }
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; }
    else { HIPCK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    return 0;
}

int c12381_sync(c12381_ctx* c) {
    int rc = bind(c); if (rc) return rc;
    rc = read_flag(c);
    pair_stamps_dump(c);
    return rc;
}

// Ordering against the caller's other streams without blocking the host (include/c12381_hip.h "Stream ordering").  Side-stream work of
// earlier calls is always joined back into the context's stream by the call that started it (ev_side), so the context's stream alone
// carries the completion of everything launched so far.
int c12381_wait_event(c12381_ctx* c, void* hip_event) {
    int rc = bind(c); if (rc) return rc;
    if (!hip_event) return C12381_E_ARG;
    HIPCK(c, hipStreamWaitEvent(c->stream, (hipEvent_t)hip_event, 0));
    return 0;
}
int c12381_record_event(c12381_ctx* c, void* hip_event) {
    int rc = bind(c); if (rc) return rc;
    if (!hip_event) return C12381_E_ARG;
    HIPCK(c, hipEventRecord((hipEvent_t)hip_event, c->stream));
    return 0;
}

#ifdef C12381_EXPERIMENTS
// experiments builds only (not declared in include/c12381_hip.h): start the clock probe on a stream of its own; `out` = 2 n device words
extern "C" int c12381_exp_clock_probe(c12381_ctx* c, unsigned long long* out, int n, int gap) {
    int rc = bind(c); if (rc) return rc;
    if (!out || n <= 0 || gap < 0) return C12381_E_ARG;
    static hipStream_t probe_stream = nullptr;          // its own stream: G1 / MSM work waits for the context's side stream
    if (!probe_stream) HIPCK(c, hipStreamCreateWithFlags(&probe_stream, hipStreamNonBlocking));
    LAUNCH_ON(c, clock_probe_kernel, dim3(1), dim3(BLOCK), probe_stream, out, n, gap);
    return 0;
}
#endif
int c12381_profile(c12381_ctx* c, int enable) {
    int rc = bind(c); if (rc) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (auto& p : c->events) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    c->events.clear();
    c->profiling = enable != 0;
    return 0;
}
int c12381_profile_read(c12381_ctx* c, int kind, double* total_ms, uint64_t* launches) {
    int rc = bind(c); if (rc) return rc;
    if (!total_ms || !launches) return C12381_E_ARG;
    HIPCK(c, hipStreamSynchronize(c->stream));
    double ms = 0; uint64_t cnt = 0;
    for (auto& p : c->events) {
        if (p.kind != kind) continue;
        float t = 0;
        HIPCK(c, hipEventElapsedTime(&t, p.a, p.b));
        ms += t; ++cnt;
    }
    *total_ms = ms; *launches = cnt;
    return 0;
}

// ---------------------------------------------------------------- Fp
static int fp_op_args(int op, const void* a, const void* b, const void* out) { return (op < 0 || op > 5 || !a || !out || (op <= 2 && !b)) ? C12381_E_ARG : 0; }
int c12381_fp_op_batch_dev(c12381_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c) ?: fp_op_args(op, a, b, out);
    if (rc || n == 0) return rc;
    LAUNCH(c, fp_op_kernel, n, op, n, a, op <= 2 ? b : nullptr, out);
    return 0;
}
int c12381_fp_op_batch(c12381_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c) ?: fp_op_args(op, a, b, out);
    if (rc || n == 0) return rc;
    return host_form(c, {{a, 48 * n}, {op <= 2 ? b : nullptr, 48 * n}}, {{out, 48 * n}},
                     [&](const staging& s) { return c12381_fp_op_batch_dev(c, op, n, s.in[0], s.in[1], s.out[0]); });
}
int c12381_fp_mulchain_dev(c12381_ctx* c, size_t n, int iters, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c); if (rc) return rc;
    if (!a || !b || !out || iters < 0) return C12381_E_ARG;
    if (n == 0) return 0;
    LAUNCH(c, fp_mulchain_kernel, n, n, iters, a, b, out);
    return 0;
}

#ifdef C12381_EXPERIMENTS
// experiments builds only (not declared in include/c12381_hip.h): the raw-limb test kernel of the Fp / Fp2 leaf (k_fp_raw.hip, fp_raw_ops.hpp).
// Host buffers: in = n x arity x 14 limbs, k = n x 4 integers, out = n x outputs x 14 limbs; arity / outputs are the op's (C12381_E_ARG otherwise).
// The op decides the kernel: the whole-element codes run one lane per element, the FH2_* codes two (fp2h_raw_kernel).
extern "C" int c12381_exp_fp_raw_batch(c12381_ctx* c, int op, size_t n, int arity, int outputs, const int32_t* in, const int32_t* k, int32_t* out) {
    int rc = bind(c); if (rc) return rc;
    if (!fp_raw_is_op(op) || arity != fp_raw_arity(op) || outputs != fp_raw_outputs(op) || !in || !k || !out) return C12381_E_ARG;
    if (n == 0) return 0;
    staging s;
    const size_t in_bytes = (arity ? (size_t)arity : 1) * NL * sizeof(int32_t) * n;
    if ((rc = stage(c, s, {{in, in_bytes}, {k, FR_MAX_K * sizeof(int32_t) * n}}, {{out, (size_t)outputs * NL * sizeof(int32_t) * n}}))) return rc;
    if (fp_raw_is_two_lane(op)) LAUNCH(c, fp2h_raw_kernel, 2 * n, op, n, (const int32_t*)s.in[0], (const int32_t*)s.in[1], (int32_t*)s.out[0]);
    else LAUNCH(c, fp_raw_kernel, n, op, n, (const int32_t*)s.in[0], (const int32_t*)s.in[1], (int32_t*)s.out[0]);
    return unstage(c, s);
}
#endif

// ---------------------------------------------------------------- G1
// C12381_F_COMPRESSED_IN: pts are n x 49 bytes (the serialized form, g1_point.hpp:87-111 -> ECP_fromOctet): from_bytes -> multiply ->
// to_bytes in ONE kernel — the square root runs in the kernel's prologue; a rejected encoding is a lane of 0xff + C12381_E_POINT
// (also the check of the fixed-base forms, with flags 0)
static int g1_mul_args(const void* pts, const void* sc, const void* out, int fmt, unsigned flags) {
    return (!pts || !sc || !out || !g1_fmt(fmt) || (flags & ~(unsigned)(C12381_F_IN_SUBGROUP | C12381_F_COMPRESSED_IN))) ? C12381_E_ARG : 0;
}
int c12381_g1_mul_batch_flags_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g1_mul_args(pts, sc, out, fmt, flags);
    if (rc || n == 0) return rc;
    const size_t stride = round_up(n, 64);
    if ((rc = g1_mul_to_proj(c, n, pts, sc, stride, (flags & C12381_F_COMPRESSED_IN) ? 49 : 96, 0, nullptr, (flags & C12381_F_IN_SUBGROUP) != 0))) return rc;
    return g1_finish(c, n, (const int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, out, fmt);
}
int c12381_g1_mul_batch_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    return c12381_g1_mul_batch_flags_dev(c, n, pts, sc, out, fmt, 0u);
}
int c12381_g1_mul_batch_flags(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g1_mul_args(pts, sc, out, fmt, flags);
    if (rc || n == 0) return rc;
    return host_form(c, {{pts, ((flags & C12381_F_COMPRESSED_IN) ? 49 : 96) * n}, {sc, 32 * n}}, {{out, (size_t)fmt * n}},
                     [&](const staging& s) { return c12381_g1_mul_batch_flags_dev(c, n, s.in[0], s.in[1], s.out[0], fmt, flags); });
}
int c12381_g1_mul_batch(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    return c12381_g1_mul_batch_flags(c, n, pts, sc, out, fmt, 0u);
}
// Per-lane sums of k products under one doubling chain (k_g1sum.hip).  One term is g1_mul_kernel itself, so k = 1 returns the bytes of
// c12381_g1_mul_batch_flags.  The table workspace is k records per lane: a launch covers CHUNK_ROUNDS / k machine rounds (4, 2, 2 for
// k = 2, 3, 4 — 524 288, 262 144, 262 144 lanes), so the slab of a 2^20 batch is 2.95, 2.21, 2.95 GB: never more than g1_mul_to_proj's.
// C12381_F_COMPRESSED_IN is refused: the loop re-reads the inputs of an exceptional lane and must not repeat k square roots there.
static int g1_mul_sum_args(size_t n, int k, const void* pts, const void* sc, const void* out, int fmt, unsigned flags) {
    static_assert(C12381_G1_MUL_SUM_MAX == G1_MUL_SUM_MAX, "C12381_G1_MUL_SUM_MAX");
    return (k < 1 || k > C12381_G1_MUL_SUM_MAX || !g1_fmt(fmt) || (flags & ~(unsigned)C12381_F_IN_SUBGROUP) || (n && (!pts || !sc || !out))) ? C12381_E_ARG : 0;
}
int c12381_g1_mul_sum_batch_dev(c12381_ctx* c, size_t n, int k, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g1_mul_sum_args(n, k, pts, sc, out, fmt, flags);
    if (rc || n == 0) return rc;
    if (k == 1) return c12381_g1_mul_batch_flags_dev(c, n, pts, sc, out, fmt, flags);
    proj_slab w;
    if ((rc = proj_ws(c, n, w))) return rc;
    const size_t full = (size_t)65536 * G1_OCC * (CHUNK_ROUNDS / (size_t)k);
    const size_t chunk = n < full ? w.stride : full;
    if ((rc = ensure(c, c12381_ctx::WS_TAB, (size_t)k * G1_TAB_DWORDS * chunk * 4))) return rc;
    auto kernel = k == 2 ? g1_mul_sum2_kernel : (k == 3 ? g1_mul_sum3_kernel : g1_mul_sum4_kernel);
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = n - off < chunk ? n - off : chunk;
        timed tm(c, 0);
        LAUNCH(c, kernel, m, m, pts + 96 * off, sc + 32 * off, n, (int32_t*)c->ws[c12381_ctx::WS_TAB], w.p, w.stride, off, c->d_flag,
               (flags & C12381_F_IN_SUBGROUP) ? 0 : 1);
    }
    return g1_finish(c, n, w.p, w.stride, out, fmt);
}
int c12381_g1_mul_sum_batch(c12381_ctx* c, size_t n, int k, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g1_mul_sum_args(n, k, pts, sc, out, fmt, flags);
    if (rc || n == 0) return rc;
    return host_form(c, {{pts, 96 * n * (size_t)k}, {sc, 32 * n * (size_t)k}}, {{out, (size_t)fmt * n}},
                     [&](const staging& s) { return c12381_g1_mul_sum_batch_dev(c, n, k, s.in[0], s.in[1], s.out[0], fmt, flags); });
}
static int g1_add_dev(c12381_ctx* c, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, int fmt) {
    proj_slab w;
    int rc;
    if ((rc = proj_ws(c, n, w))) return rc;
    LAUNCH(c, g1_add_kernel, n, n, a, b, w.p, w.stride, c->d_flag);
    return g1_finish(c, n, w.p, w.stride, out, fmt);
}
int c12381_g1_add_batch(c12381_ctx* c, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, int fmt) {
    int rc = bind(c); if (rc) return rc;
    if (!a || !b || !out || !g1_fmt(fmt)) return C12381_E_ARG;
    if (n == 0) return 0;
    return host_form(c, {{a, 96 * n}, {b, 96 * n}}, {{out, (size_t)fmt * n}}, [&](const staging& s) { return g1_add_dev(c, n, s.in[0], s.in[1], s.out[0], fmt); });
}

// MSM: the bucket method (g1_msm_pippenger); a single term (or C12381_MSM=naive) takes n independent GLV scalar
// multiplications followed by a tree sum of the projective results (the reference's Π is also n full scalar-muls,
// g1_point.hpp:389-401).  Both equal the reference's chain for every input.  Only the final point is canonical.
// out = sum of n affine points (no scalars): the header's product over G1Point values (a chain of add(point1&, point1&),
// src/miracl_core_interface.cpp:129-132 -> ECP_add) and the combine step of a product that was sharded over GPUs:
// lift + tree sum + one affine conversion — tens of microseconds for the 8 partial points of a node, where the bucket method's
// fixed stages cost 2.3 ms.
static int g1_sum_args(size_t n, const void* pts, const void* out, int fmt) { return (!out || (n && !pts) || !g1_fmt(fmt)) ? C12381_E_ARG : 0; }
int c12381_g1_sum_dev(c12381_ctx* c, size_t n, const uint8_t* pts, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_sum_args(n, pts, out, fmt);
    if (rc) return rc;
    if (n == 0) { HIPCK(c, hipMemsetAsync(out, 0, fmt, c->stream)); return 0; }
    proj_slab w;
    if ((rc = proj_ws(c, n, w))) return rc;
    LAUNCH(c, g1_lift_kernel, n, n, pts, w.p, w.stride, c->d_flag);
    const int32_t* cur = w.p;
    size_t stride = w.stride;
    if ((rc = tree_sum(c, g1_reduce_kernel, 3 * NL, n, cur, stride))) return rc;
    return g1_finish(c, 1, cur, stride, out, fmt);
}
int c12381_g1_sum(c12381_ctx* c, size_t n, const uint8_t* pts, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_sum_args(n, pts, out, fmt);
    if (rc) return rc;
    return host_form(c, {{pts, 96 * n}}, {{out, (size_t)fmt}}, [&](const staging& s) { return c12381_g1_sum_dev(c, n, s.in[0], s.out[0], fmt); });
}
// (also the check of c12381_g1_sum_of_products, with flags 0)
static int g1_msm_args(size_t n, const void* pts, const void* sc, const void* out, int fmt, unsigned flags) {
    return (!out || (n && (!pts || !sc)) || !g1_fmt(fmt) || (flags & ~(unsigned)C12381_F_COMPRESSED_IN)) ? C12381_E_ARG : 0;
}
int c12381_g1_msm_flags_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g1_msm_args(n, pts, sc, out, fmt, flags);
    if (rc) return rc;
    const int in_fmt = (flags & C12381_F_COMPRESSED_IN) ? 49 : 96;        // compressed terms are decoded by the preparation kernel
    if (n == 0) { HIPCK(c, hipMemsetAsync(out, 0, fmt, c->stream)); return 0; }
    if (n > MSM_MAX_TERMS) {
        // the sort works on 32-bit item counts and (term, half) values: larger products are cut into parts whose
        // partial points (affine, WS_BBS_B as a small staging slot) are summed by c12381_g1_sum_dev
        const size_t parts = (n + MSM_MAX_TERMS - 1) / MSM_MAX_TERMS;
        if ((rc = ensure(c, c12381_ctx::WS_BBS_B, round_up(parts * 96, 256)))) return rc;
        uint8_t* pp = (uint8_t*)c->ws[c12381_ctx::WS_BBS_B];
        for (size_t p = 0; p < parts; ++p) {
            const size_t lo = p * MSM_MAX_TERMS, m = n - lo < MSM_MAX_TERMS ? n - lo : MSM_MAX_TERMS;
            if ((rc = g1_msm_pippenger(c, m, pts + (size_t)in_fmt * lo, sc + 32 * lo, pp + 96 * p, 96, in_fmt))) return rc;
        }
        return c12381_g1_sum_dev(c, parts, pp, out, fmt);
    }
    if (msm_use_buckets(n)) return g1_msm_pippenger(c, n, pts, sc, out, fmt, in_fmt);
    size_t stride = round_up(n, 64);
    if ((rc = g1_mul_to_proj(c, n, pts, sc, stride, (size_t)in_fmt))) return rc;
    const int32_t* cur = (const int32_t*)c->ws[c12381_ctx::WS_PROJ];
    if ((rc = tree_sum(c, g1_reduce_kernel, 3 * NL, n, cur, stride))) return rc;
    return g1_finish(c, 1, cur, stride, out, fmt);
}
int c12381_g1_msm_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    return c12381_g1_msm_flags_dev(c, n, pts, sc, out, fmt, 0u);
}
int c12381_g1_msm_flags(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g1_msm_args(n, pts, sc, out, fmt, flags);
    if (rc) return rc;
    return host_form(c, {{pts, ((flags & C12381_F_COMPRESSED_IN) ? 49 : 96) * n}, {sc, 32 * n}}, {{out, (size_t)fmt}},
                     [&](const staging& s) { return c12381_g1_msm_flags_dev(c, n, s.in[0], s.in[1], s.out[0], fmt, flags); });
}
int c12381_g1_msm(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    return c12381_g1_msm_flags(c, n, pts, sc, out, fmt, 0u);
}
// sum_of_products(point1&, int n, point1*, const big*) exactly as the boundary defines it (-> ECP_muln, a plain Pippenger): the sum
// of the TRUE multiples [k_i mod r]P_i for any curve points.  On G1 it equals c12381_g1_msm — use that for throughput; this entry
// exists so that the seam function has the reference's value for every input (n plain ladders + tree sum; the seam is scalar).
int c12381_g1_sum_of_products_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_msm_args(n, pts, sc, out, fmt, 0u);
    if (rc) return rc;
    if (n == 0) { HIPCK(c, hipMemsetAsync(out, 0, fmt, c->stream)); return 0; }
    proj_slab w;
    if ((rc = proj_ws(c, n, w))) return rc;
    LAUNCH(c, g1_mul_plain_kernel, n, n, pts, sc, w.p, w.stride, c->d_flag);
    const int32_t* cur = w.p;
    size_t stride = w.stride;
    if ((rc = tree_sum(c, g1_reduce_kernel, 3 * NL, n, cur, stride))) return rc;
    return g1_finish(c, 1, cur, stride, out, fmt);
}
int c12381_g1_sum_of_products(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_msm_args(n, pts, sc, out, fmt, 0u);
    if (rc) return rc;
    return host_form(c, {{pts, 96 * n}, {sc, 32 * n}}, {{out, (size_t)fmt}},
                     [&](const staging& s) { return c12381_g1_sum_of_products_dev(c, n, s.in[0], s.in[1], s.out[0], fmt); });
}
// One host process driving several GPUs: terms are split contiguously over the contexts, every
// context runs its local MSM on its own device from its own host thread, and the partial points (96 B each) are
// summed on the first context — the elliptic-curve "all-reduce" has no RCCL reduction op, the payload is ngpu x 96 B.
// (One process per GPU with torch.distributed does the same through an all-gather: crypto12381_amd/distributed.py.)
int c12381_g1_msm_multi(c12381_ctx** ctxs, int ngpu, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    if (!ctxs || ngpu <= 0 || g1_msm_args(n, pts, sc, out, fmt, 0u)) return C12381_E_ARG;
    for (int g = 0; g < ngpu; ++g) if (!ctxs[g]) return C12381_E_ARG;
    if (ngpu == 1) return c12381_g1_msm(ctxs[0], n, pts, sc, out, fmt);
    std::vector<uint8_t> partial((size_t)96 * ngpu, 0);
    std::vector<int> rcs(ngpu, 0);
    std::vector<std::thread> th;
    for (int g = 0; g < ngpu; ++g) {
        const size_t lo = n * (size_t)g / (size_t)ngpu, hi = n * (size_t)(g + 1) / (size_t)ngpu;
        th.emplace_back([=, &partial, &rcs] { rcs[g] = c12381_g1_msm(ctxs[g], hi - lo, pts + 96 * lo, sc + 32 * lo, &partial[(size_t)96 * g], 96); });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < ngpu; ++g) if (rcs[g]) return rcs[g];
    return c12381_g1_sum(ctxs[0], (size_t)ngpu, partial.data(), out, fmt);
}

// ---------------------------------------------------------------- G2
// finish = true: the kernel leaves projective results in WS_PROJ (the caller has sized it: 6 NL x round_up(n, 64) dwords)
// and g2_finish converts them with one inversion per FINISH_M elements; false: per-lane conversion straight to `out`.
// proj_stride / proj_off (finish = true): the results go to proj[proj_off + i] of an SoA with that stride; 0 = round_up(n, 64), the batch
// entry points' own layout.  g2_finish reads elements [0, n) of the same SoA.
int c12381_host::g2_finish(c12381_ctx* c, size_t n, uint8_t* d_out, int fmt, size_t proj_stride) {
    int rc;
    const size_t stride = proj_stride ? proj_stride : round_up(n, 64);
    if ((rc = ensure(c, c12381_ctx::WS_PREF, (size_t)2 * NL * stride * 4))) return rc;
    const size_t T = finish_lanes(n);
    LAUNCH(c, g2_finish_kernel, T, n, (const int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, (int32_t*)c->ws[c12381_ctx::WS_PREF], d_out, fmt, T);
    return 0;
}
// C12381_F_COMPRESSED_IN: pts are n x 97 bytes (g2_point.hpp:73-77 -> ECP2_fromOctet), decoded in the kernel's prologue
// (also the check of the fixed-base form, with flags 0)
static int g2_mul_args(const void* pts, const void* sc, const void* out, int fmt, unsigned flags) {
    return (!pts || !sc || !out || !g2_fmt(fmt) || (flags & ~(unsigned)(C12381_F_IN_SUBGROUP | C12381_F_COMPRESSED_IN))) ? C12381_E_ARG : 0;
}
int c12381_g2_mul_batch_flags_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g2_mul_args(pts, sc, out, fmt, flags);
    if (rc || n == 0) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_PROJ, (size_t)6 * NL * round_up(n, 64) * 4))) return rc;
    if ((rc = g2_mul_dev_strided(c, n, pts, (flags & C12381_F_COMPRESSED_IN) ? 97 : 192, sc, out, fmt, nullptr, true, (flags & C12381_F_IN_SUBGROUP) != 0))) return rc;
    return g2_finish(c, n, out, fmt);
}
int c12381_g2_mul_batch_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    return c12381_g2_mul_batch_flags_dev(c, n, pts, sc, out, fmt, 0u);
}
int c12381_host::g2_mul_dev_strided(c12381_ctx* c, size_t n, const uint8_t* pts, size_t pt_stride, const uint8_t* sc, uint8_t* out, int fmt,
                                    const int32_t* skip_if, bool finish, bool in_g2, size_t proj_stride, size_t proj_off) {
    int rc;
    if (!proj_stride) proj_stride = round_up(n, 64);
    const size_t chunk = n < G2_CHUNK ? round_up(n, 64) : G2_CHUNK;
    // C12381_G2_LANES=1 keeps the one-lane-per-point kernel for the batch entry points (A/B measurements); default:
    // two lanes per point (k_g2h.hip), whose per-lane table records are those of G1 (2 x 1408 B per point)
    static const bool two_lanes = [] { const char* e = tuning_env("C12381_G2_LANES"); return !(e && e[0] == '1'); }();
    const bool pairwise = finish && two_lanes;
    if ((rc = ensure(c, c12381_ctx::WS_TAB, (size_t)(pairwise ? 2 * G2_TAB * G1_ENT_DWORDS : G2_TAB_DWORDS) * chunk * 4))) return rc;
    int32_t* proj = finish ? (int32_t*)c->ws[c12381_ctx::WS_PROJ] : nullptr;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = n - off < chunk ? n - off : chunk;
        timed tm(c, 2);
        if (pairwise) {
            LAUNCH(c, g2_mul2_kernel, 2 * m, m, pts + pt_stride * off, pt_stride, sc + 32 * off, (int32_t*)c->ws[c12381_ctx::WS_TAB], c->d_flag, skip_if, proj,
                   proj_stride, proj_off + off, in_g2 ? 1 : 0);
            continue;
        }
        LAUNCH(c, g2_mul_kernel, m, m, pts + pt_stride * off, pt_stride, sc + 32 * off, (int32_t*)c->ws[c12381_ctx::WS_TAB], chunk, out + (size_t)fmt * off, fmt,
               c->d_flag, skip_if, proj, proj_stride, proj_off + off, in_g2 ? 1 : 0);
    }
    return 0;
}
int c12381_g2_mul_batch_flags(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt, unsigned flags) {
    int rc = bind(c) ?: g2_mul_args(pts, sc, out, fmt, flags);
    if (rc || n == 0) return rc;
    return host_form(c, {{pts, ((flags & C12381_F_COMPRESSED_IN) ? 97 : 192) * n}, {sc, 32 * n}}, {{out, (size_t)fmt * n}},
                     [&](const staging& s) { return c12381_g2_mul_batch_flags_dev(c, n, s.in[0], s.in[1], s.out[0], fmt, flags); });
}
int c12381_g2_mul_batch(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    return c12381_g2_mul_batch_flags(c, n, pts, sc, out, fmt, 0u);
}
// Π q_i^{x_i} in G2 (scalars == NULL: the plain product of the points, g2_point.hpp:225-236).  The reference evaluates it as n
// multiply(point2&, big) calls and a chain of add(point2&, point2&); here: the batched scalar multiplication into the
// projective workspace, then a tree sum (two levels), one affine conversion.  Only the final point is canonical.
static int g2_msm_args(size_t n, const void* pts, const void* out, int fmt) { return (!out || (n && !pts) || !g2_fmt(fmt)) ? C12381_E_ARG : 0; }
int c12381_g2_msm_dev(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g2_msm_args(n, pts, out, fmt);
    if (rc) return rc;
    if (n == 0) { HIPCK(c, hipMemsetAsync(out, 0, fmt, c->stream)); return 0; }
    size_t stride = round_up(n, 64);
    if ((rc = ensure(c, c12381_ctx::WS_PROJ, (size_t)6 * NL * stride * 4))) return rc;
    if (sc) {
        if ((rc = g2_mul_dev_strided(c, n, pts, 192, sc, out, fmt, nullptr, true))) return rc;
    } else {
        LAUNCH(c, g2_lift_kernel, n, n, pts, (int32_t*)c->ws[c12381_ctx::WS_PROJ], stride, c->d_flag);
    }
    const int32_t* cur = (const int32_t*)c->ws[c12381_ctx::WS_PROJ];
    if ((rc = tree_sum(c, g2_reduce_kernel, 6 * NL, n, cur, stride))) return rc;
    if ((rc = ensure(c, c12381_ctx::WS_PREF, (size_t)2 * NL * 64 * 4))) return rc;
    LAUNCH_ON(c, g2_finish_kernel, dim3(1), dim3(BLOCK), c->stream, (size_t)1, cur, stride, (int32_t*)c->ws[c12381_ctx::WS_PREF], out, fmt, (size_t)1);
    return 0;
}
int c12381_g2_msm(c12381_ctx* c, size_t n, const uint8_t* pts, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g2_msm_args(n, pts, out, fmt);
    if (rc) return rc;
    return host_form(c, {{pts, 192 * n}, {sc, 32 * n}}, {{out, (size_t)fmt}},
                     [&](const staging& s) { return c12381_g2_msm_dev(c, n, s.in[0], s.in[1], s.out[0], fmt); });
}
static int g2_add_dev(c12381_ctx* c, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, int fmt) {
    LAUNCH(c, g2_add_kernel, n, n, a, (size_t)192, b, out, fmt, c->d_flag, (const int32_t*)nullptr);
    return 0;
}
int c12381_g2_add_batch(c12381_ctx* c, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, int fmt) {
    int rc = bind(c); if (rc) return rc;
    if (!a || !b || !out || !g2_fmt(fmt)) return C12381_E_ARG;
    if (n == 0) return 0;
    return host_form(c, {{a, 192 * n}, {b, 192 * n}}, {{out, (size_t)fmt * n}}, [&](const staging& s) { return g2_add_dev(c, n, s.in[0], s.in[1], s.out[0], fmt); });
}
// ---------------------------------------------------------------- decode / split pairing / GT
static int decompress_args(const void* in, const void* out, const void* status) { return (!in || !out || !status) ? C12381_E_ARG : 0; }
int c12381_g1_decompress_batch_dev(c12381_ctx* c, size_t n, const uint8_t* in49, uint8_t* out96, uint8_t* status) {
    int rc = bind(c) ?: decompress_args(in49, out96, status);
    if (rc || n == 0) return rc;
    LAUNCH(c, g1_decompress_kernel, n, n, in49, out96, status, 0);
    return 0;
}
int c12381_g2_decompress_batch_dev(c12381_ctx* c, size_t n, const uint8_t* in97, uint8_t* out192, uint8_t* status) {
    int rc = bind(c) ?: decompress_args(in97, out192, status);
    if (rc || n == 0) return rc;
    LAUNCH(c, g2_decompress_kernel, n, n, in97, out192, status, 0);
    return 0;
}
int c12381_g1_decompress_batch(c12381_ctx* c, size_t n, const uint8_t* in49, uint8_t* out96, uint8_t* status) {
    int rc = bind(c) ?: decompress_args(in49, out96, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{in49, 49 * n}}, {{out96, 96 * n}, {status, n}},
                     [&](const staging& s) { return c12381_g1_decompress_batch_dev(c, n, s.in[0], s.out[0], s.out[1]); });
}
int c12381_g2_decompress_batch(c12381_ctx* c, size_t n, const uint8_t* in97, uint8_t* out192, uint8_t* status) {
    int rc = bind(c) ?: decompress_args(in97, out192, status);
    if (rc || n == 0) return rc;
    return host_form(c, {{in97, 97 * n}}, {{out192, 192 * n}, {status, n}},
                     [&](const staging& s) { return c12381_g2_decompress_batch_dev(c, n, s.in[0], s.out[0], s.out[1]); });
}
// ---------------------------------------------------------------- hash-to-G1, Zp helpers
// mode 0: 64-byte digests (hash to G1), 1: field elements (map to the curve), 2: points (cofactor clearing)
static int g1_map_dev(c12381_ctx* c, size_t n, const uint8_t* d_in, int mode, uint8_t* d_out, int fmt) {
    proj_slab w;
    int rc;
    if ((rc = proj_ws(c, n, w))) return rc;
    LAUNCH(c, g1_from_hash_kernel, n, n, d_in, mode, w.p, w.stride, c->d_flag);
    return g1_finish(c, n, w.p, w.stride, d_out, fmt);
}
static int g1_from_hash_args(const void* digests, const void* out, int fmt) { return (!digests || !out || !g1_fmt(fmt)) ? C12381_E_ARG : 0; }
int c12381_g1_from_hash_batch_dev(c12381_ctx* c, size_t n, const uint8_t* digests, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_from_hash_args(digests, out, fmt);
    if (rc || n == 0) return rc;
    return g1_map_dev(c, n, digests, 0, out, fmt);
}
int c12381_g1_from_hash_batch(c12381_ctx* c, size_t n, const uint8_t* digests, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_from_hash_args(digests, out, fmt);
    if (rc || n == 0) return rc;
    return host_form(c, {{digests, 64 * n}}, {{out, (size_t)fmt * n}}, [&](const staging& s) { return c12381_g1_from_hash_batch_dev(c, n, s.in[0], s.out[0], fmt); });
}
int c12381_g1_map_to_point_batch(c12381_ctx* c, size_t n, const uint8_t* u48, uint8_t* out96) {
    int rc = bind(c); if (rc) return rc;
    if (!u48 || !out96) return C12381_E_ARG;
    if (n == 0) return 0;
    return host_form(c, {{u48, 48 * n}}, {{out96, 96 * n}}, [&](const staging& s) { return g1_map_dev(c, n, s.in[0], 1, s.out[0], 96); });
}
int c12381_g1_clear_cofactor_batch(c12381_ctx* c, size_t n, const uint8_t* in96, uint8_t* out96) {
    int rc = bind(c); if (rc) return rc;
    if (!in96 || !out96) return C12381_E_ARG;
    if (n == 0) return 0;
    return host_form(c, {{in96, 96 * n}}, {{out96, 96 * n}}, [&](const staging& s) { return g1_map_dev(c, n, s.in[0], 2, s.out[0], 96); });
}
// out[i] = 1 / (x[i] + gamma) (gamma may be null), simultaneous inversion in runs of ZP_INV_RUN (k_hash_zp.hip)
int c12381_host::zp_batch_inverse(c12381_ctx* c, size_t n, const uint8_t* x, const uint8_t* gamma, uint8_t* out) {
    int rc;
    if ((rc = ensure(c, c12381_ctx::WS_PREF, 32 * n))) return rc;
    const size_t T = (n + ZP_INV_RUN - 1) / ZP_INV_RUN;
    LAUNCH(c, zp_batch_inv_kernel, T, n, T, x, gamma, out, (uint32_t*)c->ws[c12381_ctx::WS_PREF]);
    return 0;
}
static int zp_op_args(int op, const void* a, const void* b, const void* out) { return (op < 0 || op > 4 || !a || !out || (op <= 2 && !b)) ? C12381_E_ARG : 0; }
int c12381_zp_op_batch_dev(c12381_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c) ?: zp_op_args(op, a, b, out);
    if (rc || n == 0) return rc;
    if (op == 4) return zp_batch_inverse(c, n, a, nullptr, out);
    LAUNCH(c, zp_op_kernel, n, op, n, a, op <= 2 ? b : nullptr, out);
    return 0;
}
int c12381_zp_op_batch(c12381_ctx* c, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c) ?: zp_op_args(op, a, b, out);
    if (rc || n == 0) return rc;
    return host_form(c, {{a, 32 * n}, {op <= 2 ? b : nullptr, 32 * n}}, {{out, 32 * n}},
                     [&](const staging& s) { return c12381_zp_op_batch_dev(c, op, n, s.in[0], s.in[1], s.out[0]); });
}
static int zp_from_hash_dev(c12381_ctx* c, size_t n, const uint8_t* digests, uint8_t* out) {
    LAUNCH(c, zp_from_hash_kernel, n, n, digests, out);
    return 0;
}
int c12381_zp_from_hash_batch(c12381_ctx* c, size_t n, const uint8_t* digests, uint8_t* out) {
    int rc = bind(c); if (rc) return rc;
    if (!digests || !out) return C12381_E_ARG;
    if (n == 0) return 0;
    return host_form(c, {{digests, 64 * n}}, {{out, 32 * n}}, [&](const staging& s) { return zp_from_hash_dev(c, n, s.in[0], s.out[0]); });
}
static int zp_inner_product_args(size_t n, const void* a, const void* out) { return (!out || (n && !a)) ? C12381_E_ARG : 0; }
// strided partial sums, 64 terms per lane and stage, ping-pong between two reduction slots
int c12381_zp_inner_product_dev(c12381_ctx* c, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c) ?: zp_inner_product_args(n, a, out);
    if (rc) return rc;
    if (n == 0) { HIPCK(c, hipMemsetAsync(out, 0, 32, c->stream)); return 0; }
    const uint8_t *cur_a = a, *cur_b = b;
    size_t cur_n = n;
    int slot = c12381_ctx::WS_RED0;
    for (;;) {
        const size_t T = (cur_n + 63) / 64;
        uint8_t* dst = out;
        if (T > 1) {
            if ((rc = ensure(c, slot, round_up(32 * T, 256)))) return rc;
            dst = (uint8_t*)c->ws[slot];
        }
        LAUNCH(c, zp_fold_kernel, T, cur_n, cur_a, cur_b, T, dst);
        if (T == 1) return 0;
        cur_a = dst; cur_b = nullptr; cur_n = T;
        slot = other_red(slot);
    }
}
int c12381_zp_inner_product(c12381_ctx* c, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    int rc = bind(c) ?: zp_inner_product_args(n, a, out);
    if (rc) return rc;
    if (n == 0) { std::memset(out, 0, 32); return 0; }
    return host_form(c, {{a, 32 * n}, {b, 32 * n}}, {{out, 32}}, [&](const staging& s) { return c12381_zp_inner_product_dev(c, n, s.in[0], s.in[1], s.out[0]); });
}
// ---------------------------------------------------------------- one base for the whole batch (g^x_i)
int c12381_g1_mul_fixed_batch_dev(c12381_ctx* c, size_t n, const uint8_t* base96, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_mul_args(base96, sc, out, fmt, 0u);
    if (rc || n == 0) return rc;
    proj_slab w;
    if ((rc = proj_ws(c, n, w))) return rc;
    const bool fb = fixed_base_enabled();
    if (fb && (rc = g1_fixed_table(c, 0, base96))) return rc;
    if ((rc = g1_fixed_column(c, n, base96, 0, sc, w.stride, 0, fb))) return rc;
    return g1_finish(c, n, w.p, w.stride, out, fmt);
}
int c12381_g1_mul_fixed_batch(c12381_ctx* c, size_t n, const uint8_t* base96, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g1_mul_args(base96, sc, out, fmt, 0u);
    if (rc || n == 0) return rc;
    return host_form(c, {{base96, 96}, {sc, 32 * n}}, {{out, (size_t)fmt * n}},
                     [&](const staging& s) { return c12381_g1_mul_fixed_batch_dev(c, n, s.in[0], s.in[1], s.out[0], fmt); });
}
int c12381_g2_mul_fixed_batch_dev(c12381_ctx* c, size_t n, const uint8_t* base192, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g2_mul_args(base192, sc, out, fmt, 0u);
    if (rc || n == 0) return rc;
    const int32_t* skip = nullptr;
    const size_t stride = round_up(n, 64);
    if ((rc = ensure(c, c12381_ctx::WS_PROJ, (size_t)6 * NL * stride * 4))) return rc;
    if (fixed_base_enabled()) {
        cached t;
        if ((rc = g2_fixed_table(c, base192, t))) return rc;
        skip = t.tabs;
        LAUNCH(c, g2_fixed_eval_kernel, n, n, skip, sc, (const uint8_t*)nullptr, out, fmt, c->d_flag, (int32_t*)c->ws[c12381_ctx::WS_PROJ], stride);
    }
    if ((rc = g2_mul_dev_strided(c, n, base192, 0, sc, out, fmt, skip, true))) return rc;      // exactly one of the two kernels fills WS_PROJ
    return g2_finish(c, n, out, fmt);
}
int c12381_g2_mul_fixed_batch(c12381_ctx* c, size_t n, const uint8_t* base192, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: g2_mul_args(base192, sc, out, fmt, 0u);
    if (rc || n == 0) return rc;
    return host_form(c, {{base192, 192}, {sc, 32 * n}}, {{out, (size_t)fmt * n}},
                     [&](const staging& s) { return c12381_g2_mul_fixed_batch_dev(c, n, s.in[0], s.in[1], s.out[0], fmt); });
}
// ---------------------------------------------------------------- per-lane sums over a set of bases shared by the batch, in G1 and in G2
// out[j] = addend + sum_(i < nb) sc[i n + j] B_i.  G::SUM (TA_FB_G1_SUM, TA_FB_G2_SUM): a gate and G*_FIXED_SUM_MAX tables of the 4080 / 2040
// multiples of fixed_base.hpp, cached per position (changing one base rebuilds one table).
// One cache-check launch, one table launch and one gate launch whatever nb; then BOTH routes are queued and the gate lets one run:
//   every base a subgroup point   G::sum_kernel: all nb tables into one accumulator per lane
//   otherwise                     the columns through the generic kernel one by one (G::column: the kernels of c12381_g1_mul_batch /
//                                 c12381_g2_mul_batch), each into proj[half, half + n) and folded into proj[0, n) (two projective arrays
//                                 whatever nb), as bbs_message_points sums its columns
// The skipped route's kernels return at their first load.  Nothing waits for the host.  The route is written once (fixed_sum_dev,
// fixed_sum_host); sum_g1 / sum_g2 hold what differs between the groups and nothing else.
static_assert(C12381_G1_FIXED_SUM_MAX == G1_FIXED_SUM_MAX && C12381_G2_FIXED_SUM_MAX == G2_FIXED_SUM_MAX, "public and device bound of nb");
struct sum_g1 : host_g1 {
    static constexpr table_array SUM = TA_FB_G1_SUM;
    static constexpr size_t PROJ_DWORDS = 3 * NL;                     // of one projective point
    static constexpr auto gate_kernel = g1_fixed_sum_gate_kernel;
    static constexpr auto sum_kernel = g1_fixed_sum_kernel;
    static constexpr auto fold_kernel = g1_fixed_sum_fold_kernel;
    static bool fmt_ok(int fmt) { return g1_fmt(fmt); }
    static int column(c12381_ctx* c, size_t n, const uint8_t* base, const uint8_t* sc, uint8_t*, int, size_t stride, size_t col_off, const int32_t* gate) {
        return g1_mul_to_proj(c, n, base, sc, stride, 0, col_off, gate);
    }
    static int finish(c12381_ctx* c, size_t n, const int32_t* proj, size_t stride, uint8_t* out, int fmt) { return g1_finish(c, n, proj, stride, out, fmt); }
};
struct sum_g2 : host_g2 {
    static constexpr table_array SUM = TA_FB_G2_SUM;
    static constexpr size_t PROJ_DWORDS = 6 * NL;
    static constexpr auto gate_kernel = g2_fixed_sum_gate_kernel;
    static constexpr auto sum_kernel = g2_fixed_sum_kernel;
    static constexpr auto fold_kernel = g2_fixed_sum_fold_kernel;
    static bool fmt_ok(int fmt) { return g2_fmt(fmt); }
    static int column(c12381_ctx* c, size_t n, const uint8_t* base, const uint8_t* sc, uint8_t* out, int fmt, size_t stride, size_t col_off, const int32_t* gate) {
        return g2_mul_dev_strided(c, n, base, 0, sc, out, fmt, gate, true, false, stride, col_off);
    }
    static int finish(c12381_ctx* c, size_t n, const int32_t*, size_t stride, uint8_t* out, int fmt) { return g2_finish(c, n, out, fmt, stride); }
};
template <class G>
static int fixed_sum_args(size_t nb, const void* bases, const void* sc, const void* out, int fmt) {
    return (nb < 1 || nb > (size_t)G::SUM.count || !bases || !sc || !out || !G::fmt_ok(fmt)) ? C12381_E_ARG : 0;
}
// The sum over bases [first, first + nb) of a list of `total` bases whose tables ALL stay current at their positions (sc: the nb columns of the
// range); the public entries are total = nb, first = 0.  A protocol with several sums over parts of one key (api_ac_bbs.hip) keeps every table
// of the key cached this way.
template <class G>
static int fixed_sum_range(c12381_ctx* c, size_t n, size_t total, size_t first, size_t nb, const uint8_t* bases, const uint8_t* addend, const uint8_t* sc,
                           uint8_t* out, int fmt) {
    int rc;
    const bool fb = fixed_base_enabled();
    cached t;
    if ((rc = fixed_tables<G>(c, G::SUM, fb ? (int)total : 0, bases, t))) return rc;            // without tables: the gate buffer alone
    bases += G::POINT_BYTES * first;
    const int32_t *gate = t.gate, *tabs = t.tabs + first * (size_t)t.stride;
    const size_t half = round_up(n, 64), stride = 2 * half;       // proj[0, n): the sums; proj[half, half + n): the generic route's current column
    if ((rc = ensure(c, c12381_ctx::WS_PROJ, G::PROJ_DWORDS * stride * 4))) return rc;
    int32_t* proj = (int32_t*)c->ws[c12381_ctx::WS_PROJ];
    LAUNCH_ON(c, G::gate_kernel, dim3(1), dim3(64), c->stream, (int)nb, bases, addend, t.gate, tabs, t.stride, fb ? 1 : 0, c->d_flag);
    if (fb) {
        LAUNCH(c, G::sum_kernel, n, n, (int)nb, gate, tabs, t.stride, sc, addend, proj, stride);
    }
    for (size_t col = 0; col < nb; ++col) {
        if ((rc = G::column(c, n, bases + G::POINT_BYTES * col, sc + 32 * n * col, out, fmt, stride, col ? half : 0, gate))) return rc;
        if (col == 0 && nb > 1) continue;                          // the first column is written in place
        LAUNCH(c, G::fold_kernel, n, n, gate, proj, stride, half, col ? 1 : 0, col + 1 == nb ? 1 : 0, addend);
    }
    return G::finish(c, n, proj, stride, out, fmt);
}
template <class G>
static int fixed_sum_dev(c12381_ctx* c, size_t n, size_t nb, const uint8_t* bases, const uint8_t* addend, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: fixed_sum_args<G>(nb, bases, sc, out, fmt);
    if (rc || n == 0) return rc;
    return fixed_sum_range<G>(c, n, nb, 0, nb, bases, addend, sc, out, fmt);
}
namespace c12381_host __attribute__((visibility("hidden"))) {
int g1_fixed_sum_range(c12381_ctx* c, size_t n, size_t total, size_t first, size_t nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* sc,
                       uint8_t* out, int fmt) {
    return fixed_sum_range<sum_g1>(c, n, total, first, nb, bases96, addend96, sc, out, fmt);
}
int g2_fixed_sum_range(c12381_ctx* c, size_t n, size_t total, size_t first, size_t nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* sc,
                       uint8_t* out, int fmt) {
    return fixed_sum_range<sum_g2>(c, n, total, first, nb, bases192, addend192, sc, out, fmt);
}
}  // namespace c12381_host
template <class G>
static int fixed_sum_host(c12381_ctx* c, size_t n, size_t nb, const uint8_t* bases, const uint8_t* addend, const uint8_t* sc, uint8_t* out, int fmt) {
    int rc = bind(c) ?: fixed_sum_args<G>(nb, bases, sc, out, fmt);
    if (rc || n == 0) return rc;
    return host_form(c, {{bases, G::POINT_BYTES * nb}, {addend, (size_t)G::POINT_BYTES}, {sc, 32 * n * nb}}, {{out, (size_t)fmt * n}},
                     [&](const staging& s) { return fixed_sum_dev<G>(c, n, nb, s.in[0], s.in[1], s.in[2], s.out[0], fmt); });
}
int c12381_g1_mul_fixed_sum_batch_dev(c12381_ctx* c, size_t n, size_t nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* sc, uint8_t* out,
                                      int fmt) { return fixed_sum_dev<sum_g1>(c, n, nb, bases96, addend96, sc, out, fmt); }
int c12381_g1_mul_fixed_sum_batch(c12381_ctx* c, size_t n, size_t nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* sc, uint8_t* out, int fmt) {
    return fixed_sum_host<sum_g1>(c, n, nb, bases96, addend96, sc, out, fmt);
}
int c12381_g2_mul_fixed_sum_batch_dev(c12381_ctx* c, size_t n, size_t nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* sc, uint8_t* out,
                                      int fmt) { return fixed_sum_dev<sum_g2>(c, n, nb, bases192, addend192, sc, out, fmt); }
int c12381_g2_mul_fixed_sum_batch(c12381_ctx* c, size_t n, size_t nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* sc, uint8_t* out, int fmt) {
    return fixed_sum_host<sum_g2>(c, n, nb, bases192, addend192, sc, out, fmt);
}
