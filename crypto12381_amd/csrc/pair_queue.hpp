// The pairing work queue of k_pair3.hip and k_pairk.hip, stated once: the schedule, the lane / group / task arithmetic, the claim, the state
// of a queued group (tagged words; st_store / st_load of the GT power's plain 16-byte rows stay in k_pair3.hip) with its hand-over flags in
// both forms, relaxed and fenced, the six-step hand-over of the final exponentiation and the output of an element.
// Translation-unit-local (anonymous namespace): every function is
// inlined into the kernels that include it.  The five bodies (pair3_queue_body, split3_queue_body, pair3_fixed_queue_body,
// gt3_pow_queue_kernel, pairk_queue_body) keep their own control flow over these pieces.
//
// THE SCHEDULE.  A pairing is ~3.4 M instructions per wavefront and every wavefront task is equally long, so a plain grid finishes in whole
// "rounds": 3121 wavefronts (2^16 pairings) on 2048 resident slots take two full double rounds although they are 1.52 rounds of work.  A
// queue kernel is launched as a grid that just fills the machine and runs two loops:
//   whole groups first — wavefronts claim groups of 21 elements from counter[1] until `ndirect` of them are taken: no hand-over, no wait on
//     a slower partner, the state stays in registers and in the LDS slot.  ndirect is the host's number (host_layouts.hpp queue_direct_groups,
//     evaluated by api_pair.hip pair_queue_setup, which sizes the state slab from the same value; the GT power alone evaluates a transcription
//     of it in the kernel); 0 when the batch fits the grid;
//   then tasks — the remaining nq groups are cut into TASKS phases each (four quarters of the Miller loop, the six steps of the final
//     exponentiation f12t_final_exp_step; five for the GT power) and handed out through counter[0].  A wavefront that finishes takes the
//     next task, so the tail of the launch is a tenth as long: whole groups finish up to a group-time apart (the two wavefronts of a SIMD do
//     not share it evenly, profiles/r02_queue_phase_times.txt), ~5 small tasks per wavefront absorb that (2^16 pairings: 22.6 -> 20.4 ms).
// Tasks are numbered PHASE-MAJOR: task = p * nq + j is phase p of queued group ndirect + j, whose state lives in block j of the slab.  A task
// of phase p waits (spins on the group's flag) only for the task of phase p - 1 of its group, which has a smaller number, was therefore claimed
// earlier by a wavefront that is running, and never waits for anything of phase >= p: no cycle, every wavefront reaches the end of the queue.
// POISON.  The spin is bounded as a last line of defence (queue_wait*): a wavefront that gives up — or reads a state word that still carries
// another tag after the same bound — marks the group poisoned instead of running on stale state.  A poisoned task skips its arithmetic and
// passes the mark on (successors start at once), the last phase writes 0xff to every output of the group and raises bad_flag[1], which the host
// reports as C12381_E_INTERNAL — a library-internal failure never looks like valid output or like a bad input point.
#pragma once
#include "kernels_common.hpp"
#include "pairing3.hpp"

namespace {

using namespace c12381;

// Miller-loop tasks per group in the queue kernels (the 64 iterations in equal parts)
constexpr int MILLER_TASKS_PER_GROUP = 4;       // 2 and 8 measured: 2 loses 4 %, 8 is within the spread of 4 (profiles/r04_ab_queue_priority.txt, r05_ab_miller_variants.txt)
static_assert(64 % MILLER_TASKS_PER_GROUP == 0, "the Miller-loop tasks divide the 64 iterations");
constexpr int MILLER_ITERS_PER_TASK = 64 / MILLER_TASKS_PER_GROUP;

// lane -> its triple: lanes 3 j, 3 j + 1, 3 j + 2 hold coefficients a, b, c of element j; lane 63 idles along as a role-0 lane of its own
__device__ __forceinline__ tri tri_of_lane(unsigned lane) {
    const unsigned trip = lane / 3u;
    tri t;
    t.role = lane == 63u ? 0 : (int)(lane - 3u * trip);
    t.base = lane == 63u ? 63 : (int)(3u * trip);
    return t;
}
// The element of group g this lane works on: e = its index, i = the index it reads (inactive lanes — lane 63 and the lanes behind a ragged
// end — shadow the last element: same instruction stream), active = it writes its output.
struct queue_elem { size_t e, i; bool active; };
__device__ __forceinline__ queue_elem queue_elem_of(size_t g, unsigned lane, size_t n) {
    queue_elem q;
    q.e = g * TRI_PER_WAVE + (lane == 63u ? TRI_PER_WAVE - 1 : lane / 3u);
    q.active = lane < 63u && q.e < n;
    q.i = q.e < n ? q.e : n - 1;
    return q;
}
// Lane 0 claims the next number of a counter; readfirstlane makes it a scalar, so phase / group and every branch on them are wave-uniform
// for the compiler too (a broadcast by shuffle leaves them "divergent": the loop was then restructured per lane set, lanes 1..63 re-entered
// it with task 0 and never left).  Every lane issues the atomic, lanes 1..63 add zero: no divergent branch in front of the scalarisation.
__device__ __forceinline__ unsigned int queue_claim(unsigned int* counter, unsigned lane) {
    const unsigned int claimed = atomicAdd(counter, lane == 0 ? 1u : 0u);
    return (unsigned int)__builtin_amdgcn_readfirstlane((int)claimed);
}

__device__ __forceinline__ void gt_load_coeff(fp4& x, const uint8_t* p576, int role) {
    const uint8_t* p = p576 + (role == 0 ? 384 : (role == 1 ? 192 : 0));
    uint32_t raw[12];
    load_raw48(raw, p); fp_from_raw48(x.b.b, raw);
    load_raw48(raw, p + 48); fp_from_raw48(x.b.a, raw);
    load_raw48(raw, p + 96); fp_from_raw48(x.a.b, raw);
    load_raw48(raw, p + 144); fp_from_raw48(x.a.a, raw);
}
__device__ __forceinline__ void gt_store_coeff(uint8_t* o576, const fp4& x, int role) {
    uint8_t* o = o576 + (role == 0 ? 384 : (role == 1 ? 192 : 0));      // FP12_toOctet: c | b | a
    uint32_t raw[12];
    fp_to_raw48(raw, x.b.b); store_raw48(o, raw);
    fp_to_raw48(raw, x.b.a); store_raw48(o + 48, raw);
    fp_to_raw48(raw, x.a.b); store_raw48(o + 96, raw);
    fp_to_raw48(raw, x.a.a); store_raw48(o + 144, raw);
}

// ---- state of a queued group between two tasks, WITHOUT cache maintenance: every 32-bit word travels in an 8-byte word together with a 32-bit tag — launch epoch and
// the phase that wrote it; a reader that sees another tag in ANY word reads again.  The accesses are agent-scope coherent (sc1: write-through /
// read past this XCD's L2 — the eight XCDs' L2s are not coherent with each other for ordinary accesses: with an L1 invalidation alone the results
// were wrong, profiles/r05_ab_fence_free_handover.txt), and a word validates itself, so no release / acquire pair is needed: none of the
// buffer_wbl2 sc1 / buffer_inv sc1 the fences of the 16-byte form (GT power, k_pair3.hip st_store) cost per task — a write-back and an invalidation of the whole XCD's L2 under
// 256 resident wavefronts whose spills and private operands live there (tasks 5-7 % longer, the whole groups running beside them 2-3 %).
// Two tagged words per lane and instruction: buffer_load / buffer_store_dwordx4 with sc1 (as relaxed agent-scope ATOMIC 8-byte accesses —
// global_load / store_dwordx2 sc1 — the same traffic took ~600 cycles of issue per instruction, 65-105 K cycles per task to arrive and 20-48 K to
// leave: they are not coalesced).  An aligned 8-byte half of a lane's 16-byte access is never torn (one lane's 16 bytes move in one transaction),
// and tearing BETWEEN the halves is harmless, each carries its own tag.  Rows of 64 lanes x 16 bytes; one row per pair of 32-bit words.
constexpr int ST_DW_F = 56, ST_DW_TC = 28;                    // 32-bit words of an Fp4 / Fp2
constexpr int STW_F = 0, STW_TC1 = ST_DW_F / 2, STW_TC2 = STW_TC1 + ST_DW_TC / 2, STW_Y1 = STW_TC2 + ST_DW_TC / 2, STW_ROWS = STW_Y1 + ST_DW_F / 2;      // 84 rows of 1 KB
static_assert((size_t)STW_ROWS * 1024 == PAIR_QUEUE_STATE_BYTES, "kernels.hpp: size of a queued group's state block");
constexpr int STW_AUX = 16 | (int)0x80000000u;                // cache policy of the buffer instructions: sc1, volatile (never merged or hoisted)
typedef int32_t stw_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t st_tag(uint32_t epoch, unsigned int writer_phase) { return (epoch << 4) | (writer_phase + 1u); }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stw_rsrc(const void* rows) {          // rows: wave-uniform
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(rows), 0, 0x7fffffff, 0x00020000);
}
template <class T, int DW>
__device__ __forceinline__ void stw_store(void* rows, unsigned lane, const T& x, uint32_t tag) {
    static_assert(sizeof(T) == DW * 4 && DW % 2 == 0, "state word count");
    const int32_t* w = reinterpret_cast<const int32_t*>(&x);
    const __amdgpu_buffer_rsrc_t rs = stw_rsrc(rows);
#pragma unroll
    for (int r = 0; r < DW / 2; ++r) {
        stw_v4 v;
        v.x = w[2 * r]; v.y = (int32_t)tag; v.z = w[2 * r + 1]; v.w = (int32_t)tag;
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)((r * 64 + lane) * 16), 0, STW_AUX);
    }
}
// false: some word still carried another tag after spin_limit re-reads (the writer never finished): the caller poisons the group
template <class T, int DW>
__device__ __forceinline__ bool stw_load(T& x, const void* rows, unsigned lane, uint32_t tag, int spin_limit, unsigned int* reread = nullptr) {
    static_assert(sizeof(T) == DW * 4 && DW % 2 == 0, "state word count");
    int32_t* w = reinterpret_cast<int32_t*>(&x);
    const __amdgpu_buffer_rsrc_t rs = stw_rsrc(rows);
    int spins = 0;
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int r = 0; r < DW / 2; ++r) {
            const stw_v4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((r * 64 + lane) * 16), 0, STW_AUX);
            w[2 * r] = v.x; w[2 * r + 1] = v.z;
            ok = ok && (uint32_t)v.y == tag && (uint32_t)v.w == tag;
        }
        if (__builtin_amdgcn_ballot_w64(!ok) == 0) return true;           // wave-uniform
        if (reread) ++*reread;
        if (spin_limit < 0 || ++spins > spin_limit) return false;
        __builtin_amdgcn_s_sleep(64);
    }
}

// ---- hand-over flags.  flags[g] = number of finished phases of group g, bit 31 = the group is POISONED (the schedule, above).
// Publishing is an atomic max, so a predecessor that was merely slow cannot clear the mark afterwards.
// spin_limit < 0 (tests only, C12381_PAIR_SPIN_LIMIT): every wait is treated as timed out.
constexpr unsigned int Q_POISON = 0x80000000u;
// The fenced forms, for state in plain 16-byte rows (GT power): acquire / release around the data.
__device__ __forceinline__ bool queue_wait(unsigned int* flags, size_t g, unsigned int p, int spin_limit) {
    if (p == 0) return false;
    int spins = 0;
    for (;;) {
        const unsigned int v = (unsigned int)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&flags[g], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT));
        if (spin_limit < 0 || (v & Q_POISON)) return true;
        if (v >= p) return false;
        if (++spins > spin_limit) return true;
        __builtin_amdgcn_s_sleep(64);
    }
}
__device__ __forceinline__ void queue_publish(unsigned int* flags, size_t g, unsigned int p, bool poisoned, unsigned lane) {
    __threadfence();
    if (lane == 0) __hip_atomic_fetch_max(&flags[g], (poisoned ? Q_POISON : 0u) | (p + 1u), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// The forms for state that travels in tagged words (stw_store / stw_load): the flag only says "worth looking" and carries the poison mark, the data
// validates itself — relaxed accesses, no cache maintenance, and the publisher does not wait for its stores either (21-48 K cycles per task while
// they drained): a reader that arrives before the last word re-reads.
__device__ __forceinline__ bool queue_wait_rlx(unsigned int* flags, size_t g, unsigned int p, int spin_limit) {
    if (p == 0) return false;
    int spins = 0;
    for (;;) {
        const unsigned int v = (unsigned int)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&flags[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (spin_limit < 0 || (v & Q_POISON)) return true;
        if (v >= p) return false;
        if (++spins > spin_limit) return true;
        __builtin_amdgcn_s_sleep(64);
    }
}
__device__ __forceinline__ void queue_publish_rlx(unsigned int* flags, size_t g, unsigned int p, bool poisoned, unsigned lane) {
    if (lane == 0) __hip_atomic_fetch_max(&flags[g], (poisoned ? Q_POISON : 0u) | (p + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gt_poison(uint8_t* o576, int role) {
    uint4* q = reinterpret_cast<uint4*>(o576 + (role == 0 ? 384 : (role == 1 ? 192 : 0)));
#pragma unroll
    for (int j = 0; j < 12; ++j) q[j] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// Diagnostic (experiments runs, C12381_PAIR_STAMPS): what ONE wavefront of a queue kernel spent its launch on, in shader-clock cycles
// (s_memtime) — whole groups, queue tasks from start to publish (state loads and stores included), hand-over waits (claim to start) —
// written once at exit as 12 words per wavefront (tools/queue_wave_stats.py).  Everything is wave-uniform (SGPRs); null pointer = off.
// Inside a task: loaded() after the state has arrived (the tag comparison has consumed it), computed() before the state is stored.
struct queue_wave_stats {
    unsigned long long* out;
    unsigned long long t_entry = 0, whole = 0, task = 0, wait = 0, t0 = 0, t1 = 0, load = 0, store = 0;
    unsigned int n_whole = 0, n_task = 0, reread = 0;
    __device__ __forceinline__ explicit queue_wave_stats(unsigned long long* wstats) : out(wstats) { if (out) t_entry = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void mark() { if (out) t0 = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void whole_done() { if (out) { whole += __builtin_amdgcn_s_memtime() - t0; ++n_whole; } }
    __device__ __forceinline__ void wait_done() { if (out) { const unsigned long long t = __builtin_amdgcn_s_memtime(); wait += t - t0; t0 = t; t1 = t; } }
    __device__ __forceinline__ void loaded() { if (out) { const unsigned long long t = __builtin_amdgcn_s_memtime(); load += t - t1; t1 = t; } }
    __device__ __forceinline__ void computed() { if (out) t1 = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void task_done() { if (out) { const unsigned long long t = __builtin_amdgcn_s_memtime(); task += t - t0; store += t - t1; ++n_task; } }
    __device__ __forceinline__ void finish() {
        if (!out || (threadIdx.x & 63u) != 0) return;
        unsigned long long* o = out + 12 * (((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6);
        o[0] = t_entry; o[1] = __builtin_amdgcn_s_memtime(); o[2] = whole; o[3] = n_whole; o[4] = task; o[5] = n_task; o[6] = wait;
        o[7] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);      // HW_ID | XCC_ID
        o[8] = load; o[9] = store; o[10] = reread;
    }
};

// Task number -> phase p, group g, the group's state block and the tags of the words this task reads (written by phase p - 1) and writes.
// Only the queued groups own a state block (pair_queue_setup): block g - ndirect.
struct queue_task { unsigned int p; size_t g; uint8_t* st; uint32_t tag_in, tag_out; };
__device__ __forceinline__ queue_task queue_task_of(unsigned int task, size_t nq, size_t ndirect, uint8_t* stw, uint32_t epoch) {
    queue_task k;
    k.p = (unsigned int)(task / nq);
    k.g = ndirect + task % nq;
    k.st = wave_uniform(stw + (k.g - ndirect) * PAIR_QUEUE_STATE_BYTES);
    k.tag_in = st_tag(epoch, k.p - 1u); k.tag_out = st_tag(epoch, k.p);
    return k;
}

// Output of one element: EQ = ok byte (1 / 0, 0xff for an invalid element), otherwise the GT value (0xff bytes when invalid); an invalid element
// raises bad_flag[0].  f12t_is_one exchanges across the triple: every lane calls it.
template <bool EQ>
__device__ __forceinline__ void pair_out(uint8_t* out, size_t e, const fp4& F, bool valid, bool active, int* bad_flag, const tri& t) {
    if (EQ) {
        const bool one = f12t_is_one(F, t);
        if (active && t.role == 0) {
            if (!valid) *bad_flag = 1;
            out[e] = valid ? (one ? 1 : 0) : 0xff;
        }
    } else if (active) {
        if (!valid) { *bad_flag = 1; gt_poison(out + 576 * e, t.role); }
        else gt_store_coeff(out + 576 * e, F, t.role);
    }
}
// ... of a poisoned group, by its last task: the group's state was never completed — 0xff outputs, bad_flag[1] (C12381_E_INTERNAL)
template <bool EQ>
__device__ __forceinline__ void pair_out_poisoned(uint8_t* out, size_t e, bool active, int* bad_flag, const tri& t) {
    if (!active) return;
    bad_flag[1] = 1;
    if (EQ) { if (t.role == 0) out[e] = 0xff; } else gt_poison(out + 576 * e, t.role);
}

// py <- -py: e(a1, a2) == e(b1, b2) is tested as e(a1, a2) * e(-b1, b2) == 1
__device__ __forceinline__ void fp_negate(fp& y) {
    fp ny;
    fp_neg(ny, y);
    fp_norm1(y, ny);
}

// One step of the final exponentiation as a queue task (f12t_final_exp_step: steps 0 .. 5 on r, with y1 from step 0 on and aux from step 4).
// `first` = the phase of step 0.  r arrives from the phase before in STW_F — or, step 0 with in0 given, from the 576-byte value at in0 — y1 in
// its own rows, aux borrows the rows of the (finished) running point tc1; each is stored for the steps after it.  Returns poisoned (a word
// never arrived); after step 5 r is the result, for the caller's output.  stats: the caller's queue_wave_stats or null — loaded() after the
// state has arrived, computed() before it is stored; reread counts the re-reads of r.
__device__ __forceinline__ bool queue_fexp_task(const queue_task& k, unsigned int first, const uint8_t* in0, fp4& r, unsigned lane, uint32_t epoch, int spin_limit,
                                                fp4& H, const tri& t, queue_wave_stats* stats = nullptr, unsigned int* reread = nullptr) {
    const int step = (int)(k.p - first);
    fp4 y1, aux;
    bool got = true;
    if (in0 && step == 0) gt_load_coeff(r, in0, t.role);
    else got = stw_load<fp4, ST_DW_F>(r, k.st + STW_F * 1024, lane, k.tag_in, spin_limit, reread);
    if (step >= 1) got = stw_load<fp4, ST_DW_F>(y1, k.st + STW_Y1 * 1024, lane, st_tag(epoch, first), spin_limit) && got;          // written by step 0
    if (step == 5) got = stw_load<fp4, ST_DW_F>(aux, k.st + STW_TC1 * 1024, lane, st_tag(epoch, first + 4u), spin_limit) && got;   // written by step 4
    if (stats) stats->loaded();
    if (!got) return true;
    f12t_final_exp_step(step, r, y1, aux, H, t);
    if (stats) stats->computed();
    if (step < 5) {
        stw_store<fp4, ST_DW_F>(k.st + STW_F * 1024, lane, r, k.tag_out);
        if (step == 0) stw_store<fp4, ST_DW_F>(k.st + STW_Y1 * 1024, lane, y1, k.tag_out);
        if (step == 4) stw_store<fp4, ST_DW_F>(k.st + STW_TC1 * 1024, lane, aux, k.tag_out);
    }
    return false;
}

}  // namespace
