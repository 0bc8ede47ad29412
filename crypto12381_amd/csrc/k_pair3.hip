// Three-lanes-per-pairing kernels (pairing3.hpp): each triple of lanes holds one Fp12 (one Fp4 coefficient per lane)
// and one G2 point (one projective coordinate per lane); 21 pairings per wavefront.
//   pair3_kernel       Miller loop + final exponentiation -> 576-byte GT
//   pair3_eq_kernel    e(a1,a2) == e(b1,b2)
#include "kernels_common.hpp"
#include "pairing3.hpp"
#include "fixed_base.hpp"
#include "pair_queue.hpp"

// (The work queue — schedule, hand-over, MILLER_TASKS_PER_GROUP — is stated in pair_queue.hpp; how many groups bypass it is the host's
// decision: host_layouts.hpp queue_direct_groups.)
// (Issue priorities for the two kinds of work — s_setprio around the whole groups / the tasks — were measured and are not in the tree: whole groups
// above tasks doubles the launch, a task holder that cannot issue stalls everyone behind its hand-over; the other two orders change nothing, the
// SIMD's age order already does that.  profiles/r04_ab_queue_priority.txt)
// gt3_pow_queue_kernel ALONE still evaluates the split itself, as every queue kernel did before the host took it over: with ndirect as an
// argument this one kernel gains scratch instructions (514 -> 518 .. 528, profiles/pair_queue_refactor_isa.txt), so the step is not taken for
// it.  A transcription of host_layouts.hpp queue_direct_groups with the override as a device symbol (C12381_QUEUE_GROUPS in an experiments
// build sets both copies, c12381_hip.hip); pair_queue_setup sizes this kernel's slab and tables from the host's value, so the two have to
// stay the same text.
__device__ int g_queue_groups_override = 0;
__device__ __forceinline__ size_t gt_pow_direct_groups(size_t ngroups, size_t nwaves) {
    if (ngroups <= nwaves) return 0;
    size_t queued = ngroups / 3;
    if (queued < nwaves / 2) queued = nwaves / 2;
    if (queued > 2 * nwaves) queued = 2 * nwaves;
    const int ov = g_queue_groups_override;
    if (ov > 0) queued = (size_t)ov < ngroups ? (size_t)ov : ngroups;
    return ngroups - queued;
}
namespace c12381 {
int set_queue_groups_override(int v) { return hipMemcpyToSymbol(HIP_SYMBOL(g_queue_groups_override), &v, sizeof(int)) == hipSuccess ? 0 : -1; }
}

using namespace c12381;

namespace {

__device__ __forceinline__ void tri_setup(tri& t, size_t& idx, bool& active, size_t n) {
    const unsigned lane = threadIdx.x & 63u;
    t = tri_of_lane(lane);
    const queue_elem q = queue_elem_of(((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6, lane, n);      // plain grid: wavefront w takes group w
    active = q.active;
    idx = q.i;
}

// One pair_slot per lane in LDS (pairing3.hpp: the Fp4 + one Fp, 304-byte stride): the running Miller value and the accumulator
// of the exponentiations by x live here, so the out-of-line tower routines read and write their hot operand at LDS latency.
// 76 KB per workgroup, two workgroups per CU.
typedef pair_slot fp4_slot;

// ---- the GT power: its tables, and the state of a queued group between two of its tasks, as rows of 64 x 16 bytes (one per lane) behind
// the fenced hand-over (pair_queue.hpp queue_wait / queue_publish)
constexpr int ST_ROWS_F = 14, ST_ROWS_TC = 7;                 // Fp4 = 56 dwords, Fp2 = 28 dwords
constexpr int GT_POW_TAB_ROWS = 16 * ST_ROWS_F;               // gt3_op_kernel's table of x^0 .. x^15 per wavefront
static_assert(GT_POW_TAB_BYTES_PER_WAVE == (size_t)GT_POW_TAB_ROWS * 64 * 16, "kernels.hpp: size of the power table per wavefront");
constexpr int ST_F = 0, ST_TC1 = ST_ROWS_F, ST_TC2 = ST_TC1 + ST_ROWS_TC, ST_Y1 = ST_TC2 + ST_ROWS_TC;

template <class T, int ROWS>
__device__ __forceinline__ void st_store(uint4* rows, unsigned lane, const T& x) {
    static_assert(sizeof(T) == ROWS * 16, "state row count");
    const int32_t* w = reinterpret_cast<const int32_t*>(&x);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) rows[(size_t)r * 64 + lane] = make_uint4((uint32_t)w[4 * r], (uint32_t)w[4 * r + 1], (uint32_t)w[4 * r + 2], (uint32_t)w[4 * r + 3]);
}
template <class T, int ROWS>
__device__ __forceinline__ void st_load(T& x, const uint4* rows, unsigned lane) {
    static_assert(sizeof(T) == ROWS * 16, "state row count");
    int32_t* w = reinterpret_cast<int32_t*>(&x);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) { const uint4 v = rows[(size_t)r * 64 + lane]; w[4 * r] = (int32_t)v.x; w[4 * r + 1] = (int32_t)v.y; w[4 * r + 2] = (int32_t)v.z; w[4 * r + 3] = (int32_t)v.w; }
}
// the table of x^0 .. x^15 of one wavefront or queued group, as the store / load callables of f12t_pow_window*
struct pow_tab_store {
    uint4* tab; unsigned lane;
    __device__ __forceinline__ void operator()(int k, const fp4& v) const { st_store<fp4, ST_ROWS_F>(tab + (size_t)k * (ST_ROWS_F * 64), lane, v); }
};
struct pow_tab_load {
    const uint4* tab; unsigned lane;
    __device__ __forceinline__ void operator()(fp4& m, int k) const { st_load<fp4, ST_ROWS_F>(m, tab + (size_t)k * (ST_ROWS_F * 64), lane); }
};

}  // namespace

namespace c12381 {

// One whole group of 21 pairings on this wavefront: Miller loop(s) + final exponentiation + output (lane element index i, shadow
// lanes inactive).  EQ: e(a1, a2) == e(b1, b2)  <=>  e(a1, a2) * e(-b1, b2) == 1: one joint Miller loop (shared squarings), one
// final exponentiation.  liner_pair.hpp:339-350 forms ate(a) * conj(ate(b)) from two separate loops; after the final
// exponentiation both are e(a) / e(b) (conj and negating the G1 argument both invert the pairing value; the Miller values differ
// by factors in Fp6, which the easy part kills), so the boolean is the same for all curve points, infinity arguments included.
template <bool EQ>
__device__ __forceinline__ void pair3_whole_group(size_t i, bool active, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2,
                                                  size_t b2_stride, uint8_t* out, int* bad_flag, fp4& H, const tri& t) {
    fp px, py; fp2 qx, qy; bool pinf, qinf, ok, okb = true;
    pair_inputs(px, py, pinf, qx, qy, qinf, ok, a1 + 96 * i, a2 + 192 * i);
    if (!ok) { pinf = true; qinf = true; }
    if (EQ) {
        fp px2, py2; fp2 qx2, qy2; bool pinf2, qinf2;
        pair_inputs(px2, py2, pinf2, qx2, qy2, qinf2, okb, b1 + 96 * i, b2 + b2_stride * i);
        if (!okb) { pinf2 = true; qinf2 = true; }
        fp_negate(py2);
        miller3_loop2(H, px, py, pinf, qx, qy, qinf, px2, py2, pinf2, qx2, qy2, qinf2, t);
    } else {
        miller3_loop(H, px, py, pinf, qx, qy, qinf, t);
    }
    fp4 F;
    slot_load(F, H);
    f12t_final_exp_ws(F, H, t);
    pair_out<EQ>(out, i, F, ok && okb, active, bad_flag, t);
}

__global__ void __launch_bounds__(BLOCK, 2) pair3_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag) {
    if ((((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * TRI_PER_WAVE >= n) return;      // whole wavefront idle
    tri t; size_t i; bool active;
    tri_setup(t, i, active, n);
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 8);                      // plain grid: the two wavefronts of a SIMD take turns (pairing3.hpp C12381_FAIR_SHARE)
    pair3_whole_group<false>(i, active, g1, g2, nullptr, nullptr, 0, gt, bad_flag, slots[threadIdx.x].v, t);
}

__global__ void __launch_bounds__(BLOCK, 2) pair3_eq_kernel(size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2,
                                                         size_t b2_stride, uint8_t* out, int* bad_flag, const int32_t* skip_if) {
    if (skip_if && skip_if[HDR_VALID] != 0) return;          // the fixed-G2 path serves this batch (pair3_prod_fixed_queue_kernel)
    if ((((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * TRI_PER_WAVE >= n) return;
    tri t; size_t i; bool active;
    tri_setup(t, i, active, n);
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 8);                      // plain grid: the two wavefronts of a SIMD take turns (pairing3.hpp C12381_FAIR_SHARE)
    pair3_whole_group<true>(i, active, a1, a2, b1, b2, b2_stride, out, bad_flag, slots[threadIdx.x].v, t);
}

// gt[i] = prod_{j < k} e(g1[j * n + i], g2[j * n + i]),  k = 1 .. MAX_PROD: pair(a, b) * pair(c, d) [* pair(e, f)] as the headers
// form it (liner_pair.hpp:291-303 -> pair_double_ate pair_BLS12381.cpp:508-626, then PAIR_fexp) with ONE joint Miller loop
// (shared squarings) and ONE final exponentiation.  miller_only: stop before the final exponentiation — the value is then
// the reference's Miller value (the product of the single-loop values; a G1 argument at infinity contributes 1, :532-541).
__global__ void __launch_bounds__(BLOCK, 2) pair3_prod_kernel(size_t n, int k, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag, int miller_only) {
    if ((((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * TRI_PER_WAVE >= n) return;      // whole wavefront idle
    tri t; size_t i; bool active;
    tri_setup(t, i, active, n);
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 8);                      // plain grid: the two wavefronts of a SIMD take turns (pairing3.hpp C12381_FAIR_SHARE)
    fp4& H = slots[threadIdx.x].v;
    miller3_pair pr[MAX_PROD];
    bool ok = true;
#pragma unroll 1
    for (int j = 0; j < k; ++j) {
        fp2 qx, qy; bool pinf, qinf, okj;
        pair_inputs(pr[j].px, pr[j].py, pinf, qx, qy, qinf, okj, g1 + 96 * ((size_t)j * n + i), g2 + 192 * ((size_t)j * n + i));
        if (!okj) { pinf = true; qinf = true; }
        ok = ok && okj;
        pr[j].skip = pinf;
        miller3_q(pr[j].Q, qx, qy, qinf);
        miller3_tc(pr[j].tc, pr[j].Q, t);
    }
    { fp4 one; f12t_one(one, t); slot_store(H, one); }
    miller3_rangeK(H, pr, k, 64, 1, t);
    f12t_conj_h(H, t);
    fp4 F;
    slot_load(F, H);
    if (!miller_only) f12t_final_exp_ws(F, H, t);
    pair_out<false>(gt, i, F, ok, active, bad_flag, t);
}

// ------------------------------------------------------------------ work-queue kernels
// The schedule — whole groups first, then phase-major tasks, hand-over and poison — is stated in pair_queue.hpp; the bodies below are its
// control flow for one kind of work each.  Here: ten tasks per queued group, four quarters of the Miller loop (state: F and the running
// point(s)) and the six steps of the final exponentiation.
template <bool EQ>
__device__ __forceinline__ void pair3_queue_body(size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, size_t b2_stride,
                                                 uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, uint32_t epoch,
                                                 fp4& H, unsigned long long* stamps = nullptr, unsigned long long* wstats = nullptr) {
    queue_wave_stats ws(wstats);
    uint8_t* const stw = reinterpret_cast<uint8_t*>(state);
    const unsigned lane = threadIdx.x & 63u;
    const tri t = tri_of_lane(lane);
    const size_t ngroups = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
    constexpr unsigned int MILLER_TASKS = MILLER_TASKS_PER_GROUP, TASKS = MILLER_TASKS + 6;
    const unsigned long long ts_entry = stamps ? __builtin_amdgcn_s_memtime() : 0ull;
    for (;;) {                                                 // whole groups first
        const size_t g = queue_claim(counter + 1, lane);
        if (g >= ndirect) break;
        const queue_elem q = queue_elem_of(g, lane, n);
        const unsigned long long ts_g0 = stamps ? __builtin_amdgcn_s_memtime() : 0ull;
        ws.mark();
        pair3_whole_group<EQ>(q.i, q.active, a1, a2, b1, b2, b2_stride, out, bad_flag, H, t);
        ws.whole_done();
        if (stamps && lane == 0) {                             // diagnostic: whole groups behind the queued groups' tasks (entry 10 nq + g)
            unsigned long long* o = stamps + 4 * ((ngroups - ndirect) * (size_t)TASKS + g);
            o[0] = ts_entry; o[1] = ts_g0; o[2] = __builtin_amdgcn_s_memtime();
            o[3] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);
        }
    }
    const size_t nq = ngroups - ndirect;                       // queued groups: ndirect .. ngroups - 1
    const size_t ntasks = nq * TASKS;
    for (;;) {
        const unsigned int task = queue_claim(counter, lane);
        if ((size_t)task >= ntasks) break;
        const queue_task k = queue_task_of(task, nq, ndirect, stw, epoch);
        const unsigned int p = k.p;
        const queue_elem q = queue_elem_of(k.g, lane, n);
        const size_t i = q.i;
        // diagnostic time stamps (C12381_PAIR_STAMPS, tools/queue_phase_times.py): claim, start after the wait, end — per task
        unsigned long long ts_claim = 0, ts_start = 0;
        if (stamps) ts_claim = __builtin_amdgcn_s_memtime();
        ws.mark();
        bool poisoned = queue_wait_rlx(flags, k.g, p, spin_limit);
        ws.wait_done();
        if (stamps) ts_start = __builtin_amdgcn_s_memtime();
        if (!poisoned && p < MILLER_TASKS) {
            fp px, py, px2, py2; fp2 qx, qy, qx2, qy2; bool pinf, qinf, pinf2 = true, qinf2 = true, ok, okb = true;
            pair_inputs(px, py, pinf, qx, qy, qinf, ok, a1 + 96 * i, a2 + 192 * i);
            if (!ok) { pinf = true; qinf = true; }
            g2p Q, Q2;
            fp2 tc, tc2;
            miller3_q(Q, qx, qy, qinf);
            if (EQ) {
                pair_inputs(px2, py2, pinf2, qx2, qy2, qinf2, okb, b1 + 96 * i, b2 + b2_stride * i);
                if (!okb) { pinf2 = true; qinf2 = true; }
                fp_negate(py2);
                miller3_q(Q2, qx2, qy2, qinf2);
            }
            if (p == 0) {
                miller3_tc(tc, Q, t);
                if (EQ) miller3_tc(tc2, Q2, t);
                fp4 one;
                f12t_one(one, t);
                slot_store(H, one);
            } else {
                fp4 f;
                bool got = stw_load<fp4, ST_DW_F>(f, k.st + STW_F * 1024, lane, k.tag_in, spin_limit);
                got = stw_load<fp2, ST_DW_TC>(tc, k.st + STW_TC1 * 1024, lane, k.tag_in, spin_limit) && got;
                if (EQ) got = stw_load<fp2, ST_DW_TC>(tc2, k.st + STW_TC2 * 1024, lane, k.tag_in, spin_limit) && got;
                poisoned = !got;
                slot_store(H, f);
            }
            ws.loaded();
            if (!poisoned) {
                const int hi = 64 - MILLER_ITERS_PER_TASK * (int)p, lo = hi - (MILLER_ITERS_PER_TASK - 1);
                if (EQ) miller3_range2(H, tc, px, py, pinf, Q, tc2, px2, py2, pinf2, Q2, hi, lo, t);
                else miller3_range(H, tc, px, py, pinf, Q, hi, lo, t);
                if (p == MILLER_TASKS - 1) f12t_conj_h(H, t);
                ws.computed();
                {
                    fp4 f;
                    slot_load(f, H);
                    stw_store<fp4, ST_DW_F>(k.st + STW_F * 1024, lane, f, k.tag_out);
                }
                if (p < MILLER_TASKS - 1) {
                    stw_store<fp2, ST_DW_TC>(k.st + STW_TC1 * 1024, lane, tc, k.tag_out);
                    if (EQ) stw_store<fp2, ST_DW_TC>(k.st + STW_TC2 * 1024, lane, tc2, k.tag_out);
                }
            }
        } else if (!poisoned) {
            fp4 r;
            poisoned = queue_fexp_task(k, MILLER_TASKS, nullptr, r, lane, epoch, spin_limit, H, t, &ws);
            if (!poisoned && p == TASKS - 1) {
                // validity of this lane's inputs (cheap next to the arithmetic; keeps the state slab free of flags)
                fp px, py; fp2 qx, qy; bool pinf, qinf, ok, okb = true;
                pair_inputs(px, py, pinf, qx, qy, qinf, ok, a1 + 96 * i, a2 + 192 * i);
                if (EQ) pair_inputs(px, py, pinf, qx, qy, qinf, okb, b1 + 96 * i, b2 + b2_stride * i);
                pair_out<EQ>(out, q.e, r, ok && okb, q.active, bad_flag, t);
            }
        }
        if (poisoned && p == TASKS - 1) pair_out_poisoned<EQ>(out, q.e, q.active, bad_flag, t);
        queue_publish_rlx(flags, k.g, p, poisoned, lane);
        ws.task_done();
        if (stamps && lane == 0) {
            unsigned long long* o = stamps + 4 * (size_t)task;
            o[0] = ts_claim; o[1] = ts_start; o[2] = __builtin_amdgcn_s_memtime();
            o[3] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);      // HW_ID | XCC_ID
        }
    }
    ws.finish();
}

__global__ void __launch_bounds__(BLOCK, 2) pair3_queue_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt, int* bad_flag, uint4* state,
                                                            unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch, unsigned long long* stamps, unsigned long long* wstats) {
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 0);
    pair3_queue_body<false>(n, g1, g2, nullptr, nullptr, 0, gt, bad_flag, state, flags, counter, ndirect, spin_limit, epoch, slots[threadIdx.x].v, stamps, wstats);
}
__global__ void __launch_bounds__(BLOCK, 2) pair3_eq_queue_kernel(size_t n, const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2,
                                                               size_t b2_stride, uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags,
                                                               unsigned int* counter, const int32_t* skip_if, size_t ndirect, int spin_limit, unsigned int epoch) {
    if (skip_if && skip_if[HDR_VALID] != 0) return;
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 0);
    pair3_queue_body<true>(n, a1, a2, b1, b2, b2_stride, out, bad_flag, state, flags, counter, ndirect, spin_limit, epoch, slots[threadIdx.x].v);
}

// ------------------------------------------------------------------ the split forms through the same queue
// pair_ate alone (MILLER = true: four quarter-loop tasks per group, output = the Miller value) and the final exponentiation alone
// (MILLER = false: its six steps, input = 576-byte Fp12 values) for batches of more than one machine round: the plain grids of
// miller3_kernel / gt3_op_kernel run 2^16 elements (1.52 rounds of equally long wavefront tasks) as two full rounds.  Schedule and
// hand-over of pair_queue.hpp; a separate body, so that the pairing kernels' code is untouched.
template <bool MILLER>
__device__ __forceinline__ void split3_queue_body(size_t n, const uint8_t* in1, const uint8_t* in2, uint8_t* out, int* bad_flag, uint4* state,
                                                  unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, uint32_t epoch, fp4& H,
                                                  unsigned long long* wstats) {
    queue_wave_stats ws(wstats);
    uint8_t* const stw = reinterpret_cast<uint8_t*>(state);
    const unsigned lane = threadIdx.x & 63u;
    const tri t = tri_of_lane(lane);
    const size_t ngroups = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
    constexpr unsigned int TASKS = MILLER ? (unsigned)MILLER_TASKS_PER_GROUP : 6u;
    for (;;) {                                                 // whole groups first
        const size_t g = queue_claim(counter + 1, lane);
        if (g >= ndirect) break;
        const queue_elem q = queue_elem_of(g, lane, n);
        const size_t i = q.i;
        ws.mark();
        if (MILLER) {
            fp px, py; fp2 qx, qy; bool pinf, qinf, ok;
            pair_inputs(px, py, pinf, qx, qy, qinf, ok, in1 + 96 * i, in2 + 192 * i);
            if (!ok) { pinf = true; qinf = true; }
            miller3_loop(H, px, py, pinf, qx, qy, qinf, t);
            fp4 F;
            slot_load(F, H);
            pair_out<false>(out, i, F, ok, q.active, bad_flag, t);
        } else {
            fp4 r;
            gt_load_coeff(r, in1 + 576 * i, t.role);
            f12t_final_exp_ws(r, H, t);
            pair_out<false>(out, i, r, true, q.active, bad_flag, t);
        }
        ws.whole_done();
    }
    const size_t nq = ngroups - ndirect;
    const size_t ntasks = nq * TASKS;
    for (;;) {
        const unsigned int task = queue_claim(counter, lane);
        if ((size_t)task >= ntasks) break;
        const queue_task k = queue_task_of(task, nq, ndirect, stw, epoch);
        const unsigned int p = k.p;
        const queue_elem q = queue_elem_of(k.g, lane, n);
        const size_t i = q.i;
        ws.mark();
        bool poisoned = queue_wait_rlx(flags, k.g, p, spin_limit);
        ws.wait_done();
        if (!poisoned && MILLER) {
            fp px, py; fp2 qx, qy; bool pinf, qinf, ok;
            pair_inputs(px, py, pinf, qx, qy, qinf, ok, in1 + 96 * i, in2 + 192 * i);
            if (!ok) { pinf = true; qinf = true; }
            g2p Q;
            fp2 tc;
            miller3_q(Q, qx, qy, qinf);
            if (p == 0) {
                miller3_tc(tc, Q, t);
                fp4 one;
                f12t_one(one, t);
                slot_store(H, one);
            } else {
                fp4 f;
                bool got = stw_load<fp4, ST_DW_F>(f, k.st + STW_F * 1024, lane, k.tag_in, spin_limit);
                got = stw_load<fp2, ST_DW_TC>(tc, k.st + STW_TC1 * 1024, lane, k.tag_in, spin_limit) && got;
                poisoned = !got;
                slot_store(H, f);
            }
            ws.loaded();
            if (!poisoned) {
                const int hi = 64 - MILLER_ITERS_PER_TASK * (int)p, lo = hi - (MILLER_ITERS_PER_TASK - 1);
                miller3_range(H, tc, px, py, pinf, Q, hi, lo, t);
                ws.computed();
                fp4 f;
                if (p == TASKS - 1) {
                    f12t_conj_h(H, t);
                    slot_load(f, H);
                    pair_out<false>(out, q.e, f, ok, q.active, bad_flag, t);
                } else {
                    slot_load(f, H);
                    stw_store<fp4, ST_DW_F>(k.st + STW_F * 1024, lane, f, k.tag_out);
                    stw_store<fp2, ST_DW_TC>(k.st + STW_TC1 * 1024, lane, tc, k.tag_out);
                }
            }
        } else if (!poisoned) {
            // the six-step hand-over of pair_queue.hpp queue_fexp_task, in place (this body's register allocation: profiles/pair_queue_refactor_isa.txt)
            const int step = (int)p;
            fp4 r, y1, aux;
            bool got = true;
            if (step == 0) gt_load_coeff(r, in1 + 576 * i, t.role);
            else got = stw_load<fp4, ST_DW_F>(r, k.st + STW_F * 1024, lane, k.tag_in, spin_limit, &ws.reread);
            if (step >= 1) got = stw_load<fp4, ST_DW_F>(y1, k.st + STW_Y1 * 1024, lane, st_tag(epoch, 0u), spin_limit) && got;      // written by step 0
            if (step == 5) got = stw_load<fp4, ST_DW_F>(aux, k.st + STW_TC1 * 1024, lane, st_tag(epoch, 4u), spin_limit) && got;    // written by step 4
            poisoned = !got;
            ws.loaded();
            if (!poisoned) {
                f12t_final_exp_step(step, r, y1, aux, H, t);
                ws.computed();
                if (step < 5) {
                    stw_store<fp4, ST_DW_F>(k.st + STW_F * 1024, lane, r, k.tag_out);
                    if (step == 0) stw_store<fp4, ST_DW_F>(k.st + STW_Y1 * 1024, lane, y1, k.tag_out);
                    if (step == 4) stw_store<fp4, ST_DW_F>(k.st + STW_TC1 * 1024, lane, aux, k.tag_out);
                } else pair_out<false>(out, q.e, r, true, q.active, bad_flag, t);
            }
        }
        if (poisoned && p == TASKS - 1) pair_out_poisoned<false>(out, q.e, q.active, bad_flag, t);
        queue_publish_rlx(flags, k.g, p, poisoned, lane);
        ws.task_done();
    }
    ws.finish();
}
__global__ void __launch_bounds__(BLOCK, 2) miller3_queue_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out, int* bad_flag, uint4* state,
                                                              unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch, unsigned long long* wstats) {
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 4);                      // a quarter of the younger wavefront's iterations at raised priority (pairing3.hpp C12381_FAIR_SHARE)
    split3_queue_body<true>(n, g1, g2, out, bad_flag, state, flags, counter, ndirect, spin_limit, epoch, slots[threadIdx.x].v, wstats);
}
__global__ void __launch_bounds__(BLOCK, 2) fexp3_queue_kernel(size_t n, const uint8_t* in576, uint8_t* out, int* bad_flag, uint4* state,
                                                            unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch, unsigned long long* wstats) {
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 4);
    split3_queue_body<false>(n, in576, nullptr, out, bad_flag, state, flags, counter, ndirect, spin_limit, epoch, slots[threadIdx.x].v, wstats);
}

// ------------------------------------------------------------------ both G2 arguments fixed for the batch
// The coefficient tables (69 lines behind the header of the fixed-base tables) and the gate over them are built by k_pairk.hip.
// ok[i] = [ e(a_i, W) * e(c_i, G) == 1 ] with W, G given by their coefficient tables.  The queue of pair_queue.hpp, ten tasks per queued
// group; the Miller tasks carry only F.  Runs only when run_if[HDR_VALID] != 0.
// TWO: product of two pairings, boolean output; otherwise one pairing per element against the table tabw, GT output
// (an invalid table — Q not on the twist — poisons every output and raises the flag).
template <bool TWO>
__device__ __forceinline__ void pair3_fixed_queue_body(size_t n, const uint8_t* a96, const uint8_t* c96, const int32_t* tabw, const int32_t* tabg,
                                                       uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter,
                                                       size_t ndirect, int spin_limit, uint32_t epoch, bool table_ok, fp4& H) {
    uint8_t* const stw = reinterpret_cast<uint8_t*>(state);
    const unsigned lane = threadIdx.x & 63u;
    const tri t = tri_of_lane(lane);
    const size_t ngroups = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
    constexpr unsigned int MILLER_TASKS = MILLER_TASKS_PER_GROUP, TASKS = MILLER_TASKS + 6;
    for (;;) {                                                 // whole groups first
        const size_t g = queue_claim(counter + 1, lane);
        if (g >= ndirect) break;
        const queue_elem q = queue_elem_of(g, lane, n);
        fp ax, ay, cx, cy; bool ainf, cinf = true, oka, okc = true;
        g1_parse96(ax, ay, ainf, oka, a96 + 96 * q.i);
        if (!oka || !table_ok) ainf = true;
        if (TWO) {
            g1_parse96(cx, cy, cinf, okc, c96 + 96 * q.i);
            if (!okc) cinf = true;
        }
        { fp4 one; f12t_one(one, t); slot_store(H, one); }
        if (TWO) miller3_range2_fixed(H, ax, ay, ainf, tabw, cx, cy, cinf, tabg, 64, 1, t);
        else miller3_range_fixed(H, ax, ay, ainf, tabw, 64, 1, t);
        f12t_conj_h(H, t);
        fp4 F;
        slot_load(F, H);
        f12t_final_exp_ws(F, H, t);
        pair_out<TWO>(out, q.e, F, oka && okc && table_ok, q.active, bad_flag, t);      // TWO: table_ok is true (the kernel runs behind the gate)
    }
    const size_t nq = ngroups - ndirect;
    const size_t ntasks = nq * TASKS;
    for (;;) {
        const unsigned int task = queue_claim(counter, lane);
        if ((size_t)task >= ntasks) break;
        const queue_task k = queue_task_of(task, nq, ndirect, stw, epoch);
        const unsigned int p = k.p;
        const queue_elem q = queue_elem_of(k.g, lane, n);
        bool poisoned = queue_wait_rlx(flags, k.g, p, spin_limit);
        fp ax, ay, cx, cy; bool ainf, cinf = true, oka, okc = true;
        if (!poisoned && (p < MILLER_TASKS || p == TASKS - 1)) {
            g1_parse96(ax, ay, ainf, oka, a96 + 96 * q.i);
            if (!oka || !table_ok) ainf = true;
            if (TWO) {
                g1_parse96(cx, cy, cinf, okc, c96 + 96 * q.i);
                if (!okc) cinf = true;
            }
        }
        if (!poisoned && p < MILLER_TASKS) {
            {
                fp4 f;
                if (p == 0) f12t_one(f, t); else poisoned = !stw_load<fp4, ST_DW_F>(f, k.st + STW_F * 1024, lane, k.tag_in, spin_limit);
                slot_store(H, f);
            }
            if (!poisoned) {
                const int hi = 64 - MILLER_ITERS_PER_TASK * (int)p, lo = hi - (MILLER_ITERS_PER_TASK - 1);
                if (TWO) miller3_range2_fixed(H, ax, ay, ainf, tabw, cx, cy, cinf, tabg, hi, lo, t);
                else miller3_range_fixed(H, ax, ay, ainf, tabw, hi, lo, t);
                if (p == MILLER_TASKS - 1) f12t_conj_h(H, t);
                fp4 f;
                slot_load(f, H);
                stw_store<fp4, ST_DW_F>(k.st + STW_F * 1024, lane, f, k.tag_out);
            }
        } else if (!poisoned) {
            fp4 r;
            poisoned = queue_fexp_task(k, MILLER_TASKS, nullptr, r, lane, epoch, spin_limit, H, t);
            if (!poisoned && p == TASKS - 1) pair_out<TWO>(out, q.e, r, oka && okc && table_ok, q.active, bad_flag, t);
        }
        if (poisoned && p == TASKS - 1) pair_out_poisoned<TWO>(out, q.e, q.active, bad_flag, t);
        queue_publish_rlx(flags, k.g, p, poisoned, lane);
    }
}
__global__ void __launch_bounds__(BLOCK, 2) pair3_prod_fixed_queue_kernel(size_t n, const uint8_t* a96, const uint8_t* c96, const int32_t* tabw,
                                                                       const int32_t* tabg, uint8_t* out, int* bad_flag, uint4* state,
                                                                       unsigned int* flags, unsigned int* counter, const int32_t* run_if, size_t ndirect, int spin_limit,
                                                                       unsigned int epoch) {
    if (run_if[HDR_VALID] == 0) return;
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 0);
    pair3_fixed_queue_body<true>(n, a96, c96, tabw, tabg, out, bad_flag, state, flags, counter, ndirect, spin_limit, epoch, true, slots[threadIdx.x].v);
}
// gt[i] = e(P_i, Q) for ONE Q given by its coefficient table (header at `buf`, lines behind it)
__global__ void __launch_bounds__(BLOCK, 2) pair3_fixed_queue_kernel(size_t n, const uint8_t* g1_96, const int32_t* buf, uint8_t* gt, int* bad_flag,
                                                                  uint4* state, unsigned int* flags, unsigned int* counter, size_t ndirect, int spin_limit, unsigned int epoch) {
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 0);
    pair3_fixed_queue_body<false>(n, g1_96, nullptr, buf + HDR_DWORDS, nullptr, gt, bad_flag, state, flags, counter, ndirect, spin_limit, epoch, buf[HDR_VALID] != 0, slots[threadIdx.x].v);
}

// ------------------------------------------------------------------ split pairing and GT arithmetic on triples
// pair_ate alone: the Miller value (not canonical as a pairing value, but the same field element as the reference's)
__global__ void __launch_bounds__(BLOCK, 2) miller3_kernel(size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out, int* bad_flag) {
    if ((((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * TRI_PER_WAVE >= n) return;
    tri t; size_t i; bool active;
    tri_setup(t, i, active, n);
    fp px, py; fp2 qx, qy; bool pinf, qinf, ok;
    pair_inputs(px, py, pinf, qx, qy, qinf, ok, g1 + 96 * i, g2 + 192 * i);
    if (!ok) { if (active) *bad_flag = 1; pinf = true; qinf = true; }
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 8);                      // plain grid: the two wavefronts of a SIMD take turns (pairing3.hpp C12381_FAIR_SHARE)
    fp4& H = slots[threadIdx.x].v;
    miller3_loop(H, px, py, pinf, qx, qy, qinf, t);
    if (active) {
        if (!ok) gt_poison(out + 576 * i, t.role);
        else { fp4 F; slot_load(F, H); gt_store_coeff(out + 576 * i, F, t.role); }
    }
}
// x^e for one wavefront's 21 elements, whole: the windowed ladder over `tab` when every triple holds a member of the cyclotomic subgroup
// (pairing3.hpp f12t_pow_window), the reference's digit sequence otherwise
__device__ __forceinline__ void gt3_pow_whole(fp4& H, const fp4& x, const uint32_t (&e)[8], bool active, uint4* tab, unsigned lane, const tri& t) {
    const bool member = f12t_is_cyclotomic(H, x, t);
    if (__builtin_amdgcn_ballot_w64(active && !member) == 0) f12t_pow_window(H, x, e, t, pow_tab_store{tab, lane}, pow_tab_load{tab, lane});
    else { slot_store(H, x); f12t_pow_generic(H, e, t); }
}
// (op 2 repeats the route choice of gt3_pow_whole with "no table" as a third case: a null-table form of gt3_pow_whole changes the register
// allocation of gt3_pow_queue_kernel, which calls it)
// op 0: a*b (FP12_mul), 1: conj(a), 2: a^e (FP12_pow, e = 32-byte exponent used as given), 3: final exponentiation
// pow_tab (op 2; may be null): 16 Fp4 rows of 64 lanes per wavefront of THIS launch (GT_POW_TAB_ROWS x 64 x 16 bytes each) — the table of
// the windowed ladder, taken when every triple of the wavefront holds a member of the cyclotomic subgroup (pairing3.hpp f12t_pow_window)
__global__ void __launch_bounds__(BLOCK, 2) gt3_op_kernel(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, uint4* pow_tab) {
    if ((((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * TRI_PER_WAVE >= n) return;
    tri t; size_t i; bool active;
    tri_setup(t, i, active, n);
    __shared__ fp4_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 8);                      // plain grid: the two wavefronts of a SIMD take turns (pairing3.hpp C12381_FAIR_SHARE)
    fp4& H = slots[threadIdx.x].v;
    fp4 x, r;
    gt_load_coeff(x, a + 576 * i, t.role);
    if (op == 0) { fp4 y; gt_load_coeff(y, b + 576 * i, t.role); f12t_mul(r, x, y, t); }
    else if (op == 1) { f12t_conj(r, x, t); }
    else if (op == 2) {
        uint32_t raw[8], e[8];
        load_raw32(raw, b + 32 * i); scalar_from_raw32(e, raw);
        bool windows = false;
        if (pow_tab) {                                             // wave-uniform
            const bool member = f12t_is_cyclotomic(H, x, t);
            windows = __builtin_amdgcn_ballot_w64(active && !member) == 0;
        }
        if (windows) {
            const unsigned lane = threadIdx.x & 63u;
            uint4* tab = wave_uniform(pow_tab + (((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * (size_t)(GT_POW_TAB_ROWS * 64));
            f12t_pow_window(H, x, e, t,
                            pow_tab_store{tab, lane}, pow_tab_load{tab, lane});
        } else { slot_store(H, x); f12t_pow_generic(H, e, t); }
        slot_load(r, H);
    }
    else { r = x; f12t_final_exp_ws(r, H, t); }
    if (active) gt_store_coeff(out + 576 * i, r, t.role);
}
// The power for batches of more than one machine round: the schedule of pair_queue.hpp with the FENCED hand-over (plain 16-byte rows, no tags),
// FIVE tasks per queued group — 0: membership test, route, table (windowed route), 1..4: a quarter of the ladder each (16 windows, or
// 64 / 64 / 64 / 65 iterations of the reference's digit sequence).  State between tasks: the accumulator (scaled form) and the route (word 0 of
// the group's second state area).  Tables: pow_tab holds one per wavefront of the grid (whole groups), then one per queued group.
// This kernel is left as it was: it evaluates the split itself (gt_pow_direct_groups, top of this file) and spells the lane / claim / element
// lines of pair_queue.hpp (tri_of_lane, queue_claim, queue_elem_of, pair_out_poisoned) in place — with ndirect as an argument or with those
// pieces called it gains scratch instructions (514 -> 517 .. 531); as it stands its listing has the parent's counts.
constexpr unsigned int GT_POW_TASKS = 5;
__global__ void __launch_bounds__(BLOCK, 2) gt3_pow_queue_kernel(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out, int* bad_flag, uint4* pow_tab,
                                                              uint4* state, unsigned int* flags, unsigned int* counter, int spin_limit) {
    __shared__ fp4_slot slots[BLOCK];
    fp4& H = slots[threadIdx.x].v;
    slot_fair_set(H, 0);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned trip = lane / 3u;
    tri t;
    t.role = lane == 63u ? 0 : (int)(lane - 3u * trip);
    t.base = lane == 63u ? 63 : (int)(3u * trip);
    const size_t ngroups = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
    constexpr int ROWS = ST_Y1 + ST_ROWS_F;
    const size_t nwaves = (size_t)gridDim.x * (BLOCK / 64);
    const size_t wave = ((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const size_t ndirect = gt_pow_direct_groups(ngroups, nwaves);
    uint4* own_tab = wave_uniform(pow_tab + wave * (size_t)(GT_POW_TAB_ROWS * 64));
    for (;;) {                                                 // whole groups first
        const unsigned int gc = atomicAdd(counter + 1, lane == 0 ? 1u : 0u);
        const size_t g = (size_t)(unsigned int)__builtin_amdgcn_readfirstlane((int)gc);
        if (g >= ndirect) break;
        const size_t el = g * TRI_PER_WAVE + (lane == 63u ? TRI_PER_WAVE - 1 : trip);
        const bool active = lane < 63u && el < n;
        const size_t i = el < n ? el : n - 1;
        fp4 x, r;
        uint32_t raw[8], e[8];
        gt_load_coeff(x, a + 576 * i, t.role);
        load_raw32(raw, b + 32 * i); scalar_from_raw32(e, raw);
        gt3_pow_whole(H, x, e, active, own_tab, lane, t);
        slot_load(r, H);
        if (active) gt_store_coeff(out + 576 * i, r, t.role);
    }
    const size_t nq = ngroups - ndirect;
    const size_t ntasks = nq * GT_POW_TASKS;
    for (;;) {
        const unsigned int claimed = atomicAdd(counter, lane == 0 ? 1u : 0u);
        const unsigned int task = (unsigned int)__builtin_amdgcn_readfirstlane((int)claimed);
        if ((size_t)task >= ntasks) break;
        const unsigned int p = (unsigned int)(task / nq);
        const size_t gq = task % nq, g = ndirect + gq;
        const size_t el = g * TRI_PER_WAVE + (lane == 63u ? TRI_PER_WAVE - 1 : trip);
        const bool active = lane < 63u && el < n;
        const size_t i = el < n ? el : n - 1;
        const bool poisoned = queue_wait(flags, g, p, spin_limit);
        uint4* st = state + gq * (size_t)ROWS * 64;
        uint4* tab = wave_uniform(pow_tab + (nwaves + gq) * (size_t)(GT_POW_TAB_ROWS * 64));
        if (poisoned) {
            if (p == GT_POW_TASKS - 1 && active) { bad_flag[1] = 1; gt_poison(out + 576 * el, t.role); }
        } else {
            fp4 x;
            uint32_t raw[8], e[8];
            gt_load_coeff(x, a + 576 * i, t.role);
            load_raw32(raw, b + 32 * i); scalar_from_raw32(e, raw);
            if (p == 0) {
                const bool member = f12t_is_cyclotomic(H, x, t);
                const bool windows = __builtin_amdgcn_ballot_w64(active && !member) == 0;
                if (windows) f12t_pow_window_table(H, x, t, pow_tab_store{tab, lane});
                f12t_pow_acc_init(H, t);
                if (lane == 0) st[ST_TC1 * 64] = make_uint4(windows ? 1u : 0u, 0u, 0u, 0u);
            } else {
                fp4 acc;
                st_load<fp4, ST_ROWS_F>(acc, st + ST_F * 64, lane);
                slot_store(H, acc);
                const bool windows = __builtin_amdgcn_readfirstlane((int)st[ST_TC1 * 64].x) != 0;
                if (windows) {
                    const int whi = 63 - 16 * ((int)p - 1);
                    f12t_pow_window_range(H, e, whi, whi - 15, t, pow_tab_load{tab, lane});
                } else {
                    const int hi = 257 - 64 * ((int)p - 1), lo = p == GT_POW_TASKS - 1 ? 1 : hi - 63;
                    f12t_pow_generic_range(H, x, e, hi, lo, t);
                }
            }
            if (p == GT_POW_TASKS - 1) {
                f12t_unscale3_h(H);
                fp4 r;
                slot_load(r, H);
                if (active) gt_store_coeff(out + 576 * el, r, t.role);
            } else {
                fp4 acc;
                slot_load(acc, H);
                st_store<fp4, ST_ROWS_F>(st + ST_F * 64, lane, acc);
            }
        }
        queue_publish(flags, g, p, poisoned, lane);
    }
}
__global__ void __launch_bounds__(BLOCK, 2) gt3_is_unity_kernel(size_t n, const uint8_t* a, uint8_t* out) {
    if ((((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6) * TRI_PER_WAVE >= n) return;
    tri t; size_t i; bool active;
    tri_setup(t, i, active, n);
    fp4 x;
    gt_load_coeff(x, a + 576 * i, t.role);
    const bool one = f12t_is_one(x, t);
    if (active && t.role == 0) out[i] = one ? 1 : 0;
}

}  // namespace c12381
