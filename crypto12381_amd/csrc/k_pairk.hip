// K-way products of pairings whose G2 arguments are all fixed for the batch (pairing3.hpp miller3_rangek_fixed):
//   gt[i] = prod_{c < K} e(P_c[i], Q_c)  or  ok[i] = [ that product == 1 ],   K <= FIXED_G2_MAX
// The verification equations of the reference's examples are such products: PS (examples/ps/src/ps.cpp:32, :98, :145), BBS+
// (examples/bbs-plus/src/bbs+.cpp:72) and bbs04's R3 (examples/bbs04/src/bbs.cpp:45, :73).  Every Q_c has a 69-line coefficient
// table with the header and cache protocol of the fixed-base tables (k_fixed.hip), so no G2 arithmetic runs per element.
// A separate translation unit: the kernels of k_pair3.hip compile exactly as before.
#include "kernels_common.hpp"
#include "pairing3.hpp"
#include "fixed_base.hpp"
#include "pair_queue.hpp"

using namespace c12381;

namespace c12381 {

// Line tables (pairing3.hpp, 69 lines) of the k points q.p[c] into tabs + c * tab_stride (header + lines), one lane per table; k = 1 is the
// table of a plain pairing against one Q.  rule: bit 0 = the point has to be an element of G2 other than infinity (need_g2: the rewritten
// verification equations hold only there; without it any point of the twist and infinity are valid, and the table holds exactly the lines the
// running-point loop would compute), bit 1 = keep the records raw (the Miller value itself is wanted: a normalised table changes it by
// factors the final exponentiation removes).  header[HDR_RULE] = rule + 1, so a table built under another rule is rebuilt.
__global__ void __launch_bounds__(BLOCK, 2) g2_lines_tables_kernel(int k, g2_cols q, int32_t* tabs, int tab_stride, int rule) {
    const int c = (int)threadIdx.x;
    if (blockIdx.x != 0 || c >= k) return;
    int32_t* buf = tabs + (size_t)c * tab_stride;
    if (buf[HDR_REBUILD] == 0 && buf[HDR_RULE] == rule + 1) return;       // cached table is current
    const bool need_g2 = (rule & 1) != 0, raw = (rule & 2) != 0;
    g2p Q;
    bool inf, ok;
    g2_parse192(Q.x, Q.y, inf, ok, q.p[c]);
    fp2_one(Q.z);
    const bool valid = need_g2 ? (ok && !inf && g2_in_subgroup(Q)) : ok;
    buf[HDR_VALID] = valid ? 1 : 0;
    buf[HDR_RULE] = rule + 1;
    if (valid) miller_lines_precompute(buf + HDR_DWORDS, Q.x, Q.y, inf, !raw);
}
// gate[HDR_VALID] = every one of the k tables is valid (the table-driven kernels run), (gate + GATE_OTHER)[HDR_VALID] = the opposite (the
// generic kernels run: read as (gate + GATE_OTHER)[HDR_VALID] by kernels that skip on "generic")
__global__ void __launch_bounds__(BLOCK, 2) gate_all_kernel(int32_t* gate, const int32_t* tabs, int tab_stride, int k) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int all = 1;
    for (int c = 0; c < k; ++c) all = all && tabs[(size_t)c * tab_stride + HDR_VALID] != 0;
    gate[HDR_VALID] = all;
    gate[GATE_OTHER + HDR_VALID] = all ? 0 : 1;
}
// The G1 arguments of the K columns, parsed once: pts[(c * n + i) * FQK_PT_DWORDS] = (px, py) of cols.p[c][i] in Montgomery limbs,
// with py negated for the columns in neg_mask; mask[i] bit c = column c is at infinity or off the curve (its lines are skipped),
// bit 31 = some column of element i is off the curve (the element's output is poisoned).  Returns at once when skip_if[HDR_VALID] != 0.
__global__ void __launch_bounds__(BLOCK, 2) pairk_prep_kernel(size_t n, int k, g1_cols cols, uint32_t neg_mask, int32_t* pts, uint32_t* mask,
                                                             const int32_t* skip_if) {
    if (skip_if && skip_if[HDR_VALID] != 0) return;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t m = 0;
    for (int c = 0; c < k; ++c) {
        fp x, y;
        bool inf, ok;
        g1_parse96(x, y, inf, ok, cols.p[c] + 96 * i);
        if ((neg_mask >> c) & 1u) fp_negate(y);
        if (!ok) m |= 0x80000000u;
        if (!ok || inf) m |= 1u << c;
        fqk_store_pt(pts + ((size_t)c * n + i) * FQK_PT_DWORDS, x, y);
    }
    mask[i] = m;
}
// dst[i] = src (n copies of one 192-byte point)
__global__ void __launch_bounds__(BLOCK, 2) g2_bcast_kernel(size_t n, const uint8_t* src, uint8_t* dst, const int32_t* skip_if) {
    if (skip_if && skip_if[HDR_VALID] != 0) return;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n * 192) return;
    dst[i] = src[i % 192];                                  // bytewise: a caller's pointer need not be aligned
}

}  // namespace c12381

namespace {

// The work queue of pair_queue.hpp over K tables (the form of pair3_fixed_queue_body, k_pair3.hip): MILLER_TASKS_PER_GROUP quarters of the
// loop, carrying only F, then the six steps of the final exponentiation (none with miller_only: the last Miller task ends the group).
// table_ok = false: every output is poisoned (a G2 point off the twist).
template <bool EQ>
__device__ __forceinline__ void pairk_queue_body(size_t n, int k, const int32_t* pts, const uint32_t* mask, const int32_t* tabs, int tab_stride,
                                                 uint8_t* out, int* bad_flag, uint4* state, unsigned int* flags, unsigned int* counter,
                                                 size_t ndirect, bool miller_only, int spin_limit, uint32_t epoch, bool table_ok, fp4& H) {
    uint8_t* const stw = reinterpret_cast<uint8_t*>(state);
    const unsigned lane = threadIdx.x & 63u;
    const tri t = tri_of_lane(lane);
    const size_t ngroups = (n + TRI_PER_WAVE - 1) / TRI_PER_WAVE;
    const size_t col_stride = n * FQK_PT_DWORDS;
    constexpr unsigned int MILLER_TASKS = MILLER_TASKS_PER_GROUP;
    const unsigned int TASKS = miller_only ? MILLER_TASKS : MILLER_TASKS + 6;
    for (;;) {                                                 // whole groups first
        const size_t g = queue_claim(counter + 1, lane);
        if (g >= ndirect) break;
        const queue_elem q = queue_elem_of(g, lane, n);
        const uint32_t m = mask[q.i];
        const bool valid = table_ok && (m >> 31) == 0;
        { fp4 one; f12t_one(one, t); slot_store(H, one); }
        miller3_rangek_fixed(H, pts + q.i * FQK_PT_DWORDS, col_stride, table_ok ? m : ~0u, k, tabs, tab_stride, 64, 1, t);
        f12t_conj_h(H, t);
        fp4 F;
        slot_load(F, H);
        if (!miller_only) f12t_final_exp_ws(F, H, t);
        pair_out<EQ>(out, q.e, F, valid, q.active, bad_flag, t);
    }
    const size_t nq = ngroups - ndirect;
    const size_t ntasks = nq * TASKS;
    for (;;) {
        const unsigned int task = queue_claim(counter, lane);
        if ((size_t)task >= ntasks) break;
        const queue_task tk = queue_task_of(task, nq, ndirect, stw, epoch);
        const unsigned int p = tk.p;
        const queue_elem q = queue_elem_of(tk.g, lane, n);
        bool poisoned = queue_wait_rlx(flags, tk.g, p, spin_limit);
        uint32_t m = ~0u;
        if (!poisoned && (p < MILLER_TASKS || p == TASKS - 1)) m = mask[q.i];
        const bool valid = table_ok && (m >> 31) == 0;
        if (!poisoned && p < MILLER_TASKS) {
            {
                fp4 f;
                if (p == 0) f12t_one(f, t); else poisoned = !stw_load<fp4, ST_DW_F>(f, tk.st + STW_F * 1024, lane, tk.tag_in, spin_limit);
                slot_store(H, f);
            }
            if (!poisoned) {
                const int hi = 64 - MILLER_ITERS_PER_TASK * (int)p, lo = hi - (MILLER_ITERS_PER_TASK - 1);
                miller3_rangek_fixed(H, pts + q.i * FQK_PT_DWORDS, col_stride, table_ok ? m : ~0u, k, tabs, tab_stride, hi, lo, t);
                if (p == MILLER_TASKS - 1) f12t_conj_h(H, t);
                fp4 f;
                slot_load(f, H);
                if (p == TASKS - 1) pair_out<EQ>(out, q.e, f, valid, q.active, bad_flag, t);      // miller_only: the last Miller task ends the group
                else stw_store<fp4, ST_DW_F>(tk.st + STW_F * 1024, lane, f, tk.tag_out);
            }
        } else if (!poisoned) {
            fp4 r;
            poisoned = queue_fexp_task(tk, MILLER_TASKS, nullptr, r, lane, epoch, spin_limit, H, t);
            if (!poisoned && p == TASKS - 1) pair_out<EQ>(out, q.e, r, valid, q.active, bad_flag, t);
        }
        if (poisoned && p == TASKS - 1) pair_out_poisoned<EQ>(out, q.e, q.active, bad_flag, t);
        queue_publish_rlx(flags, tk.g, p, poisoned, lane);
    }
}

}  // namespace

namespace c12381 {

// gt[i] = prod_{c < k} e(P_c[i], Q_c) from the prep kernel's records and the k tables (tabs = lines of table 0).  gate[HDR_VALID] = 0
// (some Q_c off the twist) poisons every output.  miller_only: the product of the Miller values (raw tables), no final exponentiation.
__global__ void __launch_bounds__(BLOCK, 2) pair3_prodk_fixed_queue_kernel(size_t n, int k, const int32_t* pts, const uint32_t* mask, const int32_t* tabs,
                                                                        int tab_stride, uint8_t* gt, int* bad_flag, uint4* state, unsigned int* flags,
                                                                        unsigned int* counter, const int32_t* gate, size_t ndirect, int miller_only,
                                                                        int spin_limit, unsigned int epoch) {
    __shared__ pair_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 0);
    pairk_queue_body<false>(n, k, pts, mask, tabs, tab_stride, gt, bad_flag, state, flags, counter, ndirect, miller_only != 0, spin_limit, epoch,
                            gate[HDR_VALID] != 0, slots[threadIdx.x].v);
}
// ok[i] = [ prod_{c < k} e(P_c[i], Q_c) == 1 ]: 1 / 0, 0xff where some P_c[i] is off the curve.  Runs only when run_if[HDR_VALID] != 0.
__global__ void __launch_bounds__(BLOCK, 2) pair3_prodk_fixed_eq_queue_kernel(size_t n, int k, const int32_t* pts, const uint32_t* mask, const int32_t* tabs,
                                                                           int tab_stride, uint8_t* ok, int* bad_flag, uint4* state, unsigned int* flags,
                                                                           unsigned int* counter, const int32_t* run_if, size_t ndirect, int spin_limit,
                                                                           unsigned int epoch) {
    if (run_if[HDR_VALID] == 0) return;
    __shared__ pair_slot slots[BLOCK];
    slot_fair_set(slots[threadIdx.x].v, 0);
    pairk_queue_body<true>(n, k, pts, mask, tabs, tab_stride, ok, bad_flag, state, flags, counter, ndirect, false, spin_limit, epoch, true,
                           slots[threadIdx.x].v);
}

}  // namespace c12381
