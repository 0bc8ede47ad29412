// Pieces of the pairing work queue shared by the queue kernels of k_pair3.hip and k_pairk.hip: GT output of a triple, the
// tagged-word state of a queued group and the relaxed hand-over flags.  Translation-unit-local (anonymous namespace): every
// function is inlined into the kernels that include it.
#pragma once
#include "kernels_common.hpp"
#include "pairing3.hpp"

namespace {

using namespace c12381;

// Miller-loop tasks per group in the queue kernels (the 64 iterations in equal parts)
constexpr int MILLER_TASKS_PER_GROUP = 4;       // 2 and 8 measured: 2 loses 4 %, 8 is within the spread of 4 (profiles/r04_ab_queue_priority.txt, r05_ab_miller_variants.txt)
static_assert(64 % MILLER_TASKS_PER_GROUP == 0, "the Miller-loop tasks divide the 64 iterations");
constexpr int MILLER_ITERS_PER_TASK = 64 / MILLER_TASKS_PER_GROUP;

__device__ __forceinline__ void gt_store_coeff(uint8_t* o576, const fp4& x, int role) {
    uint8_t* o = o576 + (role == 0 ? 384 : (role == 1 ? 192 : 0));      // FP12_toOctet: c | b | a
    uint32_t raw[12];
    fp_to_raw48(raw, x.b.b); store_raw48(o, raw);
    fp_to_raw48(raw, x.b.a); store_raw48(o + 48, raw);
    fp_to_raw48(raw, x.a.b); store_raw48(o + 96, raw);
    fp_to_raw48(raw, x.a.a); store_raw48(o + 144, raw);
}

// ---- the same state WITHOUT cache maintenance (round 5): every 32-bit word travels in an 8-byte word together with a 32-bit tag — launch epoch and
// the phase that wrote it; a reader that sees another tag in ANY word reads again.  The accesses are agent-scope coherent (sc1: write-through /
// read past this XCD's L2 — the eight XCDs' L2s are not coherent with each other for ordinary accesses: with an L1 invalidation alone the results
// were wrong, profiles/r05_ab_fence_free_handover.txt), and a word validates itself, so no release / acquire pair is needed: none of the
// buffer_wbl2 sc1 / buffer_inv sc1 the fences of the 16-byte form cost per task — a write-back and an invalidation of the whole XCD's L2 under
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

// ---- hand-over protocol of the work queue.  flags[g] = number of finished phases of group g, bit 31 = the group is
// POISONED: a wavefront gave up waiting for its predecessor (bounded spin), so the group's state is not to be trusted.
// A poisoned task skips its arithmetic and passes the mark on (successors then start at once instead of spinning
// through their own bound), the last phase writes 0xff to every output of the group and raises bad_flag[1], which the
// host reports as C12381_E_INTERNAL — a library-internal failure never looks like valid output or like a bad input point.
// Publishing is an atomic max, so a predecessor that was merely slow cannot clear the mark afterwards.
constexpr unsigned int Q_POISON = 0x80000000u;
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

}  // namespace
