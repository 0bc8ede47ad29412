// TEST HARNESS (CPU): the K-way table-driven Miller loop of pairing3.hpp (miller3_rangek_fixed) compiled for the host with
// C12381_CHECK_BOUNDS; the three lanes of a triple are three threads exchanging through a barrier-protected mailbox, as in sim.cpp.
// Not a product path.
#include <pthread.h>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/pairing3.hpp"

using namespace c12381;

namespace {
struct TriBox { pthread_barrier_t bar; unsigned char slot[3][sizeof(fp4)]; };
thread_local TriBox* tl_box = nullptr;
}
namespace c12381 {
void c12381_tri_exchange(void* out, const void* in, size_t bytes, int src_role, const tri& t) {
    std::memcpy(tl_box->slot[t.role], in, bytes);
    pthread_barrier_wait(&tl_box->bar);
    std::memcpy(out, tl_box->slot[src_role], bytes);
    pthread_barrier_wait(&tl_box->bar);
}
}

namespace {
constexpr int TAB_STRIDE = FQ_TABLE_DWORDS + 4;          // multiple of 4 dwords: every table 16-byte aligned

struct Job {
    TriBox* box; int role; size_t n; int K; const int32_t* pts; const uint32_t* mask; const int32_t* tabs; int step; int single; uint8_t* out;
};
void gt_store_coeff(uint8_t* o576, const fp4& x, int role) {
    uint8_t* o = o576 + (role == 0 ? 384 : (role == 1 ? 192 : 0));
    const fp* order[4] = {&x.b.b, &x.b.a, &x.a.b, &x.a.a};
    for (int j = 0; j < 4; ++j) { uint32_t raw[12]; fp_to_raw48(raw, *order[j]); std::memcpy(o + 48 * j, raw, 48); }
}
// one lane of every triple: conj of the K-way loop, run as the queue runs it (iterations 64 .. 1 in tasks of `step`), or (single != 0)
// column `single - 1` alone through the same function with K = 1
void* worker(void* arg) {
    Job* jb = static_cast<Job*>(arg);
    tl_box = jb->box;
    tri t; t.role = jb->role; t.base = 0;
    const size_t col_stride = jb->n * FQK_PT_DWORDS;
    for (size_t i = 0; i < jb->n; ++i) {
        pair_slot slot;
        fp4& F = slot.v;
        f12t_one(F, t);
        const int32_t* pts = jb->pts + i * FQK_PT_DWORDS;
        const int32_t* tabs = jb->tabs;
        uint32_t m = jb->mask[i];
        int K = jb->K;
        if (jb->single) {
            const int c = jb->single - 1;
            pts += (size_t)c * col_stride; tabs += (size_t)c * TAB_STRIDE; m >>= c; K = 1;
        }
        for (int hi = 64; hi >= 1; hi -= jb->step) {
            const int lo = hi - jb->step + 1 < 1 ? 1 : hi - jb->step + 1;
            miller3_rangek_fixed(F, pts, col_stride, m, K, tabs, TAB_STRIDE, hi, lo, t);
        }
        fp4 r;
        f12t_conj(r, F, t);
        gt_store_coeff(jb->out + 576 * i, r, jb->role);
    }
    return nullptr;
}
bool on_curve(const fp& x, const fp& y) {            // kernels_common.hpp g1_on_curve
    fp x2, x3, y2, four, rhs;
    fp_sqr(x2, x); fp_mul(x3, x2, x);
    fp_set_const(four, FP_FOUR);
    fp_add(rhs, x3, four);
    fp_sqr(y2, y);
    return fp_equal(y2, rhs);
}
// tables, point records and mask word, then the three lanes.  prep: the records as pairk_prep_kernel writes them (see below); otherwise
// all-zero bytes = infinity and nothing else is looked at.
int run_fixedk(size_t n, int K, const uint8_t* g1s, const uint8_t* g2s, uint32_t neg_mask, bool prep, int raw, int step, int single,
               uint8_t* out576, uint32_t* mask_out) {
    if (K < 1 || K > 31 || step < 1 || step > 64) return -1;
    std::vector<int32_t> tabv((size_t)K * TAB_STRIDE + 4), ptsv((size_t)K * n * FQK_PT_DWORDS + 4);
    int32_t* tabs = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(tabv.data()) + 15) & ~(uintptr_t)15);
    int32_t* pts = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(ptsv.data()) + 15) & ~(uintptr_t)15);
    std::vector<uint32_t> mask(n, 0);
    for (int c = 0; c < K; ++c) {
        uint32_t rq[48];
        std::memcpy(rq, g2s + 192 * c, 192);
        const bool qinf = raw_all_zero(rq, 48);
        fp2 qx, qy;
        fp_from_raw48(qx.b, rq); fp_from_raw48(qx.a, rq + 12);
        fp_from_raw48(qy.b, rq + 24); fp_from_raw48(qy.a, rq + 36);
        miller_lines_precompute(tabs + (size_t)c * TAB_STRIDE, qx, qy, qinf, raw == 0);
        for (size_t i = 0; i < n; ++i) {
            uint32_t rp[24];
            std::memcpy(rp, g1s + 96 * ((size_t)c * n + i), 96);
            fp x, y;
            fp_from_raw48(x, rp); fp_from_raw48(y, rp + 12);
            const bool inf = raw_all_zero(rp, 24);
            if (prep) {
                const bool ok = inf || on_curve(x, y);
                if ((neg_mask >> c) & 1u) { fp ny; fp_neg(ny, y); fp_norm1(y, ny); }
                if (!ok) mask[i] |= 0x80000000u;
                if (!ok || inf) mask[i] |= 1u << c;
            } else if (inf) mask[i] |= 1u << c;
            fqk_store_pt(pts + ((size_t)c * n + i) * FQK_PT_DWORDS, x, y);
        }
    }
    TriBox box;
    pthread_barrier_init(&box.bar, nullptr, 3);
    pthread_t th[3]; Job jb[3];
    for (int r = 0; r < 3; ++r) {
        jb[r] = Job{&box, r, n, K, pts, mask.data(), tabs, step, single, out576};
        pthread_create(&th[r], nullptr, worker, &jb[r]);
    }
    for (int r = 0; r < 3; ++r) pthread_join(th[r], nullptr);
    pthread_barrier_destroy(&box.bar);
    if (mask_out) std::memcpy(mask_out, mask.data(), n * sizeof(uint32_t));
    return 0;
}
}  // namespace

extern "C" {

// out[i] = conj(prod_{c < K} Miller(g1s[c*n + i], g2s[c])) with the lines of g2s[c] from miller_lines_precompute (raw records when
// raw != 0, else normalised); G1 points as the prep kernel stores them (all-zero bytes = infinity, skipped).  step: iterations per
// task (1 .. 64); single = c + 1: column c alone.
int sim_fixedk_miller(size_t n, int K, const uint8_t* g1s, const uint8_t* g2s, int raw, int step, int single, uint8_t* out576) {
    return run_fixedk(n, K, g1s, g2s, 0, false, raw, step, single, out576, nullptr);
}

// The same loop behind the records of pairk_prep_kernel (k_pairk.hip), restated for the host: every G1 argument parsed and tested against
// the curve equation, py negated (pair_queue.hpp fp_negate) for the columns in neg_mask, mask_out[i] bit c = column c is at infinity or off
// the curve, bit 31 = some column of element i is off the curve.  pair_out writes 0xff over such an element; here its value stays, so that a test
// can see that the off-curve column was skipped (its record is not zero).
int sim_fixedk_prep_miller(size_t n, int K, const uint8_t* g1s, const uint8_t* g2s, uint32_t neg_mask, int raw, int step, uint8_t* out576,
                           uint32_t* mask_out) {
    return run_fixedk(n, K, g1s, g2s, neg_mask, true, raw, step, 0, out576, mask_out);
}

}  // extern "C"
