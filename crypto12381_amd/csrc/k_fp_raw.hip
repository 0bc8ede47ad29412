// TEST KERNELS, experiments library only (-DC12381_EXPERIMENTS; the product library does not contain them): the Fp / Fp2 leaf routines on RAW
// limbs, one op code per routine (fp_raw_ops.hpp — the same dispatch tests/host_sim/fp_raw.cpp runs on the host).  fp_raw_kernel runs
// fp.hpp and the whole-element fp2.hpp one element per lane, fp2h_raw_kernel the two-lane form of fp2h.hpp two lanes per element.
// tests/test_gpu_fp_raw.py compares every output limb with the integer the mathematics predicts.
#include "kernels_common.hpp"
#include "fp_raw_ops.hpp"

using namespace c12381;

namespace c12381 {

// in [n][arity][14], k [n][4], out [n][outputs][14]; arity and outputs follow from op (fp_raw_arity / fp_raw_outputs)
__global__ void __launch_bounds__(BLOCK, 2) fp_raw_kernel(int op, size_t n, const int32_t* in, const int32_t* kk, int32_t* out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int ar = fp_raw_arity(op), no = fp_raw_outputs(op);
    fp x[FR_MAX_IN], r[FR_MAX_OUT];
    int32_t k[FR_MAX_K];
#pragma unroll
    for (int e = 0; e < FR_MAX_IN; ++e) {
        fp_zero(x[e]);
        if (e < ar) {
#pragma unroll
            for (int j = 0; j < NL; ++j) x[e].l[j] = in[(i * ar + e) * NL + j];
        }
    }
#pragma unroll
    for (int j = 0; j < FR_MAX_K; ++j) k[j] = kk[i * FR_MAX_K + j];
    fp_raw_apply(op, x, k, r);
#pragma unroll
    for (int e = 0; e < FR_MAX_OUT; ++e) {
        if (e < no) {
#pragma unroll
            for (int j = 0; j < NL; ++j) out[(i * no + e) * NL + j] = r[e].l[j];
        }
    }
}

// The two-lane ops (FH2_*): lanes 2i and 2i + 1 run element i, as g2_mul2_kernel lays a batch out.  A pair leaves together (i >= n), so the
// partner of a running lane always runs; op is uniform, so no lane of a wavefront is masked around a partner fetch.  Each lane loads the
// whole operands, takes its half by its role (fp2h_from), and stores its half of the result: out [n][2][14], out[i][role].
__global__ void __launch_bounds__(BLOCK, 2) fp2h_raw_kernel(int op, size_t n, const int32_t* in, const int32_t* kk, int32_t* out) {
    const size_t i = ((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 1;
    if (i >= n) return;
    const int ar = fp_raw_arity(op);
    fp x[FR_MAX_IN];
    int32_t k[FR_MAX_K];
#pragma unroll
    for (int e = 0; e < FR_MAX_IN; ++e) {
        fp_zero(x[e]);
        if (e < ar) {
#pragma unroll
            for (int j = 0; j < NL; ++j) x[e].l[j] = in[(i * ar + e) * NL + j];
        }
    }
#pragma unroll
    for (int j = 0; j < FR_MAX_K; ++j) k[j] = kk[i * FR_MAX_K + j];
    fp2h r;
    fp2h_raw_apply(op, x, k, r);
    const size_t o = (i * 2 + (size_t)fp2h_role()) * NL;
#pragma unroll
    for (int j = 0; j < NL; ++j) out[o + j] = r.v.l[j];
}

}  // namespace c12381
