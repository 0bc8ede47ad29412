// TEST KERNEL, experiments library only (-DC12381_EXPERIMENTS; the product library does not contain it): the Fp / Fp2 leaf routines on RAW
// limbs, one element per lane, one op code per routine (fp_raw_ops.hpp — the same dispatch tests/host_sim/fp_raw.cpp runs on the host).
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

}  // namespace c12381
