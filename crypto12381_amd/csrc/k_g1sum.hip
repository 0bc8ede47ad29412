// Kernels of the per-lane sum of K G1 products (c12381_g1_mul_sum_batch):
//   g1_mul_sum{2,3,4}_kernel   bytes -> on-curve checks -> K co-Z tables on one common Z, ONE Jacobian loop (g1.hpp g1_scalar_mul_sum)
//                              -> projective SoA in HBM, finished by g1_finish_kernel like a g1_mul_kernel launch
// One term per lane is g1_mul_kernel itself (k_g1.hip).  A translation unit of its own: the three loops compile beside the other families.
#include "kernels_common.hpp"

using namespace c12381;

namespace {

// term j of lane i of the argument-major arrays (`col` records between two terms of a lane).  A point that is not on the curve takes
// part as the point at infinity; the kernel marks its lane invalid afterwards.
struct g1_sum_in {
    const uint8_t* pts;
    const uint8_t* scalars;
    size_t col, i;
    __device__ __forceinline__ void operator()(int j, fp& px, fp& py, bool& inf, uint32_t (&k)[8]) const {
        const size_t rec = (size_t)j * col + i;
        bool at_inf, ok;
        g1_parse96(px, py, at_inf, ok, pts + 96 * rec);
        inf = at_inf || !ok;
        uint32_t raw[8];
        load_raw32(raw, scalars + 32 * rec);
        scalar_from_raw32(k, raw);
    }
};

// tab: K table records per lane, lane-major; proj as in g1_mul_kernel
template <int K>
__device__ __forceinline__ void g1_mul_sum_body(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab, int32_t* proj,
                                                size_t proj_stride, size_t proj_off, int* bad_flag, int small_term) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const g1_sum_in in{pts, scalars, col, i};
    g1p acc;
    g1_scalar_mul_sum<K>(acc, in, tab + i * (size_t)(K * G1_TAB_DWORDS));
    // per term: the on-curve verdict, and the reference's [r]phi(P) term of a scalar below x^2 (g1_mul_kernel: rare, and then as long as a
    // second scalar multiplication for its wavefront)
    bool ok_all = true;
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        const size_t rec = (size_t)j * col + i;
        fp px, py;
        bool inf, ok;
        g1_parse96(px, py, inf, ok, pts + 96 * rec);
        ok_all = ok_all && ok;
        uint32_t raw[8], k[8];
        load_raw32(raw, scalars + 32 * rec);
        scalar_from_raw32(k, raw);
        if (small_term && ok && !inf && scalar_below_x2(k)) {
            g1p base, nn;
            base.x = px; base.y = py; fp_one(base.z);
            g1_norm1(nn, acc);
            g1_glv_small_scalar_term(nn, base);
            acc = nn;
        }
    }
    if (!ok_all) {
        *bad_flag = 1;
        g1_set_invalid(acc);
    }
    g1p o;
    g1_norm1(o, acc);
    soa_store_g1(proj, proj_stride, proj_off + i, o);
}

}  // namespace

namespace c12381 {

__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_sum2_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab,
                                                            int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, int small_term) {
    g1_mul_sum_body<2>(n, pts, scalars, col, tab, proj, proj_stride, proj_off, bad_flag, small_term);
}
__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_sum3_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab,
                                                            int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, int small_term) {
    g1_mul_sum_body<3>(n, pts, scalars, col, tab, proj, proj_stride, proj_off, bad_flag, small_term);
}
__global__ void __launch_bounds__(BLOCK, G1_OCC) g1_mul_sum4_kernel(size_t n, const uint8_t* pts, const uint8_t* scalars, size_t col, int32_t* tab,
                                                            int32_t* proj, size_t proj_stride, size_t proj_off, int* bad_flag, int small_term) {
    g1_mul_sum_body<4>(n, pts, scalars, col, tab, proj, proj_stride, proj_off, bad_flag, small_term);
}

}  // namespace c12381
