// TEST HARNESS (CPU): the K-term sum of products of g1.hpp (g1_scalar_mul_sum: K co-Z tables on one common Z, one Jacobian loop, complete
// fallback) compiled for the host with C12381_CHECK_BOUNDS, lane by lane, with a report of the lanes that took the complete path.
// Not a product path.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"

using namespace c12381;

namespace {

// term j of lane i of argument-major arrays (k x n records), as the kernel's input functor hands it out
struct sim_in {
    size_t n, i;
    const uint8_t* pts;
    const uint8_t* sc;
    void operator()(int j, fp& px, fp& py, bool& inf, uint32_t (&k)[8]) const {
        uint32_t rp[24], rs[8];
        std::memcpy(rp, pts + 96 * ((size_t)j * n + i), 96);
        std::memcpy(rs, sc + 32 * ((size_t)j * n + i), 32);
        inf = raw_all_zero(rp, 24);
        fp_from_raw48(px, rp); fp_from_raw48(py, rp + 12);
        scalar_from_raw32(k, rs);
    }
};

template <int K>
void lane(size_t n, size_t i, const uint8_t* pts, const uint8_t* sc, int32_t* tab, uint8_t* o, uint8_t* complete) {
    const sim_in in{n, i, pts, sc};
    g1p acc;
    *complete = g1_scalar_mul_sum<K>(acc, in, tab) ? 1 : 0;
    for (int j = 0; j < K; ++j) {                               // the reference's [r]phi(P) term of scalars below x^2, per term
        fp px, py; bool inf; uint32_t k[8];
        in(j, px, py, inf, k);
        if (inf || !scalar_below_x2(k)) continue;
        g1p base, nn;
        base.x = px; base.y = py; fp_one(base.z);
        g1_norm1(nn, acc);
        g1_glv_small_scalar_term(nn, base);
        acc = nn;
    }
    if (g1_is_inf(acc)) { std::memset(o, 0, 96); return; }
    fp zn, zi, ax, ay;
    fp_norm1(zn, acc.z);
    fp_inv(zi, zn);
    g1_to_affine(ax, ay, acc, zi);
    uint32_t rx[12], ry[12];
    fp_to_raw48(rx, ax); fp_to_raw48(ry, ay);
    std::memcpy(o, rx, 48); std::memcpy(o + 48, ry, 48);
}

}  // namespace

extern "C" {

// out[i] = sum_(j < k) [scalars[j n + i]] pts[j n + i] for n lanes (96-byte affine points on the curve, all-zero = infinity; 32-byte
// big-endian scalars; argument-major arrays) -> 96-byte affine results (all-zero = infinity).  complete[i] = 1 when lane i recomputed
// its products with g1_scalar_mul_complete.
int sim_g1_mul_sum_batch(size_t n, int k, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, uint8_t* complete) {
    if (k < 1 || k > 4) return -1;
    std::vector<int32_t> tabv((size_t)k * G1_TAB_DWORDS + 4);
    int32_t* tab = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(tabv.data()) + 15) & ~(uintptr_t)15);
    for (size_t i = 0; i < n; ++i) {
        uint8_t* o = out + 96 * i;
        switch (k) {
            case 1: lane<1>(n, i, pts96, scalars32, tab, o, complete + i); break;
            case 2: lane<2>(n, i, pts96, scalars32, tab, o, complete + i); break;
            case 3: lane<3>(n, i, pts96, scalars32, tab, o, complete + i); break;
            default: lane<4>(n, i, pts96, scalars32, tab, o, complete + i); break;
        }
    }
    return 0;
}

}  // extern "C"
