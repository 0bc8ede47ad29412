// TEST HARNESS (CPU): the G1 scalar multiplication of g1.hpp (co-Z affine table, Jacobian loop, complete fallback) compiled for the
// host with C12381_CHECK_BOUNDS, lane by lane, with a report of the lanes that took the complete path.  Not a product path.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"

using namespace c12381;

extern "C" {

// [k]P for n lanes (96-byte affine points, all-zero = infinity; 32-byte big-endian scalars) -> 96-byte affine results (all-zero =
// infinity).  complete[i] = 1 when lane i recomputed its product with g1_scalar_mul_complete.  The reference's [r]phi(P) term of
// scalars below x^2 is added as g1_mul_kernel adds it.
int sim_g1coz_mul_batch(size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, uint8_t* complete) {
    std::vector<int32_t> tabv(G1_TAB_DWORDS + 4);
    int32_t* tab = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(tabv.data()) + 15) & ~(uintptr_t)15);
    for (size_t i = 0; i < n; ++i) {
        uint32_t rp[24], rs[8], k[8];
        std::memcpy(rp, pts96 + 96 * i, 96);
        std::memcpy(rs, scalars32 + 32 * i, 32);
        const bool inf = raw_all_zero(rp, 24);
        fp px, py;
        fp_from_raw48(px, rp); fp_from_raw48(py, rp + 12);
        scalar_from_raw32(k, rs);
        g1p acc;
        complete[i] = g1_scalar_mul(acc, px, py, inf, k, tab) ? 1 : 0;
        if (scalar_below_x2(k) && !inf) {
            g1p base, nn;
            base.x = px; base.y = py; fp_one(base.z);
            g1_norm1(nn, acc);
            g1_glv_small_scalar_term(nn, base);
            acc = nn;
        }
        uint8_t* o = out + 96 * i;
        if (g1_is_inf(acc)) { std::memset(o, 0, 96); continue; }
        fp zn, zi, ax, ay;
        fp_norm1(zn, acc.z);
        fp_inv(zi, zn);
        g1_to_affine(ax, ay, acc, zi);
        uint32_t rx[12], ry[12];
        fp_to_raw48(rx, ax); fp_to_raw48(ry, ay);
        std::memcpy(o, rx, 48); std::memcpy(o + 48, ry, 48);
    }
    return 0;
}

}  // extern "C"
