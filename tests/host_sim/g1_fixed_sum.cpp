// TEST HARNESS (CPU): the per-lane sum over shared G1 bases under the bounds checker: fixed_sum_sim.hpp with the G1 description; the
// addend is added as g1_fixed_sum_kernel adds it.  Not a product path.
#include "fixed_sum_sim.hpp"

using namespace c12381;

namespace {

struct sim_g1 : fb_g1 {
    static bool parse(g1p& p, const uint8_t* src) {
        uint32_t rp[24];
        std::memcpy(rp, src, 96);
        if (raw_all_zero(rp, 24)) { g1_set_inf(p); return false; }
        fp_from_raw48(p.x, rp); fp_from_raw48(p.y, rp + 12); fp_one(p.z);
        return true;
    }
    template <class F>
    static void entries(const uint32_t (&k)[8], F f) {                    // the windows of g1_fixed_eval_add
        uint32_t k0[4], k1[4];
        scalar_glv_split(k0, k1, k);
        for (int w = 0; w < FB_G1_WINDOWS; ++w)
            for (int h = 0; h < 2; ++h) {
                const uint32_t d = ((h ? k1 : k0)[w >> 2] >> (8 * (w & 3))) & 255u;
                if (d) f((size_t)w * FB_ENTRIES + (d - 1));
            }
    }
    static void settle(g1p& p) { g1_norm1(p); }
    static bool is_inf(const g1p& p) { return g1_is_inf(p); }
    static void encode(uint8_t* dst, const g1p& o) {
        fp zn, zi, ax, ay;
        fp_norm1(zn, o.z); fp_inv(zi, zn);
        g1_to_affine(ax, ay, o, zi);
        uint32_t rx[12], ry[12];
        fp_to_raw48(rx, ax); fp_to_raw48(ry, ay);
        std::memcpy(dst, rx, 48); std::memcpy(dst + 48, ry, 48);
    }
};

}  // namespace

// 96-byte points; see fixed_sum_sim::sim::batch
extern "C" int sim_g1_fixed_sum_batch(size_t n, int nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* scalars32, uint8_t* out) {
    return fixed_sum_sim::sim<sim_g1>::batch(n, nb, bases96, addend96, scalars32, out);
}
