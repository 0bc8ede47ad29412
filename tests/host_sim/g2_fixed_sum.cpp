// TEST HARNESS (CPU): the per-lane sum over shared G2 bases under the bounds checker: fixed_sum_sim.hpp with the G2 description; the
// addend is added as g2_fixed_sum_kernel adds it.  Not a product path.
#include "fixed_sum_sim.hpp"

using namespace c12381;

namespace {

void fp2_from_bytes96(fp2& r, const uint8_t* p) {                 // b || a
    uint32_t raw[24];
    std::memcpy(raw, p, 96);
    fp_from_raw48(r.b, raw); fp_from_raw48(r.a, raw + 12);
}
void fp2_to_bytes96(uint8_t* p, const fp2& x) {
    uint32_t raw[24];
    fp_to_raw48(raw, x.b); fp_to_raw48(raw + 12, x.a);
    std::memcpy(p, raw, 96);
}

struct sim_g2 : fb_g2 {
    static bool parse(g2p& p, const uint8_t* src) {
        uint32_t rp[48];
        std::memcpy(rp, src, 192);
        if (raw_all_zero(rp, 48)) { g2_set_inf(p); return false; }
        fp2_from_bytes96(p.x, src); fp2_from_bytes96(p.y, src + 96); fp2_one(p.z);
        return true;
    }
    template <class F>
    static void entries(const uint32_t (&k)[8], F f) {                    // the windows of g2_fixed_eval_digits
        uint32_t u[4][2];
        scalar_gs_split(u, k);
        for (int a = 0; a < 4; ++a)
            for (int w = 0; w < FB_G2_WINDOWS; ++w) {
                const uint32_t d = (u[a][w >> 2] >> (8 * (w & 3))) & 255u;
                if (d) f((size_t)w * FB_ENTRIES + (d - 1));
            }
    }
    static void settle(g2p&) {}
    static bool is_inf(const g2p& p) { return g2_is_inf(p); }
    static void encode(uint8_t* dst, const g2p& o) {
        fp2 zn, zi, ax, ay;
        fp2_norm1(zn, o.z); fp2_inv(zi, zn);
        fp2_mul(ax, o.x, zi); fp2_mul(ay, o.y, zi);
        fp2_to_bytes96(dst, ax); fp2_to_bytes96(dst + 96, ay);
    }
};

}  // namespace

// 192-byte points; see fixed_sum_sim::sim::batch
extern "C" int sim_g2_fixed_sum_batch(size_t n, int nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* scalars32, uint8_t* out) {
    return fixed_sum_sim::sim<sim_g2>::batch(n, nb, bases192, addend192, scalars32, out);
}
