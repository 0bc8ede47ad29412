// TEST HARNESS (CPU): the parts of hash-to-G1 and of the Zp fold that the other host units do not reach, compiled for the host with
// C12381_CHECK_BOUNDS: g1_map_to_point alone and g1_clear_cofactor alone (modes 1 and 2 of g1_from_hash_kernel, k_hash_zp.hip), each
// followed by the conversion of g1_finish_kernel (k_g1.hip), and the stage loop of c12381_zp_inner_product_dev over zp_fold_kernel.
// Not a product path.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"
#include "../../crypto12381_amd/csrc/fr.hpp"
#include "../../crypto12381_amd/csrc/h2c.hpp"

using namespace c12381;

namespace {

void load48(fp& r, const uint8_t* b) {
    uint32_t w[12];
    std::memcpy(w, b, 48);
    fp_from_raw48(r, w);
}
// g1_on_curve and g1_parse96 of kernels_common.hpp
bool on_curve(const fp& x, const fp& y) {
    fp x2, x3, y2, four, rhs;
    fp_sqr(x2, x); fp_mul(x3, x2, x);
    fp_set_const(four, FP_FOUR);
    fp_add(rhs, x3, four);
    fp_sqr(y2, y);
    return fp_equal(y2, rhs);
}
void parse96(fp& x, fp& y, bool& inf, bool& ok, const uint8_t* p) {
    uint32_t raw[24];
    std::memcpy(raw, p, 96);
    inf = raw_all_zero(raw, 24);
    fp_from_raw48(x, raw); fp_from_raw48(y, raw + 12);
    ok = inf || on_curve(x, y);
}
// g1_finish_kernel with one lane (T = 1) and fmt 96: the running products of the Z coordinates (1 in place of a zero), one inversion,
// the unwinding; Z = 0 gives the all-zero record of infinity, or all-ones for the mark of a rejected input (g1_is_invalid)
void finish96(const std::vector<g1p>& proj, uint8_t* out) {
    const size_t n = proj.size();
    if (n == 0) return;
    std::vector<fp> pref(n);
    fp run, one;
    fp_one(run); fp_one(one);
    for (size_t e = 0; e < n; ++e) {
        fp z = proj[e].z;
        fp_select(z, fp_is_zero(z), one, z);
        fp_mul(run, run, z);
        pref[e] = run;
    }
    fp inv;
    fp_inv(inv, run);
    for (size_t e = n; e-- > 0;) {
        g1p p = proj[e];
        const bool inf = fp_is_zero(p.z), invalid = g1_is_invalid(p);
        fp_select(p.z, inf, one, p.z);
        fp prev = e ? pref[e - 1] : one, zinv, ax, ay;
        fp_mul(zinv, inv, prev);
        fp_mul(inv, inv, p.z);
        g1_to_affine(ax, ay, p, zinv);
        uint32_t rx[12], ry[12];
        fp_to_raw48(rx, ax); fp_to_raw48(ry, ay);
        if (inf) for (int j = 0; j < 12; ++j) rx[j] = ry[j] = invalid ? 0xffffffffu : 0u;
        std::memcpy(out + 96 * e, rx, 48); std::memcpy(out + 96 * e + 48, ry, 48);
    }
}
void fr_load32(fr& r, const uint8_t* p) {
    uint32_t raw[8], k[8];
    std::memcpy(raw, p, 32);
    scalar_from_raw32(k, raw);
    fr_from_words(r, k);
}
void fr_store32(uint8_t* p, const fr& a) {
    uint32_t k[8], raw[8];
    fr_to_words(k, a);
    for (int i = 0; i < 8; ++i) raw[i] = bswap32(k[7 - i]);
    std::memcpy(p, raw, 32);
}
// zp_fold_kernel: out[t] = sum over i = t (mod T) of a[i] * b[i] (b == nullptr: of a[i])
void fold(size_t n, const uint8_t* a, const uint8_t* b, size_t T, uint8_t* out) {
    for (size_t t = 0; t < T; ++t) {
        fr acc;
        for (int j = 0; j < 8; ++j) acc.w[j] = 0;
        for (size_t i = t; i < n; i += T) {
            fr x;
            fr_load32(x, a + 32 * i);
            if (b) { fr y; fr_load32(y, b + 32 * i); fr_mul(x, x, y); }
            fr_add(acc, acc, x);
        }
        fr_store32(out + 32 * t, acc);
    }
}

}  // namespace

extern "C" {

// mode 1 of g1_from_hash_kernel: 48-byte field elements -> g1_map_to_point -> 96 bytes
int sim_h2c_map_to_point(size_t n, const uint8_t* u48, uint8_t* out96) {
    std::vector<g1p> proj(n);
    for (size_t i = 0; i < n; ++i) {
        fp u;
        g1p p;
        load48(u, u48 + 48 * i);
        g1_map_to_point(p, u);
        g1_norm1(proj[i], p);
    }
    finish96(proj, out96);
    return 0;
}

// mode 2: 96-byte affine points -> g1_clear_cofactor -> 96 bytes; *bad = 1 if a point was not on the curve (its record: all-ones)
int sim_h2c_clear_cofactor(size_t n, const uint8_t* in96, uint8_t* out96, int* bad) {
    std::vector<g1p> proj(n);
    *bad = 0;
    for (size_t i = 0; i < n; ++i) {
        g1p p;
        bool inf, ok;
        parse96(p.x, p.y, inf, ok, in96 + 96 * i);
        fp_one(p.z);
        if (inf) g1_set_inf(p);
        g1_clear_cofactor(p);
        if (!ok) { *bad = 1; fp_one(p.x); fp_zero(p.y); fp_zero(p.z); }
        g1_norm1(proj[i], p);
    }
    finish96(proj, out96);
    return 0;
}

// c12381_zp_inner_product_dev: strided partial sums, 64 terms per lane and stage, between two reduction slots; *stages = launches
int sim_zp_inner_product(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out32, int* stages) {
    *stages = 0;
    if (n == 0) { std::memset(out32, 0, 32); return 0; }
    std::vector<uint8_t> slot[2];
    const uint8_t *cur_a = a, *cur_b = b;
    size_t cur_n = n;
    int s = 0;
    for (;;) {
        const size_t T = (cur_n + 63) / 64;
        uint8_t* dst = out32;
        if (T > 1) { slot[s].assign(32 * T, 0); dst = slot[s].data(); }
        fold(cur_n, cur_a, cur_b, T, dst);
        ++*stages;
        if (T == 1) return 0;
        cur_a = dst; cur_b = nullptr; cur_n = T;
        s ^= 1;
    }
}

}  // extern "C"
