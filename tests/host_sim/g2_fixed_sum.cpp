// TEST HARNESS (CPU): the per-lane sum over shared G2 bases of fixed_base.hpp (g2_fixed_eval_sum: nb tables of multiples, one accumulator per
// lane across all bases) compiled for the host with C12381_CHECK_BOUNDS, lane by lane; the addend is added as g2_fixed_sum_kernel adds it.
// Table entries are built lazily with g2_fixed_entry, exactly as the table kernel computes them, and kept per base for the life of the
// process, so a test file pays for an entry once.  Not a product path.
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"
#include "../../crypto12381_amd/csrc/fixed_base.hpp"

using namespace c12381;

namespace {

constexpr size_t ENTRIES = (size_t)FB_G2_WINDOWS * FB_ENTRIES;
constexpr size_t TAB_STRIDE = ENTRIES * FB_G2_DWORDS;             // dwords between the tables of two bases (no headers here)

struct table {
    g2p base;
    std::vector<int32_t> entries = std::vector<int32_t>(ENTRIES * FB_G2_DWORDS, 0);
    std::vector<char> done = std::vector<char>(ENTRIES, 0);
};
std::map<std::string, table> g_tables;                            // by the base's 192 bytes

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
bool parse192(g2p& p, const uint8_t* src) {                       // -> false for the all-zero record (infinity)
    uint32_t rp[48];
    std::memcpy(rp, src, 192);
    if (raw_all_zero(rp, 48)) { g2_set_inf(p); return false; }
    fp2_from_bytes96(p.x, src); fp2_from_bytes96(p.y, src + 96); fp2_one(p.z);
    return true;
}

void build_entry(table& t, size_t L) {
    const int j = (int)(L / FB_ENTRIES);
    const uint32_t d = (uint32_t)(L % FB_ENTRIES) + 1u;
    g2p acc;
    g2_fixed_entry(acc, t.base, d, 8 * j);
    fp2 zn, zi, ax, ay;
    fp2_norm1(zn, acc.z); fp2_inv(zi, zn);
    fp2_mul(ax, acc.x, zi); fp2_mul(ay, acc.y, zi);
    fp2_norm1(ax, ax); fp2_norm1(ay, ay);
    fb_store_g2(t.entries.data() + L * FB_G2_DWORDS, ax, ay);
}

// the scalar of base i for lane j of a base-major array, as the kernel's functor hands it out
struct sim_scalars {
    const uint8_t* sc; size_t n, j;
    void operator()(int i, uint32_t (&k)[8]) const {
        uint32_t rs[8];
        std::memcpy(rs, sc + 32 * ((size_t)i * n + j), 32);
        scalar_from_raw32(k, rs);
    }
};

}  // namespace

extern "C" {

// out[j] = addend + sum_(i < nb) [scalars[i n + j]] bases[i] for n lanes through the table path (192-byte affine points on the twist, all-zero
// = infinity; addend192 may be null; 32-byte big-endian scalars, base-major) -> 192-byte affine results (all-zero = infinity).
// Returns -2 when a base is the point at infinity or not in the order-r subgroup (the library runs the generic route then).
int sim_g2_fixed_sum_batch(size_t n, int nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* scalars32, uint8_t* out) {
    if (nb < 1 || nb > 32) return -1;
    std::vector<table*> tabs((size_t)nb);
    for (int i = 0; i < nb; ++i) {
        const std::string key((const char*)bases192 + 192 * i, 192);
        auto it = g_tables.find(key);
        if (it == g_tables.end()) {
            g2p b;
            if (!parse192(b, bases192 + 192 * i) || !g2_in_subgroup(b)) return -2;
            it = g_tables.emplace(key, table()).first;
            it->second.base = b;
        }
        tabs[(size_t)i] = &it->second;
    }
    // the entries this batch reads and no table has yet
    std::vector<std::pair<table*, size_t>> need;
    for (int i = 0; i < nb; ++i)
        for (size_t j = 0; j < n; ++j) {
            uint32_t k[8], u[4][2];
            sim_scalars{scalars32, n, j}(i, k);
            scalar_mod_r(k);
            scalar_gs_split(u, k);
            for (int a = 0; a < 4; ++a)
                for (int w = 0; w < FB_G2_WINDOWS; ++w) {
                    const uint32_t d = (u[a][w >> 2] >> (8 * (w & 3))) & 255u;
                    if (!d) continue;
                    const size_t L = (size_t)w * FB_ENTRIES + (d - 1);
                    if (tabs[(size_t)i]->done[L]) continue;
                    tabs[(size_t)i]->done[L] = 1;
                    need.emplace_back(tabs[(size_t)i], L);
                }
        }
    const size_t T = need.size() < 64 ? 1 : 8;
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&, t] { for (size_t e = t; e < need.size(); e += T) build_entry(*need[e].first, need[e].second); });
    for (auto& x : th) x.join();
    // one contiguous image of the nb tables, TAB_STRIDE apart, as the kernel sees them
    std::vector<int32_t> imgv((size_t)nb * TAB_STRIDE + 4);
    int32_t* img = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(imgv.data()) + 15) & ~(uintptr_t)15);
    for (int i = 0; i < nb; ++i) std::memcpy(img + (size_t)i * TAB_STRIDE, tabs[(size_t)i]->entries.data(), TAB_STRIDE * 4);
    for (size_t j = 0; j < n; ++j) {
        g2p acc, o;
        g2_fixed_eval_sum(acc, img, TAB_STRIDE, nb, sim_scalars{scalars32, n, j});
        g2_norm1(o, acc);
        if (addend192) {
            g2p q;
            parse192(q, addend192);
            g2_add(o, q);
        }
        uint8_t* dst = out + 192 * j;
        if (g2_is_inf(o)) { std::memset(dst, 0, 192); continue; }
        fp2 zn, zi, ax, ay;
        fp2_norm1(zn, o.z); fp2_inv(zi, zn);
        fp2_mul(ax, o.x, zi); fp2_mul(ay, o.y, zi);
        fp2_to_bytes96(dst, ax); fp2_to_bytes96(dst + 96, ay);
    }
    return 0;
}

}  // extern "C"
