// TEST HARNESS (CPU): the per-lane sum over shared bases of fixed_base.hpp (fixed_eval_sum: nb tables of multiples, one accumulator per lane
// across all bases) compiled for the host with C12381_CHECK_BOUNDS, lane by lane, written once for both groups; g1_fixed_sum.cpp and
// g2_fixed_sum.cpp instantiate it with a description S derived from fb_g1 / fb_g2 that adds what only the simulation needs:
//   bool S::parse(point&, const uint8_t*)           a record of POINT_BYTES -> (x : y : 1); false and the point at infinity for all-zero
//   void S::entries(const uint32_t (&k)[8], f)      f(L) for every table entry L the evaluation of scalar k reads (the group's digit split)
//   void S::settle(point&)                          after the addend's addition, as the group's sum kernel leaves the point
//   bool S::is_inf(const point&), void S::encode(uint8_t*, const point&)     finite point -> POINT_BYTES affine bytes
// Table entries are built lazily by fixed_table_put — the routine the table kernels run — and kept per base for the life of the process,
// so a test file pays for an entry once.  Not a product path.
#pragma once
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

namespace fixed_sum_sim {
using namespace c12381;

// the scalar of base i for lane j of a base-major array, as the kernel's functor hands it out
struct sim_scalars {
    const uint8_t* sc; size_t n, j;
    void operator()(int i, uint32_t (&k)[8]) const {
        uint32_t rs[8];
        std::memcpy(rs, sc + 32 * ((size_t)i * n + j), 32);
        scalar_from_raw32(k, rs);
    }
};

template <class S>
struct sim {
    using point = typename S::point;
    static constexpr size_t ENTRIES = (size_t)S::WINDOWS * FB_ENTRIES;
    static constexpr size_t TAB_STRIDE = ENTRIES * S::ENTRY_DWORDS;       // dwords between the tables of two bases (no headers here)
    struct table {
        point base;
        std::vector<int32_t> entries = std::vector<int32_t>(TAB_STRIDE, 0);
        std::vector<char> done = std::vector<char>(ENTRIES, 0);
    };
    static std::map<std::string, table>& tables() { static std::map<std::string, table> t; return t; }      // by the base's bytes

    // out[j] = addend + sum_(i < nb) [scalars[i n + j]] bases[i] for n lanes through the table path (affine points on the curve, all-zero =
    // infinity; addend may be null; 32-byte big-endian scalars, base-major) -> affine results (all-zero = infinity).
    // Returns -2 when a base is the point at infinity or not in the order-r subgroup (the library runs the generic route then).
    static int batch(size_t n, int nb, const uint8_t* bases, const uint8_t* addend, const uint8_t* scalars32, uint8_t* out) {
        constexpr size_t PB = S::POINT_BYTES;
        if (nb < 1 || nb > 32) return -1;
        std::vector<table*> tabs((size_t)nb);
        for (int i = 0; i < nb; ++i) {
            const std::string key((const char*)bases + PB * i, PB);
            auto it = tables().find(key);
            if (it == tables().end()) {
                point b;
                if (!S::parse(b, bases + PB * i) || !S::in_subgroup(b)) return -2;
                it = tables().emplace(key, table()).first;
                it->second.base = b;
            }
            tabs[(size_t)i] = &it->second;
        }
        // the entries this batch reads and no table has yet
        std::vector<std::pair<table*, size_t>> need;
        for (int i = 0; i < nb; ++i)
            for (size_t j = 0; j < n; ++j) {
                uint32_t k[8];
                sim_scalars{scalars32, n, j}(i, k);
                scalar_mod_r(k);
                S::entries(k, [&](size_t L) {
                    table* t = tabs[(size_t)i];
                    if (t->done[L]) return;
                    t->done[L] = 1;
                    need.emplace_back(t, L);
                });
            }
        const size_t T = need.size() < 64 ? 1 : 8;
        std::vector<std::thread> th;
        for (size_t t = 0; t < T; ++t)
            th.emplace_back([&, t] {
                for (size_t e = t; e < need.size(); e += T)
                    fixed_table_put<S>(need[e].first->entries.data() + need[e].second * S::ENTRY_DWORDS, need[e].first->base, need[e].second);
            });
        for (auto& x : th) x.join();
        // one contiguous image of the nb tables, TAB_STRIDE apart, as the kernel sees them
        std::vector<int32_t> imgv((size_t)nb * TAB_STRIDE + 4);
        int32_t* img = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(imgv.data()) + 15) & ~(uintptr_t)15);
        for (int i = 0; i < nb; ++i) std::memcpy(img + (size_t)i * TAB_STRIDE, tabs[(size_t)i]->entries.data(), TAB_STRIDE * 4);
        for (size_t j = 0; j < n; ++j) {
            point acc, o;
            fixed_eval_sum<S>(acc, img, TAB_STRIDE, nb, sim_scalars{scalars32, n, j});
            S::norm1(o, acc);
            if (addend) {
                point q;
                S::parse(q, addend);
                S::add(o, q);
                S::settle(o);
            }
            uint8_t* dst = out + PB * j;
            if (S::is_inf(o)) std::memset(dst, 0, PB);
            else S::encode(dst, o);
        }
        return 0;
    }
};

}  // namespace fixed_sum_sim
