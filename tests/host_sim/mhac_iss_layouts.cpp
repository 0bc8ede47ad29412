// TEST HARNESS (CPU): the slab layouts of the MHAC-bbs issuance entries (crypto12381_amd/csrc/host_layouts.hpp) carved twice — sizing only, then on a
// malloc of exactly `bytes` — and written end to end with the byte count the entry's kernels write into each field, as tests/host_sim/mhac_layouts.cpp
// does for pres and verify.  Built with -fsanitize=address,undefined (tests/test_host_sim_mhac_iss.py) and run directly.  Chunk sizes 1, 63, 4096
// and 2^18, each capped at what the entry forms for the party count (mhac_iss_chunk: 2^18 / nparties), nparties 1, 6 and 64.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all mhac_iss_layouts.cpp -o mhac_iss_layouts && ./mhac_iss_layouts
#include "../../crypto12381_amd/csrc/host_layouts.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace c12381_host;

struct field { const char* name; uint8_t* p; size_t written; };
static int g_checked = 0;

static void check(const char* what, uint8_t* base, size_t bytes, size_t sized, size_t start, const std::vector<field>& f) {
    auto die = [&](const char* why, const char* name) { std::fprintf(stderr, "%s: %s (%s)\n", what, why, name); std::exit(1); };
    if (bytes != sized) die("sizing pass differs", "bytes");
    for (size_t i = 0; i < f.size(); ++i) {
        const size_t off = (size_t)(f[i].p - base);
        if (off % 256) die("field not 256-byte aligned", f[i].name);
        if (off < start) die("field inside the block in front of the slab", f[i].name);
        if (off + f[i].written > bytes) die("field ends behind the slab", f[i].name);
        for (size_t j = 0; j < i; ++j)
            if (f[i].p < f[j].p + f[j].written && f[j].p < f[i].p + f[i].written) die("fields overlap", f[i].name);
        std::memset(f[i].p, 0xa5, f[i].written);
    }
    ++g_checked;
}

int main() {
    const size_t ks[] = {1, 63, 4096, (size_t)1 << 18}, nps[] = {1, 6, 64};
    if (mhac_iss_chunk(1) != (size_t)1 << 18 || mhac_iss_chunk(6) != 43690 || mhac_iss_chunk(64) != 4096 || mhac_iss_chunk((size_t)1 << 19) != 1) {
        std::fprintf(stderr, "mhac_iss_chunk\n");
        return 1;
    }
    for (size_t np : nps)
        for (size_t k0 : ks) {
            const size_t cap = mhac_iss_chunk(np), k = k0 < cap ? k0 : cap, L = k * np;
            const bool big = L > 4096;                                   // the large chunks once, at the reference's shape
            for (size_t t : {(size_t)1, (size_t)3, (size_t)8}) {
                if (t > np && np != 1) continue;
                if (big && t != 3) continue;
                const size_t tt = t > np ? np : t;
                for (size_t cnt : {(size_t)0, (size_t)2, (size_t)32}) {  // nPrv of attr, nPub of iss and type
                    if (big && cnt != 2) continue;
                    {
                        const size_t sized = mhac_iss_attr_layout(nullptr, k, np, cnt).bytes;
                        uint8_t* base = (uint8_t*)std::malloc(sized);
                        const mhac_iss_attr_slab s = mhac_iss_attr_layout(base, k, np, cnt);
                        check("mhac_iss_attr", base, s.bytes, sized, MHAC_BBS_PUB_BYTES, {{"sc", s.sc, 32 * cnt * L}});
                        std::free(base);
                    }
                    {
                        const size_t sized = mhac_iss_iss_layout(nullptr, k, np, tt, cnt).bytes;
                        uint8_t* base = (uint8_t*)std::malloc(sized);
                        const mhac_iss_iss_slab s = mhac_iss_iss_layout(base, k, np, tt, cnt);
                        check("mhac_iss_iss", base, s.bytes, sized, MHAC_BBS_PUB_BYTES,
                              {{"gam", s.gam, 33}, {"c96", s.c96, 96 * L}, {"st_c", s.st_c, L}, {"st", s.st, k}, {"e32", s.e32, 32 * k}, {"inv", s.inv, 32 * k},
                               {"scl", s.scl, 32 * tt * k}, {"scp", s.scp, 32 * cnt * k}, {"nes", s.nes, 32 * L}, {"q96", s.q96, 96 * tt * k}, {"u96", s.u96, 96 * k},
                               {"v96", s.v96, 96 * k}, {"a96", s.a96, 96 * k}, {"r96", s.r96, 96 * L}, {"w96", s.w96, 96 * L}});
                        if (s.bytes > MHAC_BBS_PUB_BYTES + 256 * 15 + (353 + 321 * np + 128 * tt + 32 * cnt) * k + 255 * 15) {
                            std::fprintf(stderr, "mhac_iss_iss: more than the documented bytes per credential\n");
                            return 1;
                        }
                        std::free(base);
                    }
                    if (np == 6) {                                       // group and type do not know the party count: one pass
                        const size_t sized = mhac_iss_group_layout(nullptr, k0, t).bytes;
                        uint8_t* base = (uint8_t*)std::malloc(sized);
                        const mhac_iss_group_slab s = mhac_iss_group_layout(base, k0, t);
                        check("mhac_iss_group", base, s.bytes, sized, 0,
                              {{"p49", s.p49, 49 * t * k0}, {"p96", s.p96, 96 * t * k0}, {"st_p", s.st_p, t * k0}, {"sc", s.sc, 32 * t * k0}, {"u96", s.u96, 96 * k0},
                               {"v96", s.v96, 96 * k0}});
                        std::free(base);
                        const size_t sized2 = mhac_iss_type_layout(nullptr, k0, cnt).bytes;
                        base = (uint8_t*)std::malloc(sized2);
                        const mhac_iss_type_slab y = mhac_iss_type_layout(base, k0, cnt);
                        check("mhac_iss_type", base, y.bytes, sized2, MHAC_BBS_PUB_BYTES,
                              {{"st", y.st, k0}, {"sca", y.sca, 32 * cnt * k0}, {"r96", y.r96, 96 * k0}, {"v96", y.v96, 96 * k0}, {"p96", y.p96, 96 * k0}});
                        std::free(base);
                    }
                }
            }
        }
    std::printf("mhac iss layouts ok: %d slabs\n", g_checked);
    return 0;
}
