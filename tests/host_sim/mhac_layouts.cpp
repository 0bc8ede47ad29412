// TEST HARNESS (CPU): the MHAC-bbs slab layouts of the host API (crypto12381_amd/csrc/host_layouts.hpp) carved twice — sizing only, then on a malloc
// of exactly `bytes` — and written end to end with the byte count the entry's kernels write into each field, as tests/host_sim/host_layouts.cpp does
// for the older layouts.  Built with -fsanitize=address,undefined (tests/test_host_sim_mhac_bbs.py) and run directly.  The shapes come from the
// entry's own set derivation (mhac_bbs.hpp): n in {1, 3, 64, 65, 257}, t in {1, 3, 8}, nPrv in {0, 2, 4} at m = 4, with nothing and with one
// index revealed where one is left.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all mhac_layouts.cpp -o mhac_layouts && ./mhac_layouts
#include "../../crypto12381_amd/csrc/host_layouts.hpp"
#include "../../crypto12381_amd/csrc/mhac_bbs.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace c12381_host;
using namespace c12381;

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
    const size_t ns[] = {1, 3, 64, 65, 257}, ts[] = {1, 3, 8}, nprvs[] = {0, 2, 4};
    const uint32_t prv4[4] = {0, 2, 1, 3}, rev1[1] = {3};
    for (size_t n : ns)
        for (size_t nPrv : nprvs)
            for (size_t nRev = 0; nRev < 2; ++nRev) {
                if (nPrv == 4 && nRev) continue;                 // nothing left to reveal
                mhac_bbs_sets s;
                if (!mhac_bbs_derive(s, 4, prv4, nPrv, rev1, nRev)) { std::fprintf(stderr, "derive refused a valid shape\n"); return 1; }
                // the public block both entries put in front: the gathered list, g1, the decoded list, g2 and w, the statuses
                std::vector<uint8_t> block(MHAC_BBS_PUB_BYTES);
                const ac_bbs_public pub(block.data());
                if ((size_t)(pub.st - block.data()) + 3 + 32 > MHAC_BBS_PUB_BYTES || pub.y49 != block.data() || pub.y49 + 32 * 49 > pub.g96 || pub.g96 + 96 > pub.y96 ||
                    pub.y96 + 32 * 96 > pub.g2 || pub.g2 + 2 * 192 > pub.st) { std::fprintf(stderr, "public block\n"); return 1; }
                {
                    ac_bbs_order o;
                    const size_t nb = mhac_bbs_verify_list(o, s), nrp = s.nRevPub;
                    const size_t sized = mhac_bbs_verify_layout(nullptr, n, nb, nrp).bytes;
                    uint8_t* base = (uint8_t*)std::malloc(sized);
                    const mhac_bbs_verify_slab v = mhac_bbs_verify_layout(base, n, nb, nrp);
                    check("mhac_bbs_verify", base, v.bytes, sized, MHAC_BBS_PUB_BYTES,
                          {{"p49", v.p49, 3 * 49 * n}, {"p96", v.p96, 3 * 96 * n}, {"st_p", v.st_p, 3 * n}, {"sc3", v.sc3, 3 * 32 * n}, {"sca", v.sca, 32 * nb * n},
                           {"c32", v.c32, 32 * n}, {"st", v.st, n}, {"r96", v.r96, 96 * n}, {"s96", v.s96, 96 * n}, {"u49", v.u49, 49 * n}, {"okp", v.okp, n},
                           {"tr", v.tr, mhac_bbs_transcript_bytes(nrp) * n + 3}});       // sha3.hpp reads whole words: up to 3 bytes behind the last transcript
                    std::free(base);
                }
                for (size_t t : ts) {
                    ac_bbs_order o;
                    if (mhac_bbs_pres_list_len(s, t) > MHAC_BBS_MAX_ATTR) continue;      // refused by the entry (t = 8, nPrv = 4 fills 4 + 28 = 32: kept)
                    const size_t total = mhac_bbs_pres_list(o, s, t), nrp = s.nRevPub;
                    const size_t sized = mhac_bbs_pres_layout(nullptr, n, t, total, nrp).bytes;
                    uint8_t* base = (uint8_t*)std::malloc(sized);
                    const mhac_bbs_pres_slab p = mhac_bbs_pres_layout(base, n, t, total, nrp);
                    check("mhac_bbs_pres", base, p.bytes, sized, MHAC_BBS_PUB_BYTES,
                          {{"p49", p.p49, 4 * 49 * n}, {"p96", p.p96, 4 * 96 * n}, {"st_p", p.st_p, 4 * n}, {"st", p.st, n}, {"scr", p.scr, 2 * 32 * n},
                           {"scu", p.scu, 32 * (t + 1) * n}, {"sch", p.sch, 32 * total * n}, {"o96", p.o96, 2 * 96 * n}, {"q96", p.q96, (1 + (t < 4 ? t : 4)) * 96 * n},
                           {"u96", p.u96, 96 * n}, {"v96", p.v96, 96 * n}, {"tr", p.tr, mhac_bbs_transcript_bytes(nrp) * n + 3}});
                    std::free(base);
                }
            }
    std::printf("mhac layouts ok: %d slabs\n", g_checked);
    return 0;
}
