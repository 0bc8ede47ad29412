// TEST HARNESS (CPU): the slab layouts of the AC issuance entries (crypto12381_amd/csrc/host_layouts.hpp) carved twice — sizing only, then on a malloc
// of exactly `bytes` — and written end to end with the byte count the entry's kernels write into each field, as tests/host_sim/mhac_iss_layouts.cpp
// does.  Built with -fsanitize=address,undefined (tests/test_host_sim_ac_issue.py) and run directly.  Chunk sizes 1, 63, 4096 and 2^18, nattr 1, 4, 32.
// The public block in front of every slab is written with the bytes ac_rps_public's fields hold.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ac_issue_layouts.cpp -o ac_issue_layouts && ./ac_issue_layouts
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
// what the entries put into the public block: g, tilde_g | tilde_X, up to 32 decoded records of Y or of tilde_Y, 3 + 32 statuses
static void write_public(uint8_t* base) {
    const ac_rps_public pub(base);
    const std::vector<field> f = {{"g96", pub.g96, 96}, {"y96", pub.y96, 32 * 96}, {"g2", pub.g2, 2 * 192}, {"ty192", pub.ty192, 32 * 192}, {"st", pub.st, 3 + 32}};
    for (size_t i = 0; i < f.size(); ++i) {
        if ((size_t)(f[i].p - base) + f[i].written > AC_ISSUE_PUB_BYTES) { std::fprintf(stderr, "public block: %s ends behind it\n", f[i].name); std::exit(1); }
        for (size_t j = 0; j < i; ++j)
            if (f[i].p < f[j].p + f[j].written && f[j].p < f[i].p + f[i].written) { std::fprintf(stderr, "public block: %s overlaps\n", f[i].name); std::exit(1); }
        std::memset(f[i].p, 0x5a, f[i].written);
    }
}

int main() {
    const size_t ms[] = {1, 63, 4096, (size_t)1 << 18}, nattrs[] = {1, 4, 32};
    for (size_t m : ms)
        for (size_t na : nattrs) {
            {
                const size_t sized = ac_issue_bbs_layout(nullptr, m, na).bytes;
                uint8_t* base = (uint8_t*)std::malloc(sized);
                const ac_issue_bbs_slab s = ac_issue_bbs_layout(base, m, na);
                write_public(base);
                check("ac_issue_bbs", base, s.bytes, sized, AC_ISSUE_PUB_BYTES,
                      {{"sca", s.sca, 32 * na * m}, {"w32", s.w32, 32 * m}, {"d32", s.d32, 32 * m}, {"inv", s.inv, 32 * m}, {"st", s.st, m}, {"b96", s.b96, 96 * m},
                       {"a96", s.a96, 96 * m}});
                if (s.bytes > AC_ISSUE_PUB_BYTES + (289 + 32 * na) * m + 255 * 7) { std::fprintf(stderr, "ac_issue_bbs: more than the documented bytes per credential\n"); return 1; }
                std::free(base);
            }
            {
                const size_t sized = ac_issue_rps_layout(nullptr, m, na).bytes;
                uint8_t* base = (uint8_t*)std::malloc(sized);
                const ac_issue_rps_slab s = ac_issue_rps_layout(base, m, na);
                write_public(base);
                check("ac_issue_rps", base, s.bytes, sized, AC_ISSUE_PUB_BYTES,
                      {{"sca", s.sca, 32 * na * m}, {"al32", s.al32, 32 * m}, {"sc2", s.sc2, 64 * m}, {"st", s.st, m}, {"st_z", s.st_z, m}, {"q96", s.q96, 192 * m},
                       {"e49", s.e49, 98 * m}, {"tm97", s.tm97, 97 * m}});
                if (s.bytes > AC_ISSUE_PUB_BYTES + (485 + 32 * na) * m + 255 * 8) { std::fprintf(stderr, "ac_issue_rps: more than the documented bytes per credential\n"); return 1; }
                std::free(base);
            }
            if (na == 1) {
                const size_t sized = ac_issue_keygen_layout(nullptr, m).bytes;
                uint8_t* base = (uint8_t*)std::malloc(sized);
                const ac_issue_keygen_slab s = ac_issue_keygen_layout(base, m);
                write_public(base);
                check("ac_issue_keygen", base, s.bytes, sized, AC_ISSUE_PUB_BYTES, {{"sc", s.sc, 32 * m}});
                std::free(base);
            }
        }
    std::printf("ac issue layouts ok: %d slabs\n", g_checked);
    return 0;
}
