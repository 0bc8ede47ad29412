// TEST HARNESS (CPU): every slab layout of the host API (crypto12381_amd/csrc/host_layouts.hpp) carved twice — sizing only, then on a malloc of
// exactly `bytes` — and written end to end with the byte count the entry's kernels write into each field.  Built with
// -fsanitize=address,undefined (tests/test_host_layouts.py): a field sized below what its kernel writes runs into its neighbour (caught by
// the disjointness check) or past the slab (caught by the sanitizer).  Per layout: every field 256-byte aligned, fields pairwise disjoint,
// the last one ending at or before `bytes`, the sizing pass equal to the real one.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all host_layouts.cpp -o host_layouts && ./host_layouts
#include "../../crypto12381_amd/csrc/host_layouts.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace c12381_host;

struct field { const char* name; uint8_t* p; size_t written; };
static int g_checked = 0;

// `start`: bytes in front of the first field that belong to somebody else (bbs04's public block)
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
// carve with a null base for the size, then on exactly that many bytes
#define CARVE(slab, layout, ...) \
    const size_t sized = layout(nullptr, __VA_ARGS__).bytes; \
    uint8_t* base = (uint8_t*)std::malloc(sized); \
    const slab s = layout(base, __VA_ARGS__)

// today's rule for the groups that bypass the queue, transcribed literally: pair_queue_layout has to give these values
static size_t rule_direct(size_t ngroups, size_t nwaves, int ov) {
    if (ngroups <= nwaves) return 0;
    size_t queued = ngroups / 3;
    if (queued < nwaves / 2) queued = nwaves / 2;
    if (queued > 2 * nwaves) queued = 2 * nwaves;
    if (ov > 0) queued = (size_t)ov < ngroups ? (size_t)ov : ngroups;
    return ngroups - queued;
}
// The queue slab of the pairing kernels for n elements: head of groups + 2 words (flags, task counter, whole-group counter), one state block per
// QUEUED group (the kernels index block g - ndirect for g in [ndirect, groups)), the split equal to the transcription above.  Sizing only —
// 2^18 verifications are 344 MB — except for the head, which is carved and written.
static void check_queue(size_t n, bool tagged, int ov) {
    auto die = [&](const char* why) { std::fprintf(stderr, "pair_queue n=%zu tagged=%d override=%d: %s\n", n, (int)tagged, ov, why); std::exit(1); };
    const size_t groups = (n + 20) / 21, waves = groups < 2048 ? groups : 2048, blocks = (waves + 3) / 4, nwaves = blocks * 4;
    const size_t block_bytes = tagged ? (size_t)168 * 64 * 8 : (size_t)42 * 1024;
    const pair_queue_slab z = pair_queue_layout(nullptr, n, tagged, ov);
    if (z.flags || z.counter || z.state) die("sizing pass hands out pointers");
    if (z.blocks != blocks || z.nwaves != nwaves) die("grid");
    if (z.ndirect + z.nq != groups) die("ndirect + nq != groups");
    if (z.ndirect != rule_direct(groups, nwaves, ov)) die("ndirect differs from the rule");
    const bool all_queued = groups <= nwaves || (ov > 0 && (size_t)ov >= groups);
    if ((z.ndirect == 0) != all_queued) die("every group queued exactly when the batch fits the grid or the override covers it");
    if (z.nq == 0) die("nq == 0");                               // the rule never queues nothing: half a grid at least, an override is > 0
    const size_t head = (groups + 2) * 4;
    std::vector<uint8_t> fake(1);                                // offsets only: the slab is not allocated
    const pair_queue_slab s = pair_queue_layout(fake.data(), n, tagged, ov);
    const size_t o_flags = (size_t)(s.flags - fake.data()), o_counter = (size_t)(s.counter - fake.data()), o_state = (size_t)(s.state - fake.data());
    if (s.bytes != z.bytes || s.ndirect != z.ndirect || s.nq != z.nq) die("sizing pass differs");
    if (o_flags != 0 || o_counter != groups * 4) die("head: flags, then the two counters");
    if (o_state % 256 || o_state < head) die("state starts inside the head or unaligned");
    for (size_t g = z.ndirect; g < groups; ++g) {               // every block a queued group indexes
        const size_t lo = o_state + (g - z.ndirect) * block_bytes;
        if (lo < o_state || lo + block_bytes > z.bytes) die("a queued group's block lies outside the slab");
    }
    uint8_t* hd = (uint8_t*)std::malloc(head);                   // what pair_queue_setup zeroes per launch: exactly the head
    const pair_queue_slab h = pair_queue_layout(hd, n, tagged, ov);
    std::memset(h.flags, 0, (size_t)(h.counter - h.flags) + 8);
    std::free(hd);
    ++g_checked;
}

int main() {
    for (bool tagged : {true, false}) {                         // n = 0 (no entry launches it): no group, an empty head of the two counters
        const pair_queue_slab z = pair_queue_layout(nullptr, 0, tagged, 0);
        if (z.ndirect != 0 || z.nq != 0 || z.blocks != 0 || z.bytes != 256) { std::fprintf(stderr, "pair_queue n=0\n"); return 1; }
    }
    {                                                           // pairing work queue: group counts around every edge of the rule, each n with its neighbours
        const size_t GROUPS[] = {1, 2047, 2048, 2049, 3121, 6144, 6145, 12484};
        const int OVERRIDES[] = {0, 1, 1024, 20000};            // 20000: above every group count here
        for (size_t gr : GROUPS)
            for (size_t n : {gr * 21 - 1, gr * 21, gr * 21 + 1})
                for (int ov : OVERRIDES)
                    for (bool tagged : {true, false}) check_queue(n, tagged, ov);
    }
    const size_t NS[] = {1, 3, 64, 65, 257}, LENS[] = {0, 1, 31, 32, 40}, SMALL[] = {0, 1, 2};
    const size_t FIXED_G2_MAX = 8;                              // C12381_FIXED_G2_MAX: k = nmsg + 2 of the PS aggregate goes up to it
    for (size_t n : NS) {
        for (size_t nblk : SMALL) {                             // BBS+ wire: bbs_wire_pub_kernel, the decompression kernels, bbs_wire_prep_kernel
            const size_t npub1 = 2 + nblk;
            CARVE(bbs_wire_slab, bbs_wire_layout, n, nblk);
            check("bbs_wire", base, s.bytes, sized, 0, {{"p49", s.p49, 49 * npub1}, {"p97", s.p97, 2 * 97}, {"p96", s.p96, 96 * npub1}, {"p192", s.p192, 2 * 192},
                  {"st1", s.st1, npub1}, {"st2", s.st2, 2}, {"a49", s.a49, 49 * n}, {"A", s.A, 96 * n}, {"x", s.x, 32 * n}, {"r", s.r, 32 * n},
                  {"m", s.m, 32 * n * nblk}, {"ss", s.ss, n}, {"sa", s.sa, n}});
            std::free(base);
        }
        for (size_t nmsg : SMALL) {                             // BBS+ aggregate: n + nmsg + 2 terms of 96 bytes, two results
            const size_t terms = n + nmsg + 2;
            CARVE(bbs_aggregate_slab, bbs_aggregate_layout, terms);
            check("bbs_aggregate", base, s.bytes, sized, 0, {{"pts", s.pts, 96 * terms}, {"p12", s.p12, 2 * 96}});
            std::free(base);
        }
        for (size_t units : SMALL) {                            // PS verify: 2 + units key points, ps_wire_prep_kernel's 32 * n * units scalars
            const size_t npub = 2 + units;
            CARVE(ps_wire_slab, ps_wire_layout, n, units);
            check("ps_wire", base, s.bytes, sized, 0, {{"p192", s.p192, 192 * npub}, {"stp", s.stp, npub}, {"s49", s.s49, 98 * n}, {"s96", s.s96, 2 * 96 * n},
                  {"m", s.m, 32 * n * units}, {"st", s.st, 2 * n}});
            std::free(base);
        }
        {                                                       // PS sign: ps_generator_kernel, ps_sign_prep_kernel (64 bytes per signature, one key byte)
            CARVE(ps_sign_slab, ps_sign_layout, n);
            check("ps_sign", base, s.bytes, sized, 0, {{"gen", s.gen, 96}, {"key", s.key, 1}, {"sc", s.sc, 64 * n}});
            std::free(base);
        }
        {                                                       // PS randomize: 2 n decoded records, ps_randomize_prep_kernel, 2 n statuses
            CARVE(ps_randomize_slab, ps_randomize_layout, n);
            check("ps_randomize", base, s.bytes, sized, 0, {{"s96", s.s96, 2 * 96 * n}, {"sc", s.sc, 64 * n}, {"st", s.st, 2 * n}});
            std::free(base);
        }
        for (size_t nmsg = 0; nmsg + 2 <= FIXED_G2_MAX; ++nmsg) {   // PS aggregate: k sums, one column of n scalars
            const size_t k = nmsg + 2;
            CARVE(ps_aggregate_slab, ps_aggregate_layout, n, k);
            check("ps_aggregate", base, s.bytes, sized, 0, {{"sum", s.sum, 96 * k}, {"col", s.col, 32 * n}});
            std::free(base);
        }
        for (size_t msg_len : LENS) {                           // bbs04: behind the public block; the transcript is (msg_len + 919) bytes per signature
            {
                CARVE(bbs04_slab, bbs04_layout, n, msg_len);
                check("bbs04", base, s.bytes, sized, BBS04_PUB_BYTES, {{"t49", s.t49, 3 * 49 * n}, {"t96", s.t96, 6 * 96 * n}, {"sc", s.sc, 13 * 32 * n},
                      {"c32", s.c32, 32 * n}, {"st", s.st, n}, {"st_t", s.st_t, 3 * n}, {"r49", s.r49, 4 * 49 * n}, {"p96", s.p96, 2 * 96 * n},
                      {"gt", s.gt, 576 * n}, {"tr", s.tr, (msg_len + 919) * n}});
                const bbs04_public pub(base);                   // 4 x 49 and 2 x 97 wire bytes, 4 x 96 and 2 x 192 decoded, 6 statuses
                check("bbs04_public", base, BBS04_PUB_BYTES, BBS04_PUB_BYTES, 0, {{"wire_g1", pub.wire_g1, 4 * 49}, {"wire_g2", pub.wire_g2, 2 * 97},
                      {"g1", pub.g1, 4 * 96}, {"g2_w", pub.g2_w, 2 * 192}, {"st", pub.st, 6}});
                if (pub.h != pub.g1 + 96 || pub.u != pub.g1 + 192 || pub.v != pub.g1 + 288) { std::fprintf(stderr, "bbs04_public: g1, h, u, v not one array\n"); return 1; }
                std::free(base);
            }
            {
                CARVE(bbs04_sign_slab, bbs04_sign_layout, n, msg_len);
                check("bbs04_sign", base, s.bytes, sized, BBS04_PUB_BYTES, {{"a49", s.a49, 49 * n}, {"a96", s.a96, 96 * n}, {"st_a", s.st_a, n},
                      {"sc", s.sc, 12 * 32 * n}, {"t49", s.t49, 3 * 49 * n}, {"t96", s.t96, 3 * 96 * n}, {"r49", s.r49, 4 * 49 * n}, {"p96", s.p96, 2 * 96 * n},
                      {"gt", s.gt, 576 * n}, {"tr", s.tr, (msg_len + 919) * n}});
                std::free(base);
            }
        }
        {
            CARVE(bbs04_issue_slab, bbs04_issue_layout, n);
            check("bbs04_issue", base, s.bytes, sized, BBS04_PUB_BYTES, {{"inv", s.inv, 32 * n}, {"a49", s.a49, 49 * n}});
            std::free(base);
        }
    }
    std::printf("host layouts ok: %d slabs\n", g_checked);
    return 0;
}
