// TEST HARNESS (CPU): the per-lane scalar and byte work of the MHAC-bbs entries (csrc/mhac_bbs.hpp) compiled for the host with
// C12381_CHECK_BOUNDS.  Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/mhac_bbs.hpp"

using namespace c12381;

// The sets of (m, prv, rev): counts[7] = m, nPrv, nRev, nPub, nHid, nHidPub, nRevPub; lists[6 x 32] = prv, hid, hidpub, revpub, hp_hid, hp_pub;
// vlist / plist: the base lists of verify and of pres with t parties, lens[2] their lengths (the pres length is reported even above 32, where the
// entry refuses).  Returns 1, or 0 where the entries return C12381_E_ARG for the sets.
extern "C" int sim_mhac_bbs_sets(size_t m, const uint32_t* prv, size_t nPrv, const uint32_t* rev, size_t nRev, size_t t, uint8_t* counts, uint8_t* lists,
                                 uint8_t* vlist, uint8_t* plist, size_t* lens) {
    mhac_bbs_sets s;
    if (!mhac_bbs_derive(s, m, prv, nPrv, rev, nRev)) return 0;
    const uint8_t c[7] = {s.m, s.nPrv, s.nRev, s.nPub, s.nHid, s.nHidPub, s.nRevPub};
    std::memcpy(counts, c, 7);
    const uint8_t* l[6] = {s.prv, s.hid, s.hidpub, s.revpub, s.hp_hid, s.hp_pub};
    for (int i = 0; i < 6; ++i) std::memcpy(lists + 32 * i, l[i], 32);
    ac_bbs_order o;
    lens[0] = mhac_bbs_verify_list(o, s);
    std::memcpy(vlist, o.at, 32);
    lens[1] = mhac_bbs_pres_list(o, s, t);
    std::memcpy(plist, o.at, 32);
    return 1;
}
// the transcript of one lane from its decoded points and `count` fields of pub48 (perm: which fields, or null) — tr: 147 + 48 count bytes and 3
// bytes of padding (sha3.hpp reads whole words) — and c as 32 canonical bytes
extern "C" int sim_mhac_bbs_challenge(const uint8_t* u96, const uint8_t* a96, const uint8_t* b96, const uint8_t* pub48, size_t count, const uint8_t* perm,
                                      uint8_t* tr, uint8_t* c32) {
    uint8_t e[3][49];
    ac_bbs_encode49(e[0], u96); ac_bbs_encode49(e[1], a96); ac_bbs_encode49(e[2], b96);
    mhac_bbs_transcript(tr, e[0], e[1], e[2], pub48, count, perm);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, tr, mhac_bbs_transcript_bytes(count));
    fr_mont_to_canonical(c, c_mont);
    store_be32(c32, c);
    return 0;
}
// mhac_bbs_responses of one lane: c32 below r; out = zr | ze (96 bytes), z48, zhp48
extern "C" int sim_mhac_bbs_responses(size_t m, const uint32_t* prv, size_t nPrv, const uint32_t* rev, size_t nRev, size_t t, const uint8_t* c32,
                                      const uint8_t* rnd, const uint8_t* lam48, const uint8_t* eshare48, const uint8_t* ashare48, const uint8_t* pub48,
                                      uint8_t* zrze96, uint8_t* z48, uint8_t* zhp48) {
    mhac_bbs_sets s;
    if (!mhac_bbs_derive(s, m, prv, nPrv, rev, nRev)) return 1;
    uint32_t k[8];
    fr c_mont;
    words_from_be32(k, c32);
    fr_from_words(c_mont, k);
    mhac_bbs_responses(s, t, c_mont, rnd, lam48, eshare48, ashare48, pub48, zrze96, zrze96 + 48, z48, zhp48);
    return (int)mhac_bbs_rnd_count(s, t);
}
