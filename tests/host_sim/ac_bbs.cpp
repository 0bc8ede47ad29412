// TEST HARNESS (CPU): the per-lane scalar and byte work of the AC-bbs entries (csrc/ac_bbs.hpp) compiled for the host with
// C12381_CHECK_BOUNDS.  Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/ac_bbs.hpp"

using namespace c12381;

// the base order of the disclosure set idx: out32[k] = attribute index at position k; returns 1, or 0 where the entries return C12381_E_ARG
extern "C" int sim_ac_bbs_order(size_t nattr, const uint32_t* idx, size_t nI, uint8_t* out32) {
    ac_bbs_order o;
    if (!ac_bbs_base_order(o, nattr, idx, nI)) return 0;
    std::memcpy(out32, o.at, sizeof o.at);
    return 1;
}
// record k of block243 -> cols[49 (k n + at)], as the kernels lay the columns out
extern "C" int sim_ac_bbs_split3(size_t n, size_t at, const uint8_t* block243, uint8_t* cols) {
    ac_bbs_split3(cols, 49 * n, at, block243);
    return 0;
}
// lane j of n: `count` fields at f48 + 48 count j -> cols[32 (k n + j)], field perm[k] for column k when perm is given; ok[j] = the range check
extern "C" int sim_ac_bbs_zp_columns(size_t n, size_t count, const uint8_t* f48, const uint8_t* perm, uint8_t* cols, uint8_t* ok) {
    for (size_t j = 0; j < n; ++j) ok[j] = ac_bbs_zp_columns(cols + 32 * j, 32 * n, f48 + 48 * count * j, count, perm) ? 1 : 0;
    return 0;
}
// the transcript of one lane from its message and decoded points (tr: msg_len + 147 bytes and 3 bytes of padding: sha3.hpp reads whole words)
// and c as 32 canonical bytes
extern "C" int sim_ac_bbs_challenge(const uint8_t* msg, size_t msg_len, const uint8_t* a96, const uint8_t* b96, const uint8_t* u96, uint8_t* tr, uint8_t* c32) {
    uint8_t e[3][49];
    ac_bbs_encode49(e[0], a96); ac_bbs_encode49(e[1], b96); ac_bbs_encode49(e[2], u96);
    ac_bbs_transcript(tr, msg, msg_len, e[0], e[1], e[2]);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, tr, ac_bbs_transcript_bytes(msg_len));
    fr_mont_to_canonical(c, c_mont);
    store_be32(c32, c);
    return 0;
}
// Per lane: rnd ((3 + nJ) x 32 B, any values), c32 (below r), w48 and aJ48 (nJ fields: the hidden attributes in the order of J; below r) ->
//   st96  s, t as serialize(Zp) writes them;  u48  the nJ fields u_j;  sc128  the columns r, alpha, -w, beta the kernels multiply by
extern "C" int sim_ac_bbs_responses(size_t n, size_t nJ, const uint8_t* rnd, const uint8_t* c32, const uint8_t* w48, const uint8_t* aJ48, uint8_t* st96,
                                    uint8_t* u48, uint8_t* sc128) {
    for (size_t j = 0; j < n; ++j) {
        const uint8_t* rn = rnd + 32 * (AC_BBS_PRES_RANDOM + nJ) * j;
        fr c_mont, r, alpha, beta, w, negw, s, t, rc_mont;
        uint32_t k[8];
        words_from_be32(k, c32 + 32 * j);
        fr_from_words(c_mont, k);
        ac_bbs_pres_random(r, rn, 0); ac_bbs_pres_random(alpha, rn, 1); ac_bbs_pres_random(beta, rn, 2);
        if (!zp_parse48(w, w48 + 48 * j)) return 1;
        fr_neg(negw, w);
        ac_bbs_responses(s, t, rc_mont, c_mont, r, alpha, beta, negw);
        store_be48(st96 + 96 * j, s); store_be48(st96 + 96 * j + 48, t);
        store_be32(sc128 + 128 * j, r); store_be32(sc128 + 128 * j + 32, alpha); store_be32(sc128 + 128 * j + 64, negw); store_be32(sc128 + 128 * j + 96, beta);
        for (size_t i = 0; i < nJ; ++i) {
            fr delta, a, u;
            ac_bbs_pres_random(delta, rn, AC_BBS_PRES_RANDOM + i);
            if (!zp_parse48(a, aJ48 + 48 * (nJ * j + i))) return 1;
            ac_bbs_response_u(u, rc_mont, delta, a);
            store_be48(u48 + 48 * (nJ * j + i), u);
        }
    }
    return 0;
}
