// TEST HARNESS (CPU): the per-lane scalar and byte work of the AC-rbbs entries (csrc/ac_rbbs.hpp) compiled for the host with
// C12381_CHECK_BOUNDS.  Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/ac_rbbs.hpp"

using namespace c12381;

// q_i for every i < count from the nI disclosed fields aI48 (48 nI bytes and 3 bytes of padding: sha3.hpp reads whole words): q32[32 i] canonical
extern "C" int sim_ac_rbbs_q(const uint8_t* aI48, size_t nI, size_t count, uint8_t* q32) {
    uint64_t pre[25];
    ac_rbbs_q_prefix(pre, aI48, nI);
    for (size_t i = 0; i < count; ++i) {
        fr q_mont, q;
        ac_rbbs_q(q_mont, pre, aI48, nI, i);
        fr_mont_to_canonical(q, q_mont);
        store_be32(q32 + 32 * i, q);
    }
    return 0;
}
// the transcript of one lane from its message and five decoded points in the order A_, B_, C_J_, D_, U (tr: msg_len + 245 bytes and 3 bytes of
// padding) and c as 32 canonical bytes
extern "C" int sim_ac_rbbs_challenge(const uint8_t* msg, size_t msg_len, const uint8_t* p96x5, uint8_t* tr, uint8_t* c32) {
    uint8_t e[5][49];
    const uint8_t* ep[5];
    for (int k = 0; k < 5; ++k) { ac_bbs_encode49(e[k], p96x5 + 96 * k); ep[k] = e[k]; }
    ac_rbbs_transcript(tr, msg, msg_len, ep);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, tr, ac_rbbs_transcript_bytes(msg_len));
    fr_mont_to_canonical(c, c_mont);
    store_be32(c32, c);
    return 0;
}
// the plan of redact: returns 0 where the entry returns C12381_E_ARG, else 1 and y[32], acol[16], the counts total, d_first, nD, cj_first
extern "C" int sim_ac_rbbs_plan(size_t nattr, const uint32_t* idx, size_t nI, uint8_t* y32, uint8_t* acol16, uint8_t* counts4) {
    ac_rbbs_plan p;
    if (!ac_rbbs_redact_plan(p, nattr, idx, nI)) return 0;
    std::memcpy(y32, p.y, 32);
    std::memcpy(acol16, p.acol, 16);
    counts4[0] = p.total; counts4[1] = p.d_first; counts4[2] = p.nD; counts4[3] = p.cj_first;
    return 1;
}
// the exponents of redact for one lane as the kernel computes them: e32[32 k] and kept[k] for EVERY k < 2 nattr, from the lane's attributes
// (nattr fields below r) and q32 (nI values in the order of idx, 32 bytes each)
extern "C" int sim_ac_rbbs_conv(size_t nattr, const uint32_t* idx, size_t nI, const uint8_t* attr48, const uint8_t* q32, uint8_t* e32, uint8_t* kept) {
    ac_rbbs_plan p;
    if (!ac_rbbs_redact_plan(p, nattr, idx, nI)) return 1;
    for (size_t k = 0; k < 2 * nattr; ++k) {
        fr e;
        kept[k] = ac_rbbs_conv(e, k, nattr, p.idx, nI, p.in_I, q32, 32, attr48) ? 1 : 0;
        store_be32(e32 + 32 * k, e);
    }
    return 0;
}
