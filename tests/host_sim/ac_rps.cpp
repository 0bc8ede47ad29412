// TEST HARNESS (CPU): the per-lane scalar and byte work of the AC-rps entries (csrc/ac_rps.hpp) compiled for the host with
// C12381_CHECK_BOUNDS.  Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/ac_rps.hpp"

using namespace c12381;

// q_k for every k <= nI as the kernels compute it: the prefix is built in buf (195 + 56 nI bytes and 3 bytes of padding: sha3.hpp reads whole
// words) from the two 96-byte G1 points, the 192-byte G2 point, idx and the nI disclosed fields aI48; q32[32 k] canonical.  Returns the tail length.
extern "C" int sim_ac_rps_q(const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* ts192, size_t nattr, const uint8_t* idx, size_t nI, const uint8_t* aI48,
                            uint8_t* buf, uint8_t* q32) {
    uint8_t e1[49], e2[49], e3[97];
    ac_bbs_encode49(e1, s1_96);
    ac_bbs_encode49(e2, s2_96);
    ac_rps_encode97(e3, ts192);
    ac_rps_q_head(buf, e1, e2, e3, idx, nI);
    ac_rps_copy(ac_rps_q_fields(buf, nI), aI48, 48 * nI);
    uint64_t pre[25];
    ac_rps_q_absorb(pre, buf, nI);
    for (size_t k = 0; k <= nI; ++k) {
        fr q_mont, q;
        ac_rps_q(q_mont, pre, buf, nI, k < nI ? idx[k] : nattr);
        fr_mont_to_canonical(q, q_mont);
        store_be32(q32 + 32 * k, q);
    }
    return (int)ac_rps_q_tail_bytes(nI);
}
// the Schnorr transcript of one lane from its three decoded points sigma1_, C, C0 (tr: 147 bytes and 3 bytes of padding) and c0 as 32 canonical bytes
extern "C" int sim_ac_rps_c0(const uint8_t* p96x3, uint8_t* tr, uint8_t* c32) {
    uint8_t e[3][49];
    for (int k = 0; k < 3; ++k) ac_bbs_encode49(e[k], p96x3 + 96 * k);
    ac_bbs_transcript(tr, nullptr, 0, e[0], e[1], e[2]);
    fr c_mont, c;
    ac_bbs_challenge(c_mont, tr, AC_RPS_C0_BYTES);
    fr_mont_to_canonical(c, c_mont);
    store_be32(c32, c);
    return 0;
}
// the plan: returns 0 where the entry returns C12381_E_ARG, else 1 and y[32], total
extern "C" int sim_ac_rps_plan(size_t nattr, const uint32_t* idx, size_t nI, int cross, uint8_t* y32, uint8_t* total) {
    ac_rps_plan p;
    if (!ac_rps_pres_plan(p, nattr, idx, nI, cross != 0)) return 0;
    std::memcpy(y32, p.y, 32);
    *total = p.total;
    return 1;
}
// the exponents of the cross terms for one lane as the kernel computes them: e32[32 k] and kept[k] for EVERY k <= 2 nattr, from the lane's attributes
// (nattr fields below r) and q32 (nI + 1 values in the order of Ip, 32 bytes each)
extern "C" int sim_ac_rps_conv(size_t nattr, const uint32_t* idx, size_t nI, const uint8_t* attr48, const uint8_t* q32, uint8_t* e32, uint8_t* kept) {
    ac_rps_plan p;
    if (!ac_rps_pres_plan(p, nattr, idx, nI, false)) return 1;
    for (size_t k = 0; k <= 2 * nattr; ++k) {
        fr e;
        kept[k] = ac_rps_conv(e, k, nattr, p.idx, nI, p.in_I, q32, 32, attr48) ? 1 : 0;
        store_be32(e32 + 32 * k, e);
    }
    return 0;
}
// s0 = rho + (-c0) z as the finish kernel computes it, all 32 canonical big-endian bytes
extern "C" int sim_ac_rps_s0(const uint8_t* c32, const uint8_t* z32, const uint8_t* rho32, uint8_t* s32) {
    uint32_t k8[8];
    fr c_mont, negc, z, rho, zc, s0;
    words_from_be32(k8, c32); fr_from_words(c_mont, k8);
    words_from_be32(k8, z32); fr_set_words(z, k8);
    words_from_be32(k8, rho32); fr_set_words(rho, k8);
    fr_neg(negc, c_mont);
    fr_mul(zc, negc, z);
    fr_add(s0, rho, zc);
    store_be32(s32, s0);
    return 0;
}
