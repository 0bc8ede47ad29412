// TEST HARNESS (CPU): the per-lane scalar work of the AC issuance entries (csrc/ac_issue.hpp) compiled for the host with C12381_CHECK_BOUNDS.
// Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/ac_issue.hpp"

using namespace c12381;

// parse<Zp> of one 48-byte field: 1 when it is below r; low32: the 32 bytes a column would receive
extern "C" int sim_ac_issue_range(const uint8_t* f48, uint8_t* low32) {
    fr v;
    const bool ok = zp_parse48(v, f48);
    store_be32(low32, v);
    return ok ? 1 : 0;
}
// the range check of sk: count fields
extern "C" int sim_ac_issue_sk(const uint8_t* sk48, size_t count) {
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    return ac_issue_sk(sk, sk48, count) ? 1 : 0;
}
// rnd mod r as a 48-byte field
extern "C" void sim_ac_issue_random(const uint8_t* rnd32, uint8_t* out48) {
    fr v;
    ac_issue_random(v, rnd32);
    store_be48(out48, v);
}
// ym and y^(nattr+1) (canonical) as 48-byte fields; y48 and the attributes are taken as they come (low 32 bytes)
extern "C" void sim_ac_issue_horner(const uint8_t* y48, const uint8_t* attr48, size_t nattr, uint8_t* ym48, uint8_t* pow48) {
    fr y, y_mont, ym, p_mont, p;
    zp_parse48(y, y48);
    ac_issue_to_mont(y_mont, y);
    ac_issue_horner(ym, y_mont, attr48, nattr);
    ac_issue_power(p_mont, y_mont, nattr);
    fr_mont_to_canonical(p, p_mont);
    store_be48(ym48, ym);
    store_be48(pow48, p);
}
// One AC-bbs / AC-rbbs lane j of n: cols = nattr columns of n scalars, w32 / d32 = n scalars each.  Returns the lane's status.
extern "C" int sim_ac_issue_bbs_lane(const uint8_t* sk48, const uint8_t* attr48, size_t nattr, const uint8_t* rnd32, size_t n, size_t j, uint8_t* cols,
                                     uint8_t* w32, uint8_t* d32) {
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    ac_issue_sk(sk, sk48, 1);
    return ac_issue_bbs_lane(cols + 32 * j, 32 * n, w32 + 32 * j, d32 + 32 * j, sk[0], attr48, nattr, rnd32) ? 1 : 0;
}
// One AC-rps lane j of n: cols as above, al32 = n scalars, sc2 = the two columns x + ym | alpha y^(nattr+1)
extern "C" int sim_ac_issue_rps_lane(const uint8_t* sk96, const uint8_t* attr48, size_t nattr, const uint8_t* rnd32, size_t n, size_t j, uint8_t* cols,
                                     uint8_t* al32, uint8_t* sc2) {
    fr sk[AC_ISSUE_RPS_SK_FIELDS];
    ac_issue_sk(sk, sk96, AC_ISSUE_RPS_SK_FIELDS);
    return ac_issue_rps_lane(cols + 32 * j, 32 * n, al32 + 32 * j, sc2 + 32 * j, sc2 + 32 * (n + j), sk[0], sk[1], attr48, nattr, rnd32) ? 1 : 0;
}
