// TEST HARNESS (CPU): polynomial, the Lagrange coefficients, the base lists and the rnd offsets of the MHAC-bbs issuance entries
// (csrc/mhac_iss.hpp) compiled for the host with C12381_CHECK_BOUNDS.  Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/mhac_iss.hpp"

using namespace c12381;

// polynomial(x, a0, a) with a0 = scalar `first_a0` and the coefficients = scalars [first, first + count) of rnd (32-byte values, reduced first);
// out48: the canonical result as a 48-byte field
extern "C" int sim_mhac_iss_polynomial(uint32_t x, const uint8_t* rnd, size_t first_a0, size_t first, size_t count, uint8_t* out48) {
    fr a0, v;
    ac_bbs_pres_random(a0, rnd, first_a0);
    mhac_iss_polynomial_rnd(v, x, a0, rnd, first, count);
    store_be48(out48, v);
    return 0;
}
// lambda of the party set S (x = S + 1) as t 48-byte fields, and the set as the kernels receive it; 0 where the entries return C12381_E_ARG
extern "C" int sim_mhac_iss_lambda(const uint32_t* S, size_t t, size_t nparties, uint8_t* lam48, uint8_t* set8) {
    mhac_iss_parties_set set;
    mhac_iss_lambda lam;
    uint32_t x[MHAC_BBS_T_MAX];
    if (!mhac_iss_parties(set, x, S, t, nparties)) return 0;
    mhac_iss_lagrange(lam, x, t);
    for (size_t k = 0; k < MHAC_BBS_T_MAX; ++k) {
        fr l;
        fr_set_words(l, lam.w[k]);
        store_be48(lam48 + 48 * k, l);
    }
    std::memcpy(set8, set.at, MHAC_BBS_T_MAX);
    return 1;
}
extern "C" int sim_mhac_iss_shape_ok(size_t t, size_t nparties) { return mhac_iss_shape_ok(t, nparties) ? 1 : 0; }
// The base lists of (m, prv, rev, pub_idx): alist / lens[0] attr's (the sets of (m, prv, {})), plist / lens[1] iss' (0xff.. and lens[1] = ~0 where
// pub_idx is refused), tlist + tat / lens[2] type's.  Returns 0 where derive refuses the sets of type.
extern "C" int sim_mhac_iss_lists(size_t m, const uint32_t* prv, size_t nPrv, const uint32_t* rev, size_t nRev, const uint32_t* pub_idx, size_t nPub,
                                  uint8_t* alist, uint8_t* plist, uint8_t* tlist, uint8_t* tat, size_t* lens) {
    mhac_bbs_sets s;
    ac_bbs_order o;
    if (!mhac_bbs_derive(s, m, prv, nPrv, nullptr, 0)) return 0;
    lens[0] = mhac_iss_attr_list(o, s);
    std::memcpy(alist, o.at, 32);
    if (mhac_iss_pub_list(o, m, pub_idx, nPub)) { lens[1] = nPub; std::memcpy(plist, o.at, 32); } else { lens[1] = ~(size_t)0; std::memset(plist, 0xff, 32); }
    if (!mhac_bbs_derive(s, m, prv, nPrv, rev, nRev)) return 0;
    mhac_iss_type_plan p;
    lens[2] = mhac_iss_type_list(p, s);
    std::memcpy(tlist, p.list.at, 32);
    std::memcpy(tat, p.at, 32);
    return 1;
}
// counts[0] = attr's scalars per credential, counts[1 + ii] = where the coefficients of private attribute ii start (ii < nPrv), counts[33] = iss'
// scalars per credential, counts[34] = where its coefficients start
extern "C" void sim_mhac_iss_rnd(size_t m, size_t nPrv, size_t t, size_t* counts) {
    counts[0] = mhac_iss_attr_rnd_count(m, nPrv, t);
    for (size_t ii = 0; ii < nPrv; ++ii) counts[1 + ii] = mhac_iss_attr_rnd_coeff(m, t, ii);
    counts[33] = mhac_iss_iss_rnd_count(t);
    counts[34] = mhac_iss_iss_rnd_coeff();
}
