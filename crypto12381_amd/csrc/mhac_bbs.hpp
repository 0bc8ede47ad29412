// Per-lane scalar and byte work of the MHAC-bbs credential entries (examples/MHAC-bbs/src/cred_pres.cpp, verify_pres.cpp of the reference), host-
// and device-compilable like ac_bbs.hpp (tests/host_sim/mhac_bbs.cpp runs it on the CPU under C12381_CHECK_BOUNDS):
//   mhac_bbs_derive          Prv, Rev -> Pub, Hid, HidPub, RevPub and the positions pres needs, with the argument checks
//   mhac_bbs_verify_list     the base list of verify's C_hid: h[Prv[ii]] in the caller's order, then h[HidPub[ii]] ascending
//   mhac_bbs_pres_list       the base list of pres' U: h[Hid[ii]] ascending, then t - 1 times h[Prv[ii]] — exactly the reference's terms
//   mhac_bbs_transcript      U | A_ | B_ | the revealed public values as 48-byte fields; c is ac_bbs_challenge of it
//   mhac_bbs_rnd_*           where r, alpha, beta_share, beta_share_j, gamma_share sit in a lane's rnd
//   mhac_bbs_responses       zr, ze, z[ii], zhp[ii] of pres
// Values travel as CANONICAL residues (fr words, not Montgomery form) unless a name or a comment says otherwise, as in ac_bbs.hpp.
#pragma once
#include "ac_bbs.hpp"   // ac_bbs_order, ac_bbs_encode49, ac_bbs_challenge, ac_bbs_pres_random, fr_mont_to_canonical; ps.hpp: zp_parse48

namespace c12381 {

constexpr size_t MHAC_BBS_FIXED_BYTES = 242;          // Pres.fixed_part = A_ | B_ | ch | zr | ze
constexpr size_t MHAC_BBS_POINT_BYTES = 3 * 49;       // U | A_ | B_ in front of the revealed values of the transcript
constexpr size_t MHAC_BBS_MAX_ATTR = AC_BBS_MAX_ATTR; // C12381_G1_FIXED_SUM_MAX: one fixed-base table per position of a base list
constexpr size_t MHAC_BBS_T_MAX = 8;                  // C12381_MHAC_T_MAX

// The index sets of a batch as the reference derives them (cred_pres.cpp:33-52, verify_pres.cpp:27-35).  Positions are below 32.
struct mhac_bbs_sets {
    uint8_t m, nPrv, nRev, nPub, nHid, nHidPub, nRevPub, unused;
    uint8_t prv[MHAC_BBS_MAX_ATTR];      // Prv in the caller's order
    uint8_t hid[MHAC_BBS_MAX_ATTR];      // Hid = the indices below m that are not in Rev, ascending
    uint8_t hidpub[MHAC_BBS_MAX_ATTR];   // HidPub = Hid without Prv, ascending
    uint8_t revpub[MHAC_BBS_MAX_ATTR];   // I_Pub_in_Rev: the positions of Pub whose attribute is in Rev, ascending
    uint8_t hp_hid[MHAC_BBS_MAX_ATTR];   // I_Hid_in_HidPub: the position of HidPub[ii] in Hid
    uint8_t hp_pub[MHAC_BBS_MAX_ATTR];   // I_Pub_in_HidPub: the position of HidPub[ii] in Pub
};

// Returns false for m = 0, m > MHAC_BBS_MAX_ATTR, an index >= m, a repeated index in either set, or an index in both sets; s is complete
// exactly when it returns true.  prv / rev may be null when their count is 0.
C12381_HD bool mhac_bbs_derive(mhac_bbs_sets& s, size_t m, const uint32_t* prv, size_t nPrv, const uint32_t* rev, size_t nRev) {
    if (m == 0 || m > MHAC_BBS_MAX_ATTR || nPrv > m || nRev > m) return false;
    uint32_t in_prv = 0, in_rev = 0;
    for (size_t k = 0; k < MHAC_BBS_MAX_ATTR; ++k) s.prv[k] = s.hid[k] = s.hidpub[k] = s.revpub[k] = s.hp_hid[k] = s.hp_pub[k] = 0;
    for (size_t k = 0; k < nPrv; ++k) {
        const uint32_t i = prv[k];
        if (i >= m || ((in_prv >> i) & 1u)) return false;
        in_prv |= 1u << i;
        s.prv[k] = (uint8_t)i;
    }
    for (size_t k = 0; k < nRev; ++k) {
        const uint32_t i = rev[k];
        if (i >= m || ((in_rev >> i) & 1u)) return false;
        in_rev |= 1u << i;
    }
    if (in_prv & in_rev) return false;
    size_t nPub = 0, nHid = 0, nHidPub = 0, nRevPub = 0;
    for (size_t i = 0; i < m; ++i) {
        const bool p = (in_prv >> i) & 1u, r = (in_rev >> i) & 1u;
        if (!r && !p) { s.hidpub[nHidPub] = (uint8_t)i; s.hp_hid[nHidPub] = (uint8_t)nHid; s.hp_pub[nHidPub] = (uint8_t)nPub; ++nHidPub; }
        if (r) s.revpub[nRevPub++] = (uint8_t)nPub;          // Rev and Prv are disjoint: a revealed index is a position of Pub
        if (!r) s.hid[nHid++] = (uint8_t)i;
        if (!p) ++nPub;
    }
    s.m = (uint8_t)m; s.nPrv = (uint8_t)nPrv; s.nRev = (uint8_t)nRev; s.nPub = (uint8_t)nPub; s.nHid = (uint8_t)nHid;
    s.nHidPub = (uint8_t)nHidPub; s.nRevPub = (uint8_t)nRevPub; s.unused = 0;
    return true;
}

// verify_pres.cpp:39-42: prod_ii h[Prv[ii]]^z[ii] * prod_ii h[HidPub[ii]]^zhp[ii]; returns the length nPrv + nHidPub = nHid <= m
C12381_HD size_t mhac_bbs_verify_list(ac_bbs_order& o, const mhac_bbs_sets& s) {
    size_t k = 0;
    for (size_t ii = 0; ii < s.nPrv; ++ii) o.at[k++] = s.prv[ii];
    for (size_t ii = 0; ii < s.nHidPub; ++ii) o.at[k++] = s.hidpub[ii];
    const size_t nb = k;
    for (; k < AC_BBS_MAX_ATTR; ++k) o.at[k] = 0;
    return nb;
}
// cred_pres.cpp:73-80: prod_(ii < nHid) h[Hid[ii]]^bj[ii], then for k = 1 .. t - 1 prod_(ii < nPrv) h[Prv[ii]]^b[(k - 1) nPrv + ii].  Returns the
// length nHid + (t - 1) nPrv, which the caller refuses above MHAC_BBS_MAX_ATTR; o holds the positions below that bound.
C12381_HD size_t mhac_bbs_pres_list_len(const mhac_bbs_sets& s, size_t t) { return (size_t)s.nHid + (t - 1) * s.nPrv; }
C12381_HD size_t mhac_bbs_pres_list(ac_bbs_order& o, const mhac_bbs_sets& s, size_t t) {
    const size_t total = mhac_bbs_pres_list_len(s, t);
    for (size_t k = 0; k < AC_BBS_MAX_ATTR; ++k) {
        uint8_t at = 0;
        if (k < s.nHid) at = s.hid[k];
        else if (k < total) at = s.prv[(k - s.nHid) % s.nPrv];
        o.at[k] = at;
    }
    return total;
}

// hash(U, A_, B_, pub_a[ii] (ii in I_Pub_in_Rev)) (cred_pres.cpp:86, verify_pres.cpp:45): the three 49-byte encodings, then field perm[k] of
// pub48 (perm = nullptr: field k) for k < count, 48 bytes each as serialize(Zp) writes a value below r
C12381_HD size_t mhac_bbs_transcript_bytes(size_t count) { return MHAC_BBS_POINT_BYTES + 48 * count; }
C12381_HD void mhac_bbs_transcript(uint8_t* out, const uint8_t* u49, const uint8_t* a49, const uint8_t* b49, const uint8_t* pub48, size_t count,
                                   const uint8_t* perm) {
#pragma unroll 1
    for (int b = 0; b < 49; ++b) { out[b] = u49[b]; out[49 + b] = a49[b]; out[98 + b] = b49[b]; }
#pragma unroll 1
    for (size_t k = 0; k < count; ++k) {
        const uint8_t* f = pub48 + 48 * (perm ? perm[k] : k);
#pragma unroll 1
        for (int b = 0; b < 48; ++b) out[MHAC_BBS_POINT_BYTES + 48 * k + b] = f[b];
    }
}

// A lane's rnd: r, alpha, beta_share[(t - 1) nPrv], beta_share_j[nHid], gamma_share[t] — the order the reference draws them in
C12381_HD size_t mhac_bbs_rnd_count(const mhac_bbs_sets& s, size_t t) { return 2 + (t - 1) * s.nPrv + s.nHid + t; }
C12381_HD size_t mhac_bbs_rnd_beta(const mhac_bbs_sets&, size_t y) { return 2 + y; }
C12381_HD size_t mhac_bbs_rnd_betaj(const mhac_bbs_sets& s, size_t t, size_t ii) { return 2 + (t - 1) * s.nPrv + ii; }
C12381_HD size_t mhac_bbs_rnd_gamma(const mhac_bbs_sets& s, size_t t, size_t k) { return 2 + (t - 1) * s.nPrv + s.nHid + k; }

// a b for canonical a, b
C12381_HD void mhac_bbs_mul(fr& r, const fr& a, const fr& b) {
    fr r2, am;
    fr_set_words(r2, FR_R2);
    fr_mul(am, a, r2);
    fr_mul(r, am, b);
}
// The responses of one lane (cred_pres.cpp:87-105, j = 0), from fields that passed the range check:
//   zr = alpha + ch r                    ze = sum_k ( gamma[k] + ch (-e_k lambda_k) ), -e the Zp negation (-0 = 0)
//   z[ii] = bj[ii] + ch r a_0[ii] lambda_0 + sum_(k >= 1) ( b[(k - 1) nPrv + ii] + ch r a_k[ii] lambda_k )        bj indexed by ii itself
//   zhp[ii] = bj[hp_hid[ii]] + ch pub[hp_pub[ii]] r
// rnd: the lane's scalars; lam48, eshare48: t fields; ashare48: t x nPrv fields party-major; pub48: the nPub fields of the lane.
// zr48, ze48: one field each; z48: nPrv fields; zhp48: nHidPub fields.
C12381_HD void mhac_bbs_responses(const mhac_bbs_sets& s, size_t t, const fr& c_mont, const uint8_t* rnd, const uint8_t* lam48, const uint8_t* eshare48,
                                  const uint8_t* ashare48, const uint8_t* pub48, uint8_t* zr48, uint8_t* ze48, uint8_t* z48, uint8_t* zhp48) {
    fr r, v, w, rc, rc_mont, r2, acc;
    fr_set_words(r2, FR_R2);
    ac_bbs_pres_random(r, rnd, 0);
    ac_bbs_pres_random(v, rnd, 1);
    fr_mul(rc, c_mont, r);                           // Montgomery x canonical = canonical
    fr_add(acc, v, rc);
    store_be48(zr48, acc);
    fr_mul(rc_mont, rc, r2);
#pragma unroll 1
    for (size_t k = 0; k < t; ++k) {
        fr e, lam, term;
        zp_parse48(e, eshare48 + 48 * k);
        zp_parse48(lam, lam48 + 48 * k);
        fr_neg(w, e);
        mhac_bbs_mul(v, w, lam);
        fr_mul(term, c_mont, v);
        ac_bbs_pres_random(v, rnd, mhac_bbs_rnd_gamma(s, t, k));
        fr_add(term, term, v);
        if (k == 0) acc = term; else fr_add(acc, acc, term);
    }
    store_be48(ze48, acc);
#pragma unroll 1
    for (size_t ii = 0; ii < s.nPrv; ++ii) {
        ac_bbs_pres_random(acc, rnd, mhac_bbs_rnd_betaj(s, t, ii));
#pragma unroll 1
        for (size_t k = 0; k < t; ++k) {
            fr a, lam, term;
            zp_parse48(a, ashare48 + 48 * (k * s.nPrv + ii));
            zp_parse48(lam, lam48 + 48 * k);
            mhac_bbs_mul(v, a, lam);
            fr_mul(term, rc_mont, v);
            fr_add(acc, acc, term);
            if (k) { ac_bbs_pres_random(v, rnd, mhac_bbs_rnd_beta(s, (k - 1) * s.nPrv + ii)); fr_add(acc, acc, v); }
        }
        store_be48(z48 + 48 * ii, acc);
    }
#pragma unroll 1
    for (size_t ii = 0; ii < s.nHidPub; ++ii) {
        fr a, term;
        ac_bbs_pres_random(acc, rnd, mhac_bbs_rnd_betaj(s, t, s.hp_hid[ii]));
        zp_parse48(a, pub48 + 48 * s.hp_pub[ii]);
        fr_mul(term, rc_mont, a);
        fr_add(acc, acc, term);
        store_be48(zhp48 + 48 * ii, acc);
    }
}

}  // namespace c12381
