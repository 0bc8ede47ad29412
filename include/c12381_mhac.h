/* c12381_mhac.h — the multi-holder (threshold) credential entries of the MI355X-native batched BLS12-381 backend: cred_pres and verify_pres of the
 * reference's examples/MHAC-bbs from their wire formats, in one call per batch.  Conventions, status codes, the context, the stream-ordering rules of
 * the "_dev" forms and everything c12381_ac.h says at its top about decoding and exactness are inherited: this header includes c12381_ac.h.
 */
#ifndef C12381_MHAC_H
#define C12381_MHAC_H

#include "c12381_ac.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MHAC-bbs credentials (examples/MHAC-bbs/src/cred_pres.cpp, verify_pres.cpp) from the WIRE formats ------------------------------------------ */
/* Wire layouts (examples/MHAC-bbs/include/bbs.hpp, mhac_bbs.hpp):
 *   pp_146     PublicParameters.g1_g2 = serialize(g1, g2)                    49 + 97 = 146 bytes
 *   h_49       PublicParameters.h, m records serialize(h_i)                  m x 49 bytes
 *   pk_97      PublicKey = serialize(w)                                      97 bytes
 *   crev_49    PresType.C_rev, cpub_49 PresType.C_pub, A_49 Creds.A, D_49 PresGroup.D: one 49-byte record per presentation each
 *   fixed_242  Pres.fixed_part = serialize(A_, B_, ch, zr, ze)               2 x 49 + 3 x 48 = 242 bytes per presentation
 *   z_48       Pres.z, nPrv fields per presentation; zhp_48 Pres.z_hid_pub, nHidPub fields per presentation (lane-major)
 *   values     serialize(Zp) fields of 48 bytes
 * Decoding is the library's, as in c12381_ac.h: from_bytes with the header layer's "leading 0x00 = infinity", x taken mod p, no subgroup check;
 * parse<Zp>'s range check (48 big-endian bytes below r).  Records are read bytewise: no alignment requirement on them.
 *
 * The index sets are ONE pair for the batch.  prv: nPrv indices in the caller's order — z[ii] and a_share[.][ii] belong to h[prv[ii]]; rev: nRev
 * indices, of which only membership matters.  Both are HOST arrays in both forms, parameters of the call like m, read before anything is launched.
 * Derived as the reference derives them: Pub = the ascending complement of Prv, Hid = the ascending complement of Rev, HidPub = Hid without Prv
 * (ascending), RevPub = the positions of Pub whose attribute is in Rev (ascending); nPub, nHid, nHidPub, nRevPub are their sizes.
 * C12381_E_ARG: m = 0, m > C12381_G1_FIXED_SUM_MAX, t = 0 or t > C12381_MHAC_T_MAX (pres), an index >= m, a repeated index in either set, an
 * index in both sets (the reference has no public value to hash for it, and beta_share_j[ii] of cred_pres.cpp:89 needs nHid >= nPrv), a null
 * set pointer with a non-zero count, any other null pointer that is not allowed below.  Argument errors are checked before the empty-batch rule;
 * n = 0 then returns C12381_OK and touches nothing.  Batches run in chunks of up to 2^18.
 *
 * Both entries evaluate, `^` being multiply (PAIR_G1mul, exact for EVERY curve point: h records, A, D, A_, B_, C_rev, C_pub may lie outside G1 or
 * at infinity, w outside G2) and `*` add; no verdict and no output rests on a subgroup assumption the device has not checked:
 *   ch = SHA3-512(U | A_ | B_ | pub_a at RevPub ..) mod r     hash(U, A_, B_, pub_a[ii] (ii in I_Pub_in_Rev)).to(Zp): the three points 49-byte
 *                                              compressed as hash() re-serialises the parsed ones (a leading 0x00 hashes as 49 zeros whatever
 *                                              follows, an x >= p as its residue), then the revealed values as 48-byte fields:
 *                                              147 + 48 nRevPub bytes.
 * h is parsed lazily: only the records an entry's sums use are read and decoded (verify: Prv and HidPub; pres: Hid).  g1 of pp is decoded, as
 * parse<G1, G2> does, and not used.  Sums over h run from the tables of c12381_g1_mul_fixed_sum_batch (its workspace, its routes: tables when
 * every base of the list is a point of G1 other than infinity, the generic kernel column by column otherwise).
 *
 * What the reference's formulas imply (tests/test_mhac_bbs_cases.py pins it with the builders): cred_pres indexes beta_share_j by ii in z[ii]
 * (cred_pres.cpp:89) while U carries beta_share_j[ii] on h[Hid[ii]] (:76), so an honest presentation verifies only when Hid[ii] = Prv[ii] for
 * every ii < nPrv — the reference's own test (m = 4, Prv = (0, 2), Rev = (1)) satisfies it, (Prv = (0, 2), Rev = ()) and Prv = (2, 0) do not.
 * The entries reproduce the formulas either way.
 *
 * c12381_mhac_bbs_verify_batch: ok[j] = verify_pres(pp, pk, type_j, Prv, revealed_j, pres_j) (verify_pres.cpp:6-46):
 *   C_hid = prod_ii h[Prv[ii]]^z[ii] * prod_ii h[HidPub[ii]]^zhp[ii]          one fixed-base sum of nPrv + nHidPub = nHid <= m terms
 *   U     = B_^(-ch) * C_rev^zr * A_^ze * C_hid                               -ch the reference's Zp negation (the scalar r - ch, -0 = 0) on B_ itself
 *   ok    = [ ch == H(U, A_, B_, revealed) ] and [ e(A_, w) == e(B_, g2) ]
 * pub_48 holds the REVEALED public values only, n x nRevPub fields lane-major in ascending Pub position: a verifier holds no others (the
 * reference's verify_pres takes the whole public span and range-checks it; this entry neither reads nor checks the hidden ones).  z_48, zhp_48,
 * pub_48 may each be NULL when its count is 0.
 * The three per-lane powers are ONE k = 3 product under one doubling chain (c12381_g1_mul_sum_batch).  The pairing half is c12381_ps_verify_batch
 * with no messages (g2, X2 = w, s1 = A_, s2 = B_), its route for a w outside G2 included.  The reference has no "A_ != infinity" test: a lane with
 * A_ = B_ = infinity is judged by the formulas alone.
 * Status: ok[j] = 1 / 0 as verify_pres returns; 0xff where the reference would throw: A_, B_ or C_rev does not decode (bad tag, x not on the
 * curve), or ch, zr, ze, a z, a zhp or a revealed value is >= r.  A pp / used h / pk that does not decode makes every lane 0xff and returns
 * C12381_E_POINT (the _dev form reports it at the next c12381_sync); the context stays usable.
 * Workspace (c12381_trim releases it): per presentation of a chunk of up to 2^18, 956 + 32 nHid + 48 nRevPub bytes, besides the workspaces of the
 * entries named above. */
#define C12381_MHAC_T_MAX 8
int c12381_mhac_bbs_verify_batch(c12381_ctx* ctx, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                                 const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* pk_97, const uint8_t* crev_49, const uint8_t* fixed_242,
                                 const uint8_t* z_48, const uint8_t* zhp_48, const uint8_t* pub_48, uint8_t* ok);
int c12381_mhac_bbs_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                                     const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* pk_97, const uint8_t* crev_49, const uint8_t* fixed_242,
                                     const uint8_t* z_48, const uint8_t* zhp_48, const uint8_t* pub_48, uint8_t* ok);
/* c12381_mhac_bbs_pres_batch: cred_pres(pp, creds, group, type, Prv, public_attributes, attr_shares) (cred_pres.cpp:6-113) for t parties with the
 * caller's randomness.  The caller selects the rows of S: the entry never sees S or the n parties.  Per presentation, lane-major:
 *   A_49      creds.A                                  D_49      group.D
 *   lam_48    t fields, group.lambda                   eshare_48 t fields, e_share[S[k]] in the order of S
 *   ashare_48 t x nPrv fields, a_share[S[k]][ii], party-major (NULL allowed when nPrv = 0)
 *   crev_49, cpub_49   type.C_rev, type.C_pub
 *   pub_48    the WHOLE public span, nPub fields in Pub order; every field is range-checked (NULL allowed when nPub = 0)
 *   rnd       the 2 + (t - 1) nPrv + nHid + t scalars the reference draws, in its order: r, alpha, beta_share, beta_share_j, gamma_share;
 *             32 big-endian bytes each, any value below 2^256, reduced mod r first
 * With j = 0 as in the reference (`size_t j = 0;`), b = beta_share, bj = beta_share_j, g = gamma_share, a_k = a_share[S[k]], e_k = e_share[S[k]]:
 *   A_ = A^r        B_ = (C_pub * D)^r
 *   U  = C_rev^alpha * prod_(ii < nHid) h[Hid[ii]]^bj[ii] * A_^g[0] * prod_(k = 1 .. t-1) ( prod_(ii < nPrv) h[Prv[ii]]^b[(k-1) nPrv + ii] * A_^g[k] )
 *   ch as above
 *   zr = alpha + ch r        ze = sum_k ( g[k] + ch (-e_k lambda_k) )
 *   z[ii]   = bj[ii] + ch r a_0[ii] lambda_0 + sum_(k >= 1) ( b[(k-1) nPrv + ii] + ch r a_k[ii] lambda_k )     ii < nPrv; bj is indexed by ii,
 *                                                                                                         NOT by the position of Prv[ii] in Hid
 *   zhp[ii] = bj[ position of HidPub[ii] in Hid ] + ch pub_a[ position of HidPub[ii] in Pub ] r
 * The Zp results are canonical residues.  The curve points are exact for every input: A_ is an unchecked per-lane point, so its t powers are t
 * separate multiply calls whose results are added — never one power of the sum of the g[k]; with C_rev^alpha that makes t + 1 per-lane powers,
 * ceil((t + 1) / 4) products of at most C12381_G1_MUL_SUM_MAX terms joined by additions.  A_ and B_ are one generic G1 column of 2 n lanes.  The
 * h terms form ONE base list of exactly the reference's terms, nHid + (t - 1) nPrv positions; a list longer than C12381_G1_FIXED_SUM_MAX is
 * refused (C12381_E_ARG).  Exponents on one base meet only on the table route, where the device has checked that base to be a point of G1 other
 * than infinity; the generic route multiplies position by position.
 * Outputs: fixed_242 (n x 242 bytes), z_48 (n x nPrv x 48 bytes, may be NULL when nPrv = 0), zhp_48 (n x nHidPub x 48 bytes, may be NULL when
 * nHidPub = 0), status (n bytes).
 * Status: status[j] = 0, or 0xff where the reference would throw: A, D, C_rev or C_pub does not decode, or a lambda, e_share, a_share or public
 * value is >= r.  That presentation's fixed_242, z_48 and zhp_48 bytes are then all 0xff, the other lanes are unaffected and the call returns
 * C12381_OK.  A pp or used h record that does not decode behaves as in verify: every status and output byte 0xff, C12381_E_POINT.
 * NOT constant-time: the scalar multiplications and the table look-ups take data-dependent paths and addresses.  The secrets the call is given
 * (the shares, lambda, the randomness) and values derived from them stay in the context's device workspaces (and, for the host form, its staging
 * buffer) until a later call overwrites them or c12381_trim frees them; nothing is wiped.
 * Workspace: per presentation of a chunk of up to 2^18, 1692 + 32 (t + nHid + (t - 1) nPrv) + 48 nRevPub bytes, besides the workspaces of the
 * entries used. */
int c12381_mhac_bbs_pres_batch(c12381_ctx* ctx, size_t n, size_t m, size_t t, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                               const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* A_49, const uint8_t* D_49, const uint8_t* lam_48,
                               const uint8_t* eshare_48, const uint8_t* ashare_48, const uint8_t* crev_49, const uint8_t* cpub_49, const uint8_t* pub_48,
                               const uint8_t* rnd, uint8_t* fixed_242, uint8_t* z_48, uint8_t* zhp_48, uint8_t* status);
int c12381_mhac_bbs_pres_batch_dev(c12381_ctx* ctx, size_t n, size_t m, size_t t, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                                   const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* A_49, const uint8_t* D_49, const uint8_t* lam_48,
                                   const uint8_t* eshare_48, const uint8_t* ashare_48, const uint8_t* crev_49, const uint8_t* cpub_49, const uint8_t* pub_48,
                                   const uint8_t* rnd, uint8_t* fixed_242, uint8_t* z_48, uint8_t* zhp_48, uint8_t* status);

#ifdef __cplusplus
}
#endif

#endif
