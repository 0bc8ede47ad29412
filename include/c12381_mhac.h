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

/* MHAC-bbs issuance: generate_attributes, cred_iss, make_pres_group, make_pres_type --------------------------------------------------------- */
/* Everything that produces the inputs of c12381_mhac_bbs_pres_batch, so that a caller goes from the issuer's key to a verified presentation
 * through this library alone: setup -> attr -> iss -> group -> type -> pres -> verify, device-resident in the _dev forms.  Every convention above
 * and of c12381_ac.h holds: decoding (leading 0x00 = infinity, x taken mod p, no subgroup check), parse<Zp> (48 big-endian bytes below r), `^` =
 * PAIR_G1mul, exact for every curve point; index sets (prv, rev, pub_idx, S) are HOST arrays in both forms, read before anything is launched;
 * argument errors are checked before the empty-batch rule; a pp or used h record that does not decode makes every output byte 0xff and returns
 * C12381_E_POINT (the _dev form reports it at the next c12381_sync); the caller's randomness is 32-byte values below 2^256, reduced mod r first, in
 * the order the reference draws them.  NOT constant-time, and nothing is wiped, as c12381_mhac_bbs_pres_batch states.
 *
 * Parties: a credential is shared among nparties parties, any t of which present.  polynomial(x, a0, a) = a0 + sum_i a[i] x^(i + 1) is evaluated
 * at x = 1 .. nparties.  nparties <= C12381_MHAC_PARTIES_MAX = 64: with t <= C12381_MHAC_T_MAX = 8 every power x^i the entries form is at most
 * 64^7 = 2^42 < 2^53, so the reference's `(type)std::pow(x, i)` (zp_number.hpp:1100) is the exact integer power for every accepted shape; above 2^53
 * the reference's own value is a rounded double and nothing could be exact against it.
 * C12381_E_ARG, all four entries: t = 0, t > C12381_MHAC_T_MAX, t > nparties, nparties = 0 or > C12381_MHAC_PARTIES_MAX, m = 0 or
 * m > C12381_G1_FIXED_SUM_MAX, an index out of range or repeated, a null pointer that is not explicitly allowed.
 * Per-party arrays are credential-major: record i of credential j is at position j nparties + i.  attr and iss run a chunk of max(1, 2^18 /
 * nparties) credentials at a time, so that no launch exceeds 2^18 lanes; group and type run chunks of 2^18 presentations.
 *
 * c12381_mhac_bbs_attr_batch: generate_attributes(pp, t, nparties, Prv, random) (generate_attributes.cpp:6-37).
 *   rnd        per credential m + nPrv (t - 1) scalars: attr[0 .. m), then a; a[ii (t - 1) .. (ii + 1)(t - 1)) belongs to private attribute ii
 *   share[k][ii] = polynomial(k + 1, attr[Prv[ii]], a[ii (t - 1) .. (ii + 1)(t - 1)))         k < nparties
 *   C[k]       = prod_ii h[Prv[ii]]^share[k][ii]                                              nPrv = 0: infinity
 * Outputs: pub_48 (n x nPub fields, attr at Pub, Pub the ascending complement of Prv; NULL allowed when nPub = 0), ashare_48 (n x nparties x nPrv
 * fields, party-major: the layout pres reads its rows in; NULL allowed when nPrv = 0), C_49 (n x nparties records).  prv may be NULL when nPrv = 0.
 * Only the Prv records of h are decoded.  The commitments are ONE fixed-base sum of n nparties lanes over nPrv bases (c12381_g1_mul_fixed_sum_batch:
 * its tables, its generic route for a base outside G1).  No per-lane input can fail: there is no status output.
 * Workspace: 32 nPrv nparties bytes per credential of a chunk, besides the workspaces of the entries used.
 *
 * c12381_mhac_bbs_iss_batch: cred_iss(pp, sk, t, commitment, public_indexes, public_attributes, random) (cred_iss.cpp:43-85).
 *   pub_idx    the reference's public_indexes in the caller's order, nPub <= m distinct indices below m: pub_a[ii] belongs to h[pub_idx[ii]]
 *              (NULL allowed when nPub = 0, and pub_48 with it)
 *   sk_48      the issuer's gamma, ONE field for the batch;  C_49 n x nparties records;  pub_48 n x nPub fields
 *   rnd        per credential t scalars: e, then the t - 1 coefficients a
 *   C_a        = g1 * prod_(i < t) C[i]^lambda_i * prod_ii h[pub_idx[ii]]^pub_a[ii]          lambda_i = prod_(j != i) (-x_j / (x_i - x_j)), x = 1 .. t
 *   A          = C_a^inverse(gamma + e)                                                      inverse(0) = 0: A is then infinity
 *   e_share[i] = polynomial(i + 1, e, a)                                                     i < nparties
 *   D[i]       = C[i] * A^(-e_share[i])                                                      the Zp negation, -0 = 0
 * Each C[i] is an unchecked per-lane point, so each C[i]^lambda_i is a multiply of its own (products of at most C12381_G1_MUL_SUM_MAX terms joined
 * by additions, as in pres); the public terms are one fixed-base sum with addend g1; inverse(gamma + e) is the simultaneous inversion of
 * c12381_zp_op_batch; the D column is one generic G1 column of n nparties lanes.
 * Outputs: A_49 (n records), eshare_48 (n x nparties fields), D_49 (n x nparties records), status (n bytes).
 * Status: status[j] = 0, or 0xff where the reference would throw: one of the credential's nparties C records does not decode, or a public value is
 * >= r.  That credential's A, e_share and D bytes are then all 0xff and the other credentials are untouched.  sk_48 >= r: every output byte is 0xff
 * and the call returns C12381_E_ARG (the _dev form at the next c12381_sync) — the rule of c12381_bbs04_open_batch for gmsk.
 * Workspace: 353 + 321 nparties + 128 t + 32 nPub bytes per credential of a chunk, besides the workspaces of the entries used.
 *
 * c12381_mhac_bbs_group_batch: make_pres_group(creds, S) (make_pres_group.cpp:6-21), and the selection of the rows of S that pres leaves to the caller.
 *   S          t distinct party indices below nparties, in the caller's order; x[k] = S[k] + 1
 *   lambda[k]  = prod_(y != k) (-x[y] / (x[k] - x[y]))                                        the same for every presentation of the batch
 *   D          = prod_k D_share[S[k]]^lambda[k]                                               per-term multiplies, as above
 * Inputs: D_49 (n x nparties records, of which only the rows of S are read), eshare_48 (n x nparties fields), ashare_48 (n x nparties x nPrv fields).
 * Outputs: lam_48 (n x t fields — per presentation, because that is what pres takes), Dg_49 (n records), eS_48 (n x t fields), aS_48 (n x t x nPrv
 * fields), status (n bytes).  eS_48 and aS_48 are the rows of S gathered in the order of S, copied verbatim with no range check (pres checks them);
 * each may be NULL together with its input (one of the pair NULL and the other not: C12381_E_ARG); with nPrv = 0 ashare_48 and aS_48 are not looked
 * at.  nPrv > C12381_G1_FIXED_SUM_MAX: C12381_E_ARG.
 * Status: 0, or 0xff where a D record of S does not decode; that presentation's D, lambda and gathered rows are then 0xff bytes.  There is no pp:
 * the entry never returns C12381_E_POINT.
 * Workspace: 192 + 178 t bytes per presentation of a chunk, besides the workspaces of the entries used.
 *
 * c12381_mhac_bbs_type_batch: make_pres_type(pp, Rev, Prv, public_attributes) (make_pres_type.cpp:6-38).  The sets are those of verify and pres.
 *   C_rev      = g1 * prod_(ii in RevPub) h[Pub[ii]]^pub_a[ii]
 *   C_pub      = C_rev * prod_(ii in PubHid) h[Pub[ii]]^pub_a[ii]                              PubHid: the positions of Pub whose attribute is in Hid
 * pub_48: the WHOLE public span, n x nPub fields in Pub order, every field range-checked (NULL allowed when nPub = 0).  Only the Pub records of h are
 * decoded; they form ONE base list, the revealed positions in front, and the two sums run over its two ranges; an empty range leaves its addend.
 * Outputs: crev_49, cpub_49 (n records each), status (n bytes): 0, or 0xff — and both records 0xff bytes — where a public value is >= r.
 * Workspace: 289 + 32 nPub bytes per presentation of a chunk, besides the workspaces of the entries used. */
#define C12381_MHAC_PARTIES_MAX 64
int c12381_mhac_bbs_attr_batch(c12381_ctx* ctx, size_t n, size_t m, size_t t, size_t nparties, size_t nPrv, const uint32_t* prv, const uint8_t* pp_146,
                               const uint8_t* h_49, const uint8_t* rnd, uint8_t* pub_48, uint8_t* ashare_48, uint8_t* C_49);
int c12381_mhac_bbs_attr_batch_dev(c12381_ctx* ctx, size_t n, size_t m, size_t t, size_t nparties, size_t nPrv, const uint32_t* prv, const uint8_t* pp_146,
                                   const uint8_t* h_49, const uint8_t* rnd, uint8_t* pub_48, uint8_t* ashare_48, uint8_t* C_49);
int c12381_mhac_bbs_iss_batch(c12381_ctx* ctx, size_t n, size_t m, size_t t, size_t nparties, size_t nPub, const uint32_t* pub_idx, const uint8_t* pp_146,
                              const uint8_t* h_49, const uint8_t* sk_48, const uint8_t* C_49, const uint8_t* pub_48, const uint8_t* rnd, uint8_t* A_49,
                              uint8_t* eshare_48, uint8_t* D_49, uint8_t* status);
int c12381_mhac_bbs_iss_batch_dev(c12381_ctx* ctx, size_t n, size_t m, size_t t, size_t nparties, size_t nPub, const uint32_t* pub_idx, const uint8_t* pp_146,
                                  const uint8_t* h_49, const uint8_t* sk_48, const uint8_t* C_49, const uint8_t* pub_48, const uint8_t* rnd, uint8_t* A_49,
                                  uint8_t* eshare_48, uint8_t* D_49, uint8_t* status);
int c12381_mhac_bbs_group_batch(c12381_ctx* ctx, size_t n, size_t nparties, size_t t, const uint32_t* S, size_t nPrv, const uint8_t* D_49,
                                const uint8_t* eshare_48, const uint8_t* ashare_48, uint8_t* lam_48, uint8_t* Dg_49, uint8_t* eS_48, uint8_t* aS_48,
                                uint8_t* status);
int c12381_mhac_bbs_group_batch_dev(c12381_ctx* ctx, size_t n, size_t nparties, size_t t, const uint32_t* S, size_t nPrv, const uint8_t* D_49,
                                    const uint8_t* eshare_48, const uint8_t* ashare_48, uint8_t* lam_48, uint8_t* Dg_49, uint8_t* eS_48, uint8_t* aS_48,
                                    uint8_t* status);
int c12381_mhac_bbs_type_batch(c12381_ctx* ctx, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev, const uint8_t* pp_146,
                               const uint8_t* h_49, const uint8_t* pub_48, uint8_t* crev_49, uint8_t* cpub_49, uint8_t* status);
int c12381_mhac_bbs_type_batch_dev(c12381_ctx* ctx, size_t n, size_t m, size_t nPrv, const uint32_t* prv, size_t nRev, const uint32_t* rev,
                                   const uint8_t* pp_146, const uint8_t* h_49, const uint8_t* pub_48, uint8_t* crev_49, uint8_t* cpub_49, uint8_t* status);

#ifdef __cplusplus
}
#endif

#endif
