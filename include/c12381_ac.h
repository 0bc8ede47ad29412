/* c12381_ac.h — the anonymous-credential entries of the MI355X-native batched BLS12-381 backend: whole protocols of the reference's
 * examples/AC-* from their wire formats, in one call per batch.  Conventions, status codes, the context and the stream-ordering rules of the
 * "_dev" forms are those of c12381_hip.h, which this header includes.
 */
#ifndef C12381_AC_H
#define C12381_AC_H

#include "c12381_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* AC-bbs credentials (examples/AC-bbs/src/pres.cpp, verify.cpp) from the WIRE formats ---------------------------------------------------- */
/* Wire layouts (examples/AC-bbs/include/AC-bbs.hpp):
 *   pk_243     pk.fixed_part = serialize(g, tilde_g, tilde_X)                49 + 97 + 97 = 243 bytes
 *   Y_49       pk.Y, nattr records serialize(Y_i)                            nattr x 49 bytes
 *   signature  serialize(A, w)                                               49 + 48 = 97 bytes
 *   pres_243   PresInfo.fixed_part = serialize(A_, B_, U, s, t)              3 x 49 + 2 x 48 = 243 bytes per presentation
 *   u_48       PresInfo.u, nJ fields serialize(u_j) per presentation         n x nJ x 48 bytes, lane-major; may be NULL when nJ = 0
 *   attributes serialize(Zp) fields of 48 bytes
 *   messages   msg_len raw bytes each, contiguous (msg_len = 0 allowed, msgs may then be NULL)
 * Decoding is the library's everywhere: from_bytes with the header layer's "leading 0x00 = infinity" (g1_point.hpp:87-111 / g2_point.hpp:73-77;
 * x taken mod p, no subgroup check) and parse<Zp>'s range check (48 big-endian bytes below r, zp_number.hpp:226-236).  Records are read
 * bytewise: no alignment requirement on them.  Messages are copied bytewise into the transcript.
 *
 * The disclosure set is ONE set for the batch: idx, nI indices in the order the caller's I lists them (attr_48 of verify follows that order).
 * idx is a HOST array in both forms — it is a parameter of the call like nattr, read before anything is launched.  J is the ascending
 * list of the indices below nattr that are not in idx, nJ = nattr - nI; u_j and delta_j belong to J[j] as in the reference.  nI = 0 and nJ = 0
 * are both valid.  C12381_E_ARG: nattr = 0, nattr > C12381_G1_FIXED_SUM_MAX, nI > nattr, an index >= nattr, a repeated index, a null idx with
 * nI > 0, any other null pointer that is not allowed above.  Argument errors are checked before the empty-batch rule; n = 0 then returns
 * C12381_OK and touches nothing.
 *
 * Both entries evaluate, `^` being multiply (PAIR_G1mul, the library's G1 kernels, exact for EVERY curve point: the key, A, A_, B_ may lie
 * outside G1 / G2 or at infinity):
 *   c = SHA3-512(msg | A_ | B_ | U) mod r      hash(m, A_, B_, U).to(Zp): the message bytes with no length prefix (set.hpp:355-384), then the
 *                                              points 49-byte compressed, msg_len + 147 bytes.  Verify hashes the points re-encoded from the
 *                                              parsed ones, as hash() serialises them: a leading 0x00 hashes as 49 zeros whatever follows, an
 *                                              x >= p as its residue (c12381_bbs04_verify_batch does the same).
 * Fixed-base tables: every sum over the Y_i runs from the tables of c12381_g1_mul_fixed_sum_batch (its workspace, its routes: tables when every
 * base of the sum is a point of G1 other than infinity, the generic kernel column by column otherwise) over ONE base list of nattr positions —
 * the Y of the disclosed attributes in the order of idx, then the Y of the hidden ones ascending.  Each sum takes a range of that list and the
 * tables of all nattr positions are kept current by every one of them, so a later call of either entry with the same pk and idx builds no
 * table (one check launch per sum); a call of c12381_g1_mul_fixed_sum_batch with other bases in between takes the positions it uses.
 *
 * c12381_ac_bbs_verify_batch: ok[j] = verify(m_j, attr_j, I, pres_j, pk) (verify.cpp:6-26):
 *   K  = g * prod_(i in I) Y_i^a_i                                                                one fixed-base sum with the addend g
 *   ok = [ e(A_, tilde_X) == e(B_, tilde_g) ] and [ U * B_^c == K^s * A_^t * prod_j Y_J[j]^u_j ]
 * attr_48 holds the DISCLOSED values only, n x nI fields lane-major in the order of idx (NULL allowed when nI = 0).  The reference's verify
 * takes the holder's whole attribute span and range-checks the hidden entries too; a verifier does not hold those, so this entry neither
 * reads nor checks them.
 * The pairing half is c12381_ps_verify_batch with no messages (g2 = tilde_g, X2 = tilde_X, s1 = A_, s2 = B_), its route for key points outside
 * G2 included.  The other half is R = K^s * A_^t * (-B_)^c as ONE per-lane product of three powers under one doubling chain
 * (c12381_g1_mul_sum_batch), plus the fixed-base sum over Y_J, compared with U: multiply(-B, c) = -multiply(B, c) for every curve point because
 * every term of the GLV form is linear in the point (the scalar -c mod r on B_ would be another point off the subgroup and is not used).
 * Status: ok[j] = 1 / 0 as verify returns; 0xff where the reference would throw: A_, B_ or U does not decode (bad tag, x not on the curve), or
 * s, t, a u_j or a disclosed a_i is >= r.  A pk that does not decode (g, tilde_g, tilde_X or a Y_i) makes every lane 0xff and returns
 * C12381_E_POINT (the _dev form reports it at the next c12381_sync); the context stays usable.
 * Workspace (c12381_trim releases it): per presentation of a chunk of up to 2^18, 1359 + 32 nattr + msg_len bytes, besides the workspaces of the
 * entries named above (window tables of the k = 3 product: 3 x 2816 bytes per lane of a launch; the pairing queue). */
int c12381_ac_bbs_verify_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                               const uint8_t* Y_49, const uint8_t* pres_243, const uint8_t* u_48, const uint8_t* attr_48, const uint8_t* msgs,
                               uint8_t* ok);
int c12381_ac_bbs_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                   const uint8_t* Y_49, const uint8_t* pres_243, const uint8_t* u_48, const uint8_t* attr_48, const uint8_t* msgs,
                                   uint8_t* ok);
/* c12381_ac_bbs_pres_batch: pres(m_j, attr_j, sig_j, I, pk) (pres.cpp:6-42) with the caller's randomness.
 *   attr_48  the holder's WHOLE span, n x nattr fields lane-major in attribute order; every field is range-checked, as materialize does
 *   sig_97   n signatures serialize(A, w)
 *   rnd      per presentation the 3 + nJ scalars the reference draws, in its order: r, alpha, beta, delta_0 .. delta_(nJ-1), 32 big-endian bytes
 *            each; any value below 2^256, reduced mod r first
 * Per presentation, negation being the reference's Zp negation (the scalar r - w; -0 = 0):
 *   C_I = g * prod_I Y_i^a_i      C_J = prod_J Y_j^a_j      A_ = A^r      B_ = (C_I * C_J)^r * A_^(-w)
 *   U = C_I^alpha * A_^beta * prod_j Y_J[j]^delta_j         c as above
 *   s = alpha + r c               t = beta + (-w) c         u_j = delta_j + r c a_J[j]
 * (B_ and the first two factors of U are one per-lane product of two powers over 2 n lanes.)
 * Outputs: pres_243 (n x 243 bytes), u_48 (n x nJ x 48 bytes, may be NULL when nJ = 0), status (n bytes).
 * Status: status[j] = 0, or 0xff where the reference would throw: A does not decode, or w or an attribute is >= r.  That presentation's
 * pres_243 and u_48 bytes are then all 0xff, the other lanes are unaffected and the call returns C12381_OK.  A pk that does not decode behaves
 * as in verify: every status and output byte 0xff, C12381_E_POINT.
 * NOT constant-time: the scalar multiplications and the table look-ups take data-dependent paths and addresses.  The secrets the call is
 * given (the attributes, w, r, alpha, beta, delta_j) and values derived from them stay in the context's device workspaces (and, for the host
 * form, its staging buffer) until a later call overwrites them or c12381_trim frees them; nothing is wiped.
 * Workspace: per presentation of a chunk of up to 2^18, 1273 + 32 (nattr + nJ) + msg_len bytes, besides the workspaces of the entries used
 * (window tables of the k = 2 product over 2 n lanes: 2 x 2816 bytes per lane of a launch). */
int c12381_ac_bbs_pres_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                             const uint8_t* Y_49, const uint8_t* attr_48, const uint8_t* sig_97, const uint8_t* msgs, const uint8_t* rnd,
                             uint8_t* pres_243, uint8_t* u_48, uint8_t* status);
int c12381_ac_bbs_pres_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                 const uint8_t* Y_49, const uint8_t* attr_48, const uint8_t* sig_97, const uint8_t* msgs, const uint8_t* rnd,
                                 uint8_t* pres_243, uint8_t* u_48, uint8_t* status);

/* AC-rbbs credentials (examples/AC-rbbs/src/redact.cpp, pres.cpp, verify.cpp) from the WIRE formats ---------------------------------------- */
/* The redactable family on top of AC-bbs: presentations of constant size (341 bytes whatever nJ), for a per-credential redact step and a second
 * pairing equation over a hashed G2 combination.  Wire layouts (examples/AC-rbbs/include/AC-rbbs.hpp):
 *   pk_243     pk.fixed_part = serialize(g, tilde_g, tilde_X)                49 + 97 + 97 = 243 bytes
 *   Y_49       pk.Y, 2 nattr records of 49 bytes (Y[nattr] = g, keygen.cpp:31-38)
 *   tY_97      pk.tilde_Y, nattr records of 97 bytes
 *   sig_97     Signature = serialize(A, w)                                   49 + 48 = 97 bytes
 *   cache_196  RedactCache = serialize(C_I, C_J, B, D)                       4 x 49 = 196 bytes
 *   pres_341   PresInfo = serialize(A_, B_, C_J_, D_, U, s, t)               5 x 49 + 2 x 48 = 341 bytes
 *   attributes serialize(Zp) fields of 48 bytes; messages msg_len raw bytes each (msg_len = 0 allowed, msgs may then be NULL)
 * Everything said above for AC-bbs carries over unchanged: the library's decoding and parse<Zp>'s range check, bytewise reads, ONE disclosure set
 * per batch with idx a HOST array in both forms, the C12381_E_ARG conditions (nattr = 0, nattr > C12381_G1_FIXED_SUM_MAX, nI > nattr, an index >=
 * nattr, a repeated index, a null idx with nI > 0, any null pointer not allowed below) checked before the empty-batch rule, n = 0 returning C12381_OK
 * and touching nothing, `^` = multiply exact for EVERY curve point (keys and records outside G1 / G2 and at infinity included; no verdict rests on
 * a subgroup assumption the device has not checked), 0xff lanes where the reference would throw, and a key that does not decode: every lane 0xff
 * and C12381_E_POINT (the _dev form reports it at the next c12381_sync), the context stays usable.  Batches run in chunks of up to 2^18.
 * Hashes (set.hpp:327-392):
 *   c   = SHA3-512(msg | A_ | B_ | C_J_ | D_ | U) mod r    no length prefix; the five points 49-byte compressed as hash() re-serialises the parsed
 *                                                          points (a leading 0x00 hashes as 49 zeros, an x >= p as its residue): msg_len + 245 bytes
 *   q_i = SHA3-512(a_I[0] | .. | a_I[nI-1] | i) mod r      the disclosed values as 48-byte fields in the order of idx, then the size_t i as 8
 *                                                          little-endian bytes: 48 nI + 8 bytes.  Only i in I is ever used; those nI are computed,
 *                                                          the whole blocks of the shared prefix absorbed once per lane.
 *
 * c12381_ac_rbbs_verify_batch: ok[j] = verify(m_j, attr_j, I, pres_j, pk) (verify.cpp:6-24); attr_48 holds the DISCLOSED values only, n x nI fields
 * lane-major in the order of idx (NULL allowed when nI = 0).  With K = g * prod_I Y_i^a_i (one fixed-base sum with the addend g):
 *   ok = [ e(A_, tilde_X) == e(C_J_ * B_, tilde_g) ]                            c12381_ps_verify_batch with no messages, s1 = A_, s2 = C_J_ + B_
 *    and [ U * B_^c == K^s * A_^t ]                                             K^s A_^t (-B_)^c as ONE k = 3 product, compared with U
 *    and [ e(C_J_, prod_I tilde_Y[nattr-1-i]^q_i) == e(D_, tilde_g) ]           the PS check with NO X2: g2 = tilde_g, Y2 = the used tilde_Y, m = q_i
 * The third equation takes the routes of c12381_ps_verify_batch, picked on the device: e(-D_, tilde_g) * prod_I e(q_i C_J_, tilde_Y..) == 1 as one
 * (nI + 1)-way product over line tables when tilde_g and the used tilde_Y are elements of G2 other than infinity and nI + 1 <= C12381_FIXED_G2_MAX;
 * otherwise W = sum_I q_i tilde_Y.. (the G2 fixed-base sum for nI + 1 > C12381_FIXED_G2_MAX, column by column below; nI = 0: infinity) and pair_eq.
 * The reference parses pk.Y and pk.tilde_Y lazily: only Y_i and tilde_Y[nattr-1-i] for i in I are read and decoded, an undecodable record that
 * verify never touches does not fail the call.  nattr up to C12381_G1_FIXED_SUM_MAX.
 * Status: ok[j] = 1 / 0; 0xff: one of the five points does not decode, or s, t or a disclosed a_i is >= r.  Key failure: g, tilde_g, tilde_X or a
 * USED record of Y / tilde_Y does not decode.
 * Workspace (c12381_trim releases it): per presentation of a chunk 1752 + 64 nI + msg_len bytes, besides the workspaces of the entries used.
 * Both pairing equations share the line-table array of c12381_ps_verify_batch: its second table alternates between tilde_X and the first used
 * tilde_Y, so each chunk rebuilds that one table twice. */
int c12381_ac_rbbs_verify_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                const uint8_t* Y_49, const uint8_t* tY_97, const uint8_t* pres_341, const uint8_t* attr_48, const uint8_t* msgs,
                                uint8_t* ok);
int c12381_ac_rbbs_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, size_t msg_len, const uint8_t* pk_243,
                                    const uint8_t* Y_49, const uint8_t* tY_97, const uint8_t* pres_341, const uint8_t* attr_48, const uint8_t* msgs,
                                    uint8_t* ok);
/* c12381_ac_rbbs_pres_batch: pres(m_j, sig_j, cache_j) (pres.cpp:6-27) with the caller's randomness; no key and no index set.
 *   rnd      per presentation r, alpha, beta, 32 big-endian bytes each; any value below 2^256, reduced mod r first
 * Per presentation, negation being the reference's Zp negation (the scalar r - w; -0 = 0):
 *   A_, B_, C_J_, D_ = A^r, B^r, C_J^r, D^r      one generic G1 column of 4 n lanes
 *   U = C_I^alpha * A_^beta                       one k = 2 product;  c as above;  s = alpha + r c,  t = beta + (-w) c
 * Outputs: pres_341 (n x 341 bytes), status (n bytes): 0, or 0xff — and a record of 0xff bytes — where the reference would throw: A or a cache
 * point does not decode, or w >= r; the other lanes are unaffected and the call returns C12381_OK.
 * NOT constant-time: the scalar multiplications take data-dependent paths and addresses.  The secrets the call is given (w, r, alpha, beta) and
 * values derived from them stay in the context's device workspaces (and, for the host form, its staging buffer) until a later call overwrites
 * them or c12381_trim frees them; nothing is wiped.
 * Workspace: per presentation of a chunk 2117 + msg_len bytes, besides the workspaces of the entries used. */
int c12381_ac_rbbs_pres_batch(c12381_ctx* ctx, size_t n, size_t msg_len, const uint8_t* sig_97, const uint8_t* cache_196, const uint8_t* msgs,
                              const uint8_t* rnd, uint8_t* pres_341, uint8_t* status);
int c12381_ac_rbbs_pres_batch_dev(c12381_ctx* ctx, size_t n, size_t msg_len, const uint8_t* sig_97, const uint8_t* cache_196, const uint8_t* msgs,
                                  const uint8_t* rnd, uint8_t* pres_341, uint8_t* status);
/* c12381_ac_rbbs_redact_batch: redact(attr_j, sig_j, I, pk) (redact.cpp:7-44).  attr_48: the holder's WHOLE span, n x nattr fields lane-major in
 * attribute order, every field range-checked.  With J the indices outside I and q_i as above, per credential:
 *   C_I = g * prod_I Y_i^a_i      C_J = prod_J Y_j^a_j      B = C_I * A^(-w)
 *   D = prod_(k in K_D) Y[k]^e_k,  e_k = sum_(i in I, k-nattr+i in J) q_i a_(k-nattr+i) mod r,  K_D = { nattr - i + j : i in I, j in J }
 * exactly the k the reference's filter keeps; the empty product is infinity.  The three Y-sums are ranges of ONE base list of at most 2 nattr - 1
 * records of pk.Y, evaluated through the tables of c12381_g1_mul_fixed_sum_batch (its workspace, its routes), so a second call with the same key
 * and set builds no table.  That is why redact accepts nattr <= C12381_G1_FIXED_SUM_MAX / 2 = 16 ONLY and returns C12381_E_ARG above it (verify
 * and pres take credentials of up to 32 attributes).
 * Outputs: cache_196 (n x 196 bytes), status (n bytes): 0, or 0xff — and a record of 0xff bytes — where the reference would throw: A does not
 * decode, or w or an attribute is >= r.  The reference materialises all of pk.Y here: g, tilde_g, tilde_X or ANY of the 2 nattr records of Y_49
 * not decoding is a key failure.
 * NOT constant-time, and nothing is wiped, as for pres: the attributes, w and the values derived from them stay in the workspaces.
 * Workspace: per credential of a chunk 659 + 32 nattr + 80 nI + 32 |K_D| bytes, besides the workspaces of the entries used. */
int c12381_ac_rbbs_redact_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                const uint8_t* attr_48, const uint8_t* sig_97, uint8_t* cache_196, uint8_t* status);
int c12381_ac_rbbs_redact_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                    const uint8_t* attr_48, const uint8_t* sig_97, uint8_t* cache_196, uint8_t* status);

/* AC-rps credentials (examples/AC-rps/src/redact.cpp, pres.cpp, verify.cpp) from the WIRE formats ------------------------------------------ */
/* The redactable PS family: a user key z, presentations of constant size (389 bytes), two pairing equations whose G2 argument differs per
 * presentation.  Wire layouts (examples/AC-rps/include/AC-rps.hpp), n = nattr:
 *   pk_243     pk.fixed_part = serialize(g, tilde_g, tilde_X)                49 + 97 + 97 = 243 bytes
 *   Y_49       pk.Y, 2 nattr + 1 records of 49 bytes, Y[k] = g^(y^(k+1)) (keygen.cpp:26-37)
 *   tY_97      pk.tilde_Y, nattr + 1 records of 97 bytes
 *   sig_195    Signature = serialize(h, sigma, tilde_M)                      49 + 49 + 97 = 195 bytes
 *   cache_97   RedactCache = serialize(tilde_H)                              97 bytes
 *   pres_389   PresInfo = serialize(sigma1_, sigma2_, sigma3_, C, tilde_sigma_, c0, s0)   4 x 49 + 97 + 2 x 48 = 389 bytes
 *   usk_48     UserSecretKey = serialize(z)                                  48 bytes
 *   attributes serialize(Zp) fields of 48 bytes
 * The reference's pres and verify take a message m and never read it (pres.cpp:8, verify.cpp:6): these entries have NO message parameter.
 * Everything said above for AC-bbs / AC-rbbs carries over unchanged: the library's decoding (a leading 0x00 is infinity, x taken mod p, no subgroup
 * check) and parse<Zp>'s range check, bytewise reads, ONE disclosure set per batch with idx a HOST array in both forms, the C12381_E_ARG conditions
 * (nattr = 0, nattr > C12381_G1_FIXED_SUM_MAX, nI > nattr, an index >= nattr, a repeated index, a null idx with nI > 0, any null pointer not allowed
 * below, and what each entry adds) checked before the empty-batch rule, n = 0 returning C12381_OK and touching nothing, `^` = multiply exact for
 * EVERY curve point (keys and records outside G1 / G2 and at infinity included; no verdict rests on a subgroup assumption the device has not
 * checked), 0xff lanes where the reference would throw, and a key that does not decode: every lane 0xff and C12381_E_POINT (the _dev form reports
 * it at the next c12381_sync), the context stays usable.  Batches run in chunks of up to 2^18.
 * Parsing (set.hpp:114-160): a tuple parse — Signature, PresInfo, pk.fixed_part — decodes EVERY field, used or not; a range parse — pk.Y,
 * pk.tilde_Y, the attributes — is lazy unless `| materialize` follows: only the elements an entry indexes are decoded or range-checked.
 * Hashes (set.hpp:327-392), Ip = idx followed by nattr:
 *   q_k = SHA3-512(sigma1_ | sigma2_ | tilde_sigma_ | idx[0] .. idx[nI-1] | a_I[0] .. a_I[nI-1] | Ip[k]) mod r, k <= nI
 *         the points 49 / 49 / 97-byte compressed as hash() re-serialises the parsed points (a leading 0x00 hashes as zeros, an x >= p as its
 *         residue), every index as the 8 little-endian bytes of a size_t, the disclosed values as 48-byte fields in the order of idx:
 *         203 + 56 nI bytes.  The whole blocks of the shared 195 + 56 nI-byte prefix are absorbed once per lane.
 *   c0  = SHA3-512(sigma1_ | C | C0) mod r                                    147 bytes
 *
 * c12381_ac_rps_verify_batch: ok[j] = verify(m_j, attr_j, I, pres_j, pk) (verify.cpp:6-38); attr_48 holds the DISCLOSED values only, n x nI fields
 * lane-major in the order of idx (NULL allowed when nI = 0).  Per presentation, in the reference's order:
 *   C0 = sigma1_^s0 * C^c0                                                      ONE k = 2 product (c12381_g1_mul_sum_batch)
 *   c0 != hash(sigma1_, C, C0)  ->  ok = 0, WHATEVER the disclosed values hold: the reference returns before it reads them
 *   S  = prod_(k <= nI) Y[nattr - Ip[k]]^q_k                                     the G1 fixed-base sum over nI + 1 bases, no addend
 *   W  = tilde_X * tilde_sigma_ * prod_I tilde_Y[i]^a_i                          the G2 fixed-base sum with the addend tilde_X, one G2 addition per lane
 *   ok = [ e(sigma1_, W) * e(C, tilde_Y[nattr]) == e(sigma2_, tilde_g) ] and [ e(sigma3_, tilde_g) == e(S, tilde_sigma_) ]
 * Each equation is evaluated as the reference's header does (liner_pair.hpp:291-350): Miller values, conjugate of the right side, multiply, one
 * final exponentiation, is_unity.  W and tilde_sigma_ are per-lane G2 points nobody has checked for subgroup membership, so no equation is split
 * bilinearly over them and no conjugate is replaced by a negated point: (sigma1_, W) and (S, tilde_sigma_) run the running-point Miller loop
 * (c12381_miller_batch), (C, tilde_Y[nattr]), (sigma2_, tilde_g) and (sigma3_, tilde_g) the line tables (c12381_pair_product_fixed_g2_batch with
 * C12381_F_MILLER_ONLY, the same bytes for every Q), and the GT entries join them, both equations as one column of 2 n lanes.
 * Key records: Y[nattr - idx[k]], Y[0], tilde_Y[idx[k]] and tilde_Y[nattr] alone are read and decoded; an undecodable record that verify never
 * touches has no effect.  C12381_E_ARG also for nI + 1 > C12381_G1_FIXED_SUM_MAX.
 * Status: ok[j] = 1 / 0; 0xff: one of the five points does not decode, c0 or s0 is >= r, or — behind a matching c0 — a disclosed a_i is >= r.  Key
 * failure: g, tilde_g, tilde_X or a USED record of Y / tilde_Y does not decode.
 * Workspace (c12381_trim releases it): per presentation of a chunk 6632 + 120 nI bytes, besides the workspaces of the entries used.  The two
 * line-table products share one table position, which alternates between tilde_Y[nattr] and tilde_g: each chunk rebuilds that table twice. */
int c12381_ac_rps_verify_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                               const uint8_t* tY_97, const uint8_t* pres_389, const uint8_t* attr_48, uint8_t* ok);
int c12381_ac_rps_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                   const uint8_t* tY_97, const uint8_t* pres_389, const uint8_t* attr_48, uint8_t* ok);
/* c12381_ac_rps_pres_batch: pres(m_j, attr_j, sig_j, I, cache_j, usk_j, pk) (pres.cpp:8-62) with the caller's randomness.
 *   attr_48  the holder's WHOLE span, n x nattr fields lane-major in attribute order; every field is range-checked, as materialize does
 *   rnd      per presentation r, t, rho in the order the reference draws them, 32 big-endian bytes each; any value below 2^256, reduced mod r first
 * Per presentation, negation being the reference's Zp negation (-0 = 0), J the indices outside I:
 *   sigma1_ = h^r                    sigma2_ = sigma^r * sigma1_^t              ONE k = 2 product
 *   C = sigma1_^z                    C0 = sigma1_^rho                           one generic G1 column of 2 n lanes
 *   tilde_sigma_ = tilde_g^t * tilde_H                                          c12381_g2_mul_fixed_batch and one G2 addition per lane
 *   sigma3_ = prod_(k <= nI) Y[nattr - Ip[k]]^(t q_k) * prod_(k in K) Y[k]^e_k,  q_k as above from the encodings just made,
 *             e_k = sum over the ii <= nI with j = k + Ip[ii] - nattr - 1 in J of q_ii a_j mod r,  K = the k of [0, 2 nattr] with at least one such ii
 *   c0 as above,  s0 = rho + (-c0) z
 * sigma3_ is ONE sum over one base list through the tables of c12381_g1_mul_fixed_sum_batch (its workspace, its routes): the nI + 1 fixed positions
 * in the order of Ip — verify's list, so the two entries share those tables — then K ascending.  The list holds exactly the reference's terms: a
 * record that appears in both parts takes two positions and no zero scalar is put anywhere, because multiply(P, 0) and k1 P + k2 P differ from the
 * merged forms for points outside G1.  That is why pres returns C12381_E_ARG when nI + 1 + |K| > C12381_G1_FIXED_SUM_MAX = 32: every set fits for
 * nattr <= 12, larger credentials only with sets whose K is small enough — (16, {0, 3}) fills the list exactly, (13, {1 .. 11}) is the smallest shape
 * refused — (verify and redact take up to 32 attributes).  With J empty sigma3_ is the
 * fixed part alone.
 * Outputs: pres_389 (n x 389 bytes), status (n bytes): 0, or 0xff — and a record of 0xff bytes — where the reference would throw: h, sigma, tilde_M
 * (decoded though unused) or tilde_H does not decode, or z or ANY attribute is >= r; the other lanes are unaffected and the call returns C12381_OK.
 * The reference materialises pk.Y here: g, tilde_g, tilde_X or ANY of the 2 nattr + 1 records of Y_49 not decoding is a key failure.
 * NOT constant-time: the scalar multiplications and the table look-ups take data-dependent paths and addresses.  The secrets the call is given (the
 * attributes, z, r, t, rho) and values derived from them stay in the context's device workspaces (and, for the host form, its staging buffer)
 * until a later call overwrites them or c12381_trim frees them; nothing is wiped.
 * Workspace: per presentation of a chunk 2293 + 88 nI + 32 (nI + 1 + |K|) bytes, besides the workspaces of the entries used. */
int c12381_ac_rps_pres_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                             const uint8_t* attr_48, const uint8_t* sig_195, const uint8_t* cache_97, const uint8_t* usk_48, const uint8_t* rnd,
                             uint8_t* pres_389, uint8_t* status);
int c12381_ac_rps_pres_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* pk_243, const uint8_t* Y_49,
                                 const uint8_t* attr_48, const uint8_t* sig_195, const uint8_t* cache_97, const uint8_t* usk_48, const uint8_t* rnd,
                                 uint8_t* pres_389, uint8_t* status);
/* c12381_ac_rps_redact_batch: redact(attr_j, sig_j, I, pk) (redact.cpp:6-16): tilde_H = tilde_M / prod_I tilde_Y[i]^a_i, evaluated as the G2 fixed-base
 * sum over the used tilde_Y with no addend (the positions of verify's sum: shared tables), negated and added to tilde_M — miracl_core::sub is
 * add-the-negative.  nI = 0: tilde_M re-encoded.  There is no pk_243: redact never parses pk.fixed_part.  attr_48 is the holder's WHOLE span, n x
 * nattr fields lane-major, but only the disclosed fields are read and range-checked.
 * Outputs: cache_97 (n x 97 bytes), status (n bytes): 0, or 0xff — and a record of 0xff bytes — where the reference would throw: h, sigma (decoded
 * though unused) or tilde_M does not decode, or a disclosed a_i is >= r.  Key failure: a USED record tilde_Y[idx[k]] does not decode.
 * NOT constant-time, and nothing is wiped, as for pres: the disclosed attributes and the values derived from them stay in the workspaces.
 * Workspace: per credential of a chunk 872 + 32 nI bytes, besides the workspaces of the entries used. */
int c12381_ac_rps_redact_batch(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* tY_97, const uint8_t* attr_48,
                               const uint8_t* sig_195, uint8_t* cache_97, uint8_t* status);
int c12381_ac_rps_redact_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, size_t nI, const uint32_t* idx, const uint8_t* tY_97, const uint8_t* attr_48,
                                   const uint8_t* sig_195, uint8_t* cache_97, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* C12381_AC_H */
