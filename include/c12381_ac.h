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

#ifdef __cplusplus
}
#endif
#endif /* C12381_AC_H */
