/* c12381_ac_issue.h — the issuer's side of the anonymous-credential entries of the MI355X-native batched BLS12-381 backend: issue of the
 * reference's examples/AC-bbs, AC-rbbs and AC-rps, and AC-rps' user_keygen, from their wire formats, in one call per batch.  They produce what
 * the entries of c12381_ac.h consume (sig_97, sig_195, usk_48, upk); conventions, status codes, the context and the stream-ordering rules of the
 * "_dev" forms are those of c12381_hip.h, the wire layouts and semantics those of c12381_ac.h, which this header includes.
 */
#ifndef C12381_AC_ISSUE_H
#define C12381_AC_ISSUE_H

#include "c12381_ac.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Inputs common to the four entries, besides the wire layouts of c12381_ac.h (pk_243, Y_49, tY_97, sig_97, sig_195, usk_48):
 *   sk_48 / sk_96   the issuer's PrivateKey: serialize(x) (AC-bbs, 48 bytes) or serialize(x, y) (AC-rbbs, AC-rps, 96 bytes); ONE key per batch
 *   attr_48         the holder's WHOLE span, n x nattr fields of 48 bytes lane-major in attribute order.  EVERY field is range-checked, because
 *                   every index is read by the products of issue
 *   rnd_32          per credential the ONE scalar the reference draws in the call (w, usk or alpha), 32 big-endian bytes, any value below 2^256,
 *                   reduced mod r first.  The value 0 (and r) is computed through like any other.  n x 32 bytes
 *   upk_49          UserPublicKey = serialize(Z), 49 bytes, one record PER CREDENTIAL: n x 49 bytes
 * Everything said in c12381_ac.h carries over unchanged: the library's decoding (a leading 0x00 is infinity, x taken mod p, no subgroup check) and
 * parse<Zp>'s range check of 48-byte fields, bytewise reads, `^` = multiply exact for EVERY curve point — keys and upk may lie outside G1 / G2 or at
 * infinity — 0xff lanes where the reference would throw, batches in chunks of up to 2^18.  A tuple parse (pk.fixed_part, sk) decodes EVERY field,
 * used or not; a range parse (pk.Y, pk.tilde_Y) is lazy: only the records an entry indexes are decoded.
 * No scalar is merged across two points, and none into a point's exponent that the reference applies to the finished point: h^(x + ym) is a
 * multiplication of the point h, not g^(alpha (x + ym)), and (g * prod Y_i^a_i)^e is a multiplication of the finished sum, not a sum with scaled
 * exponents.  For points outside the subgroup those differ, as c12381_ac.h explains for (-B_)^c.
 * Status and return codes, every entry:
 *   status[j] = 0, or 0xff — and a record of 0xff bytes — where the reference would throw for credential j: an attribute >= r, or (AC-rps issue) a upk
 *   that does not decode.  The other lanes are unaffected and the call returns C12381_OK.
 *   A key that does not decode — g, tilde_g, tilde_X (the tuple parse decodes all three, used or not) or a USED record of Y / tilde_Y — makes every
 *   status and output byte 0xff and returns C12381_E_POINT; the _dev form reports it at the next c12381_sync, once.
 *   A field of sk >= r makes every status and output byte 0xff and returns C12381_E_ARG (the _dev form: at the next c12381_sync), as
 *   c12381_bbs04_open_batch does for gmsk; it takes precedence over C12381_E_POINT.  In both cases the context stays usable.
 *   C12381_E_ARG, checked before the empty-batch rule: nattr = 0, nattr > C12381_G1_FIXED_SUM_MAX (AC-rps: C12381_G2_FIXED_SUM_MAX), any null
 *   pointer.  n = 0 then returns C12381_OK and touches nothing.
 * NOT constant-time: the scalar multiplications and the table look-ups take data-dependent paths and addresses.  sk is read on the device; the
 * secrets a call is given (sk, the attributes, w, usk, alpha) and the values derived from them (x + w and its inverse, x + ym, alpha y^(nattr+1))
 * stay in the context's device workspaces (and, for the host form, its staging buffer) until a later call overwrites them or c12381_trim frees
 * them; nothing is wiped.  The _dev forms never make the host wait. */

/* c12381_ac_bbs_issue_batch: sig_97[j] = issue(keys, attr_j) (examples/AC-bbs/src/issue.cpp:6-18), w_j = rnd_32[j] mod r:
 *   A = (g * prod_(i < nattr) Y_i^a_i)^inverse(x + w)          Signature = serialize(A, w), 49 + 48 bytes
 * inverse(0) = 0 (BIG_invmodp), so for w = r - x, A is multiply(B, 0): infinity for B in G1, whatever PAIR_G1mul makes of it otherwise (see
 * c12381_bbs04_issue_batch).  The sum is ONE G1 fixed-base sum with the addend g over the base list Y[0 .. nattr) in ATTRIBUTE order, from the
 * positional tables of c12381_g1_mul_fixed_sum_batch (its workspace, its routes: tables when every base is a point of G1 other than infinity, the
 * generic kernel column by column otherwise); then the simultaneous inversion of c12381_zp_op_batch and one generic G1 column — the shape of
 * c12381_bbs_plus_sign_batch.  The base list coincides with the list of c12381_ac_bbs_pres_batch / _verify_batch only for an EMPTY disclosure set
 * (theirs puts the disclosed attributes in front): an issuer and a verifier sharing one context rebuild the tables of the positions that differ.
 * Y_49: nattr records, all used.  Outputs: sig_97 (n x 97 bytes), status (n bytes).
 * Workspace (c12381_trim releases it): per credential of a chunk 289 + 32 nattr bytes, besides the workspaces of the entries named above. */
int c12381_ac_bbs_issue_batch(c12381_ctx* ctx, size_t n, size_t nattr, const uint8_t* sk_48, const uint8_t* pk_243, const uint8_t* Y_49,
                              const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status);
int c12381_ac_bbs_issue_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, const uint8_t* sk_48, const uint8_t* pk_243, const uint8_t* Y_49,
                                  const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status);
/* c12381_ac_rbbs_issue_batch: examples/AC-rbbs/src/issue.cpp:6-18 — the same computation, the same implementation.  It differs in sk only:
 * sk_96 = serialize(x, y), BOTH fields range-checked though y is not used.  Y_49 holds the 2 nattr records of an AC-rbbs key, of which only
 * Y[0 .. nattr) are read: the range parse is lazy, an undecodable Y[k], k >= nattr, has no effect. */
int c12381_ac_rbbs_issue_batch(c12381_ctx* ctx, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* Y_49,
                               const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status);
int c12381_ac_rbbs_issue_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* Y_49,
                                   const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_97, uint8_t* status);

/* c12381_ac_rps_user_keygen_batch: user_keygen(pk) (examples/AC-rps/src/user_keygen.cpp:6-14): usk_j = rnd_32[j] mod r, upk_j = g^usk_j through g's
 * fixed-base route (c12381_g1_mul_fixed_batch: its table, or the generic kernel when g lies outside G1 or at infinity).
 * Outputs: usk_48 (n x 48 bytes, serialize(usk)) and upk_49 (n x 49 bytes).  There is no per-lane failure and no status array; pk_243 not decoding
 * is the key failure above (both outputs 0xff, C12381_E_POINT).  C12381_E_ARG: a null pointer.
 * Workspace: 32 bytes per key pair of a chunk. */
int c12381_ac_rps_user_keygen_batch(c12381_ctx* ctx, size_t n, const uint8_t* pk_243, const uint8_t* rnd_32, uint8_t* usk_48, uint8_t* upk_49);
int c12381_ac_rps_user_keygen_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* pk_243, const uint8_t* rnd_32, uint8_t* usk_48, uint8_t* upk_49);

/* c12381_ac_rps_issue_batch: sig_195[j] = issue(keys, upk_j, attr_j) (examples/AC-rps/src/issue.cpp:6-39), alpha_j = rnd_32[j] mod r, Z = upk_j:
 *   h       = g^alpha                                          g's fixed-base route, as user_keygen
 *   ym      = sum_(i < nattr) a_i y^(i+1)                       Horner's rule in y, on the device
 *   sigma   = h^(x + ym) * Z^(alpha y^(nattr+1))                ONE k = 2 per-lane product over (h, Z) (c12381_g1_mul_sum_batch)
 *   tilde_M = prod_(i < nattr) tilde_Y[i]^a_i                   the G2 fixed-base sum with no addend over tilde_Y[0 .. nattr), attribute order
 *   Signature = serialize(h, sigma, tilde_M), 49 + 49 + 97 bytes
 * alpha = 0 gives h = infinity and sigma = multiply(infinity, ..) * multiply(Z, 0).  tY_97 holds the nattr + 1 records of the key; tilde_Y[nattr] is
 * never read, an undecodable one has no effect.  pk.Y is not a parameter: issue never touches it.  The tables of the G2 sum are the positional ones
 * of c12381_g2_mul_fixed_sum_batch; they coincide with those of c12381_ac_rps_redact_batch / _verify_batch where idx[k] = k.
 * Outputs: sig_195 (n x 195 bytes), status (n bytes): 0, or 0xff for an attribute >= r or a upk_j that does not decode (bad tag, x not on the curve;
 * a leading 0x00 IS infinity whatever follows).
 * Workspace: per credential of a chunk 485 + 32 nattr bytes, besides the workspaces of the entries named above (window tables of the k = 2 product:
 * 2 x 2816 bytes per lane of a launch). */
int c12381_ac_rps_issue_batch(c12381_ctx* ctx, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* tY_97,
                              const uint8_t* upk_49, const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_195, uint8_t* status);
int c12381_ac_rps_issue_batch_dev(c12381_ctx* ctx, size_t n, size_t nattr, const uint8_t* sk_96, const uint8_t* pk_243, const uint8_t* tY_97,
                                  const uint8_t* upk_49, const uint8_t* attr_48, const uint8_t* rnd_32, uint8_t* sig_195, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* C12381_AC_ISSUE_H */
