/* c12381_hip.h — C ABI of the MI355X-native batched BLS12-381 backend.
 *
 * This is the drop-in boundary for crypto12381's hot path.  The reference's seam is the set of
 * C++ free functions in namespace crypto12381::detail::miracl_core
 * (include/crypto12381/miracl_core_interface.hpp:16-204, defined in
 * src/miracl_core_interface.cpp:12-289 of the reference); it is scalar (one element per call)
 * and cannot express a 2^20 batch, so the entry points below are the batched forms of the
 * throughput functions of that seam.  Each entry cites the reference function it replaces.
 * INTEGRATION.md shows the reference-side binding (a replacement miracl_core_interface.cpp).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns 0 on success or a negative
 *     C12381_E_* code; no exceptions, no allocation visible to the caller.
 *   - All data is canonical big-endian bytes, bit-identical to the reference's encodings:
 *       Fp      48 B
 *       scalar  32 B   any value < 2^256; reduced mod r first (PAIR_G1mul pair_BLS12381.cpp:879-881)
 *       G1      96 B   x||y affine (ECP_toOctet uncompressed body, ecp_BLS12381.cpp:478-488);
 *                      96 zero bytes = point at infinity
 *               49 B   02|03 || x   compressed; 49 zero bytes = infinity (g1_point.hpp:113-117)
 *       G2     192 B   x.b||x.a||y.b||y.a (FP2_toBytes fp2_BLS12381.cpp:83-87: imaginary part first);
 *                      zeros = infinity;   97 B compressed 02|03 || x.b || x.a
 *       GT     576 B   c||b||a, each Fp4 b||a, each Fp2 b||a (FP12_toOctet fp12_BLS12381.cpp:923-929)
 *   - "host" entry points take host pointers (the library stages through its own device buffers);
 *     "_dev" entry points take DEVICE pointers (16-byte aligned) and run asynchronously on the
 *     context's stream; call c12381_sync() before reading results.
 *   - Stream ordering of "_dev" calls.  Every kernel of a context runs on the CONTEXT'S stream (its own, or the
 *     one given to c12381_set_stream) and only there: inputs must be COMPLETE ON THAT STREAM when the call
 *     is made, and outputs are ordered only with later work on that stream.  A caller that fills the inputs
 *     on another stream (a framework's default stream, a copy stream) records an event there and hands it to
 *     c12381_wait_event() before the call; a caller that consumes the outputs on another stream calls
 *     c12381_record_event() after it and waits for that event on its own stream.  Neither blocks the host.
 *     Without such an edge the library may read half-written inputs: by construction it cannot see a foreign
 *     stream (c12381_sync() or a device-wide synchronise are the host-blocking alternatives).
 *   - One context per host thread / per GPU; contexts are independent (thread-compatible).
 *   - There is no CPU fallback: without a usable HIP device c12381_create fails.
 */
#ifndef C12381_HIP_H
#define C12381_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct c12381_ctx c12381_ctx;

enum {
    C12381_OK = 0,
    C12381_E_ARG = -1,      /* bad argument (null pointer, unknown format or op) */
    C12381_E_HIP = -2,      /* HIP runtime error; see c12381_last_error */
    C12381_E_POINT = -3,    /* at least one input point is not on the curve (its output is all 0xff) */
    C12381_E_NOMEM = -4,
    C12381_E_INTERNAL = -5  /* library-internal failure (a work-queue hand-over between wavefronts timed out); the
                               affected outputs are all 0xff, never stale values; see c12381_last_error */
};

/* context -------------------------------------------------------------------------------- */
int c12381_create(int device, c12381_ctx** out);
void c12381_destroy(c12381_ctx* ctx);
const char* c12381_last_error(const c12381_ctx* ctx);
/* use an existing hipStream_t (passed as void*) for all work of this context; NULL = own stream */
int c12381_set_stream(c12381_ctx* ctx, void* hip_stream);
/* wait for the context's stream; returns C12381_E_INTERNAL / C12381_E_POINT if any kernel since the last
 * status read (every host entry point and every c12381_sync reads and clears the status) raised one:
 * callers of _dev entry points separate logical operations with c12381_sync() */
int c12381_sync(c12381_ctx* ctx);
/* Device-side ordering against other streams for the "_dev" entry points (see "Stream ordering" above); `hip_event` is a hipEvent_t
 * passed as void*, created and destroyed by the caller.
 *   c12381_wait_event:   all work the context launches AFTER this call waits for the event (hipStreamWaitEvent on the context's
 *                        stream): record the event on the stream that produced the inputs, then call this, then the _dev entry point.
 *   c12381_record_event: records the event on the context's stream behind everything launched so far (including the library's
 *                        side-stream work, which is joined first): make the consuming stream wait for it.
 * No counterpart in the reference (its seam is synchronous host code, include/crypto12381/miracl_core_interface.hpp:186-204). */
int c12381_wait_event(c12381_ctx* ctx, void* hip_event);
int c12381_record_event(c12381_ctx* ctx, void* hip_event);
/* Device workspaces grow to the largest call a context has served and are kept for the next one (a 2^20 G1 batch: 2.95 GB of window tables;
 * a GT power of 2^16 elements: 1.4 GB of power tables; 2^18 BBS+ verifications: a 344 MB state slab of the pairing work queue, one per
 * context, so a second streaming context doubles it).  c12381_trim waits for the context's
 * streams and frees all of them; cached fixed-base / line tables are rebuilt by the next call that needs them.  (The reference's seam never
 * allocates: src/miracl_core_interface.cpp works on caller-owned PODs.) */
int c12381_trim(c12381_ctx* ctx);
/* Per-kernel timing with HIP events on the context's stream (used by bench.py for the roofline
 * figure).  enable != 0 starts a fresh recording; kind: 0 = G1 scalar-mul kernel, 1 = G1 finish
 * (inversion + encode) kernel, 2 = G2 scalar-mul kernel, 3 = pairing kernel, 4 = pairing-equality kernel, 5 = MSM bucket kernel,
 * 6 = Miller-loop kernel (c12381_miller_batch_dev), 7 = GT operation / final-exponentiation kernel (c12381_gt_op_batch_dev).
 * c12381_profile_read synchronises the stream. */
int c12381_profile(c12381_ctx* ctx, int enable);
int c12381_profile_read(c12381_ctx* ctx, int kind, double* total_ms, uint64_t* launches);
/* ABI version: major << 16 | minor */
int c12381_version(void);

/* Fp (test / roofline hook) --------------------------------------------------------------- */
/* op: 0 mul, 1 add, 2 sub, 3 sqr, 4 neg, 5 inv.  Replaces FP_nres + FP_mul/FP_add/FP_sub/FP_sqr/
 * FP_neg/FP_inv + FP_redc (fp_BLS12381.cpp:223,396,485,500,466,588,817,234).  b may be NULL for
 * unary ops.  Inputs are 48-byte big-endian values below 2^384, taken mod p; outputs are canonical;
 * the inverse of 0 is 0. */
int c12381_fp_op_batch(c12381_ctx* ctx, int op, size_t n, const uint8_t* a48, const uint8_t* b48, uint8_t* out48);
int c12381_fp_op_batch_dev(c12381_ctx* ctx, int op, size_t n, const uint8_t* a48, const uint8_t* b48, uint8_t* out48);
/* register-resident chain of `iters` Montgomery multiplications per element (x <- x*y), used to
 * calibrate the integer-VALU roofline; out = final x */
int c12381_fp_mulchain_dev(c12381_ctx* ctx, size_t n, int iters, const uint8_t* a48, const uint8_t* b48, uint8_t* out48);

/* G1 ------------------------------------------------------------------------------------- */
/* out[i] = scalars[i] * pts[i].  Batched form of multiply(point1&, const big&)
 * (miracl_core_interface.hpp:122, src/miracl_core_interface.cpp:174-177 -> PAIR_G1mul) followed by
 * to_bytes(bytes_view&, point1&, compressed) (:113-116 -> ECP_toOctet).  out_fmt = 49 or 96. */
int c12381_g1_mul_batch(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g1_mul_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
/* The same with caller assertions.  C12381_F_IN_SUBGROUP: every input point lies in the order-r subgroup (G1 / G2).
 * Why it exists: the reference never checks membership and its multiply() (PAIR_G1mul pair_BLS12381.cpp:876-924 after
 * glv() :793-805; PAIR_G2mul :927-983 after gs() :814-873) adds [r]phi(P) to the result when k mod r < x^2 (any scalar of
 * at most 127 bits) and [r]psi^i(Q) for a zero odd base-|x| digit; those terms vanish on the subgroup and are cofactor
 * points elsewhere.  The default entry points reproduce them for EVERY curve point, which costs each such lane a
 * membership test as long as a scalar multiplication (2^20 G1 multiplications with 64-bit scalars: 40 ms instead of 28 ms).
 * With the flag the test is skipped: results are identical on subgroup points (tests/test_gpu_g1.py) and are plain
 * [k mod x^2]P - [k div x^2]phi(P) off it. */
#define C12381_F_IN_SUBGROUP 1u
/* C12381_F_COMPRESSED_IN: the points arrive in their serialized form — n x 49 bytes (G1) / n x 97 bytes (G2) as the header layer
 * parses them (g1_point.hpp:87-111, g2_point.hpp:73-77: a leading 0x00 is the point at infinity) in front of from_bytes(point1& /
 * point2&, bytes_view&) (src/miracl_core_interface.cpp:109-112, 187-190 -> ECP_fromOctet ecp_BLS12381.cpp:495-545 / ECP2_fromOctet
 * ecp2_BLS12381.cpp:225-266: tags 0x02 / 0x03 (G2: any tag but 0x04), x taken mod p, on-curve by construction, no subgroup check).
 * from_bytes -> multiply / pair / product is then ONE call: the square root runs in the prologue of the scalar-multiplication and
 * MSM-preparation kernels (the pairing entry decodes into a workspace first: its kernels read their inputs once per queue task).
 * A rejected encoding behaves like a point that is not on the curve: its output lane is 0xff (an MSM leaves the term out) and the
 * call returns C12381_E_POINT — the status semantics of c12381_g1_decompress_batch.  Accepted by c12381_g1_mul_batch_flags,
 * c12381_g2_mul_batch_flags, c12381_g1_msm_flags, c12381_pair_batch_flags and their _dev forms. */
#define C12381_F_COMPRESSED_IN 4u
int c12381_g1_mul_batch_flags(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
int c12381_g1_mul_batch_flags_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
/* out[i] = sum_(j < k) scalars[j n + i] * pts[j n + i]: a product of k powers PER LANE under one doubling chain — the shape of the
 * Schnorr-type equations that end the reference's proof checks (examples/bbs04/src/bbs.cpp:70-75 u^sa * T1^-c, examples/AC-rps/src/
 * verify.cpp:16, examples/MHAC-bbs/src/verify_pres.cpp:43) and of the header layer's fused g^x * h^y (double_multiply,
 * g1_point.hpp:317-353 -> src/miracl_core_interface.cpp:179-182 -> ECP_mul2; Π[n] walks its range in such pairs, g1_point.hpp:391-401).
 * pts / scalars are argument-major arrays of k n records as in c12381_pair_product_batch; 1 <= k <= C12381_G1_MUL_SUM_MAX; out_fmt = 49 or 96.
 * The value of every lane is multiply(point1&, const big&) on each term (PAIR_G1mul: scalar mod r, GLV form, with the [r]phi(P) term of
 * k mod r < x^2) followed by add(point1&, point1&), for EVERY curve point and every 256-bit scalar — the contract of c12381_g1_mul_batch
 * and c12381_g1_msm; k = 1 returns the bytes of c12381_g1_mul_batch_flags.  For points of G1 this equals double_multiply / ECP_mul2 and
 * the header-level Π; off the subgroup the two differ because ECP_mul2 forms the true multiples [k_i mod r]P_i where this entry goes
 * through multiply()'s GLV form: that case stays with c12381_g1_sum_of_products.
 * The k tables of a lane share one accumulator: 125 doublings per lane instead of 125 k, one projective result and one affine
 * conversion.  The loop's additions are incomplete; a lane that meets an exceptional one recomputes its k products with the complete
 * formulas.  No lane of independent random points does, but lanes built from RELATED points (Q = +-P, Q = 2P, Q = phi(P), a product
 * that cancels to infinity) and from points of small order do: such a batch is correct and runs at the complete path's speed.
 * Status: a point that is not on the curve makes its lane 0xff and the call return C12381_E_POINT, the other lanes are unaffected;
 * n = 0 returns C12381_OK and touches nothing.  flags: C12381_F_IN_SUBGROUP (see c12381_g1_mul_batch_flags);
 * C12381_F_COMPRESSED_IN and every other flag are refused (C12381_E_ARG), as are k outside its range, a bad out_fmt and null pointers.
 * Workspace: k table records of 2816 B per lane of a launch, at most 2.95 GB for any n (launches of 4, 2, 2 machine rounds for k = 2, 3, 4). */
#define C12381_G1_MUL_SUM_MAX 4
int c12381_g1_mul_sum_batch(c12381_ctx* ctx, size_t n, int k, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
int c12381_g1_mul_sum_batch_dev(c12381_ctx* ctx, size_t n, int k, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
/* out[i] = a[i] + b[i].  Batched add(point1&, point1&) (:129-132 -> ECP_add). */
int c12381_g1_add_batch(c12381_ctx* ctx, size_t n, const uint8_t* a96, const uint8_t* b96, uint8_t* out, int out_fmt);
/* out = sum_i scalars[i] * pts[i]  (the reference's Π[n](g[i]^x[i]), g1_point.hpp:371-404, and
 * sum_of_products(point1&, int, point1*, const big*) :134-137 -> ECP_muln). */
int c12381_g1_msm(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g1_msm_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
/* the same with C12381_F_COMPRESSED_IN (pts = n x 49 bytes): parse<G1> + Π in one call */
int c12381_g1_msm_flags(c12381_ctx* ctx, size_t n, const uint8_t* pts, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
int c12381_g1_msm_flags_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
/* out = sum_i pts[i] (no scalars): the header layer's product over G1Point values — a chain of add(point1&, point1&)
 * (miracl_core_interface.hpp:101, src/miracl_core_interface.cpp:129-132 -> ECP_add) — and the combine step of a product sharded
 * over GPUs (N partial points of 96 B).  n = 0 gives infinity; a point that is not on the curve is left out and
 * reported (C12381_E_POINT). */
int c12381_g1_sum(c12381_ctx* ctx, size_t n, const uint8_t* pts96, uint8_t* out, int out_fmt);
int c12381_g1_sum_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts96, uint8_t* out, int out_fmt);
/* The boundary function sum_of_products(point1&, int, point1*, const big*) with the reference's value for EVERY input
 * (src/miracl_core_interface.cpp:134-137 -> ECP_muln ecp_BLS12381.cpp:1112-1148, a plain Pippenger): the sum of the true multiples
 * [k_i mod r]P_i.  For points of G1 this equals c12381_g1_msm, which is the fast path; off the subgroup the two differ because the
 * header-level Π — what c12381_g1_msm reproduces — goes through multiply()'s GLV form (tests/golden/g1.json
 * offsubgroup_msm49 vs offsubgroup_sum_of_products49). */
int c12381_g1_sum_of_products(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g1_sum_of_products_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
/* the same product over several GPUs driven by ONE host process: terms split contiguously over ctxs[0..ngpu-1] (one
 * context per device, created by the caller), local MSMs run concurrently, the ngpu partial points are summed on
 * ctxs[0] (the combine is an elliptic-curve addition, 96 B per GPU). */
int c12381_g1_msm_multi(c12381_ctx** ctxs, int ngpu, size_t n, const uint8_t* points96, const uint8_t* scalars32, uint8_t* out, int out_fmt);

/* G2 ------------------------------------------------------------------------------------- */
/* out[i] = scalars[i] * pts[i].  Batched multiply(point2&, const big&) (miracl_core_interface.hpp:152,
 * src/miracl_core_interface.cpp:202-205 -> PAIR_G2mul) + to_bytes(bytes_view&, point2&, compressed)
 * (:192-195 -> ECP2_toOctet).  out_fmt = 97 or 192. */
int c12381_g2_mul_batch(c12381_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g2_mul_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out, int out_fmt);
/* with caller assertions (C12381_F_IN_SUBGROUP, see c12381_g1_mul_batch_flags) */
int c12381_g2_mul_batch_flags(c12381_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
int c12381_g2_mul_batch_flags_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out, int out_fmt, unsigned flags);
/* out = sum_i scalars[i] * pts[i] in G2; scalars == NULL: the plain sum of the points — product(type_identity<G2Point>, r)
 * (g2_point.hpp:225-236: get_infinity + a chain of add(point2&, point2&)); with scalars it is what the header layer evaluates
 * for Π[n](q[i]^x[i]) (eager multiply(point2&, big) :202-217, then that chain).  n = 0 gives infinity. */
int c12381_g2_msm(c12381_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g2_msm_dev(c12381_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out, int out_fmt);
/* out[i] = a[i] + b[i].  Batched add(point2&, point2&) (:212-215 -> ECP2_add). */
int c12381_g2_add_batch(c12381_ctx* ctx, size_t n, const uint8_t* a192, const uint8_t* b192, uint8_t* out, int out_fmt);

/* pairing -------------------------------------------------------------------------------- */
/* gt[i] = e(g1[i], g2[i]): pair_ate(fp12&, point2&, point1&) + pair_final_exponentiation(fp12&) +
 * to_bytes(bytes_view&, fp12&) (miracl_core_interface.hpp:199-201,189; src/miracl_core_interface.cpp:
 * 276-284, 246-249 -> PAIR_ate, PAIR_fexp, FP12_toOctet). */
int c12381_pair_batch(c12381_ctx* ctx, size_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* gt576);
int c12381_pair_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* gt576);
/* the same with C12381_F_COMPRESSED_IN (g1 = n x 49, g2 = n x 97 bytes): from_bytes x 2 + pair in one call */
int c12381_pair_batch_flags(c12381_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt576, unsigned flags);
int c12381_pair_batch_flags_dev(c12381_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt576, unsigned flags);
/* gt[i] = prod_{j < k} e(g1s[j * n + i], g2s[j * n + i]) for k = 1, 2 or 3 (argument-major arrays of k * n points):
 * pair(a, b) * pair(c, d) as the header layer forms it (liner_pair.hpp:291-303) ->
 * pair_double_ate(fp12&, point2&, point1&, point2&, point1&) (miracl_core_interface.hpp:203-204,
 * src/miracl_core_interface.cpp:286-289 -> PAIR_double_ate pair_BLS12381.cpp:508-626) + pair_final_exponentiation: ONE
 * joint Miller loop with shared Fp12 squarings and ONE final exponentiation per element (k = 3: the triple products of
 * the PS / bbs04 / AC-* examples).  A G1 argument at infinity contributes 1 (:532-541).
 * flags: C12381_F_MILLER_ONLY stops before the final exponentiation — the output is the reference's Miller value
 * (FP12_toOctet bytes of the product of the k single-loop values), what pair_double_ate itself returns. */
#define C12381_F_MILLER_ONLY 2u
int c12381_pair_product_batch(c12381_ctx* ctx, size_t n, int k, const uint8_t* g1s_96, const uint8_t* g2s_192, uint8_t* gt576, unsigned flags);
int c12381_pair_product_batch_dev(c12381_ctx* ctx, size_t n, int k, const uint8_t* g1s_96, const uint8_t* g2s_192, uint8_t* gt576, unsigned flags);
/* ok[i] = (e(a1[i], a2[i]) == e(b1[i], b2[i])) as the reference's header evaluates it
 * (liner_pair.hpp:339-350): two pair_ate, conjugate, multiply, ONE pair_final_exponentiation, is_unity.
 * ok[i] is 1 / 0, or 0xff when an input point of lane i is not on its curve. */
int c12381_pair_eq_batch(c12381_ctx* ctx, size_t n, const uint8_t* a1_96, const uint8_t* a2_192, const uint8_t* b1_96,
                         const uint8_t* b2_192, uint8_t* ok);
int c12381_pair_eq_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* a1_96, const uint8_t* a2_192, const uint8_t* b1_96,
                             const uint8_t* b2_192, uint8_t* ok);

/* wire formats either side of the path -------------------------------------- */
/* Batched from_bytes(point1&, bytes_view&) for 49-byte compressed input (miracl_core_interface.hpp:92,
 * src/miracl_core_interface.cpp:109-112 -> ECP_fromOctet -> ECP_setx: one square root per point, on-curve by
 * construction, NO subgroup check, x taken mod p).  A leading 0x00 byte means infinity (g1_point.hpp:89-93).
 * status[i] = 1 ok / 0 reject; out96[i] = x||y, zeros for infinity or reject. */
int c12381_g1_decompress_batch(c12381_ctx* ctx, size_t n, const uint8_t* in49, uint8_t* out96, uint8_t* status);
/* Batched from_bytes(point2&, bytes_view&) for 97-byte input (:146, :187-190 -> ECP2_fromOctet -> ECP2_setx);
 * any tag other than 0x04 and 0x00 is treated as compressed with sign = tag & 1, as the reference does. */
int c12381_g2_decompress_batch(c12381_ctx* ctx, size_t n, const uint8_t* in97, uint8_t* out192, uint8_t* status);
/* device-pointer forms (wire bytes already on the device; the 49- / 97-byte records are read bytewise, no alignment
 * requirement on them; out and status as above) */
int c12381_g1_decompress_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* in49, uint8_t* out96, uint8_t* status);
int c12381_g2_decompress_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* in97, uint8_t* out192, uint8_t* status);

/* split pairing and GT arithmetic (what the reference's GTMiller / GTPoint types call) ----------- */
/* pair_ate(fp12&, point2&, point1&) alone (:199 -> 276-279 -> PAIR_ate): the Miller value as FP12_toOctet bytes. */
int c12381_miller_batch(c12381_ctx* ctx, size_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* out576);
int c12381_miller_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* out576);
/* pair_final_exponentiation(fp12&) alone (:201 -> 281-284 -> PAIR_fexp). */
int c12381_fexp_batch(c12381_ctx* ctx, size_t n, const uint8_t* in576, uint8_t* out576);
int c12381_fexp_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* in576, uint8_t* out576);
/* op 0: multiply(fp12& r, fp12& v) r*=v (:193 -> 256-259 -> FP12_mul); 1: conjugate (:191 -> 251-254);
 * 2: pow(fp12&, fp12& base, const big&) (:195 -> 261-264 -> FP12_pow; b = 32-byte exponents, used as given,
 *    unitary squarings exactly like the reference: bases outside the cyclotomic subgroup go through the reference's
 *    own digit sequence, members — every pairing value — through a 4-bit windowed ladder that returns the same
 *    bytes; the device holds 224 KB of table per wavefront of 21 elements, at most 1.4 GB);
 * 3: final exponentiation. */
int c12381_gt_op_batch(c12381_ctx* ctx, int op, size_t n, const uint8_t* a576, const uint8_t* b, uint8_t* out576);
int c12381_gt_op_batch_dev(c12381_ctx* ctx, int op, size_t n, const uint8_t* a576, const uint8_t* b, uint8_t* out576);
/* is_unity(fp12&) (:197 -> 271-274 -> FP12_isunity): out[i] = 1 / 0. */
int c12381_gt_is_unity_batch(c12381_ctx* ctx, size_t n, const uint8_t* a576, uint8_t* out);
int c12381_gt_is_unity_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* a576, uint8_t* out);

/* gt[i] = e(g1[i], Q) with ONE G2 argument for the batch (pair(P_i, g2) against a generator or public key — the
 * shape of every verification equation in the reference's examples): pair_ate + pair_final_exponentiation + to_bytes as
 * c12381_pair_batch, but the line coefficients of Q are computed once and kept until Q changes.  Identical bytes to
 * c12381_pair_batch on n copies of Q for every Q (infinity included); Q not on the twist poisons all outputs. */
int c12381_pair_fixed_g2_batch(c12381_ctx* ctx, size_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* gt576);
int c12381_pair_fixed_g2_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* gt576);
/* gt[i] = prod_{j < k} e(g1s[j*n + i], g2s[j]) for 1 <= k <= C12381_FIXED_G2_MAX: the product of pairings whose G2 arguments are
 * public points shared by the batch — the shape of every verification equation in the reference's examples (PS
 * examples/ps/src/ps.cpp:32, :98, :145; BBS+ examples/bbs-plus/src/bbs+.cpp:72; bbs04 R3 examples/bbs04/src/bbs.cpp:45, :73).  g1s is
 * argument-major as in c12381_pair_product_batch, g2s holds k points.  Each point gets a line table, kept until the point changes,
 * and the k Miller loops share their squarings.  For k <= 3 bytes and status equal c12381_pair_product_batch with every G2 point
 * repeated n times; for any k the result is the GT product of the k c12381_pair_fixed_g2_batch values.  flags: C12381_F_MILLER_ONLY
 * (the product of the k c12381_miller_batch values).  A G1 point off the curve poisons its lane, a G2 point off the twist every lane
 * (C12381_E_POINT). */
#define C12381_FIXED_G2_MAX 8
int c12381_pair_product_fixed_g2_batch(c12381_ctx* ctx, size_t n, int k, const uint8_t* g1s_96, const uint8_t* g2s_192, uint8_t* gt576, unsigned flags);
int c12381_pair_product_fixed_g2_batch_dev(c12381_ctx* ctx, size_t n, int k, const uint8_t* g1s_96, const uint8_t* g2s_192, uint8_t* gt576, unsigned flags);

/* PS batch verification: ok[j] = [ e(s1_j, X2 + sum_i m[i*n + j] * Y2_i) == e(s2_j, g2) ], the check of the reference's
 * examples/ps/src/ps.cpp:84-99 (one message: :26-33; example_ps.cpp:39), evaluated as liner_pair.hpp:336-350 (two Miller values,
 * conjugate, multiply, one final exponentiation, is_unity).  Y2 holds nmsg points, m is message-major; nmsg = 0 is allowed (Y2 and m
 * may then be null); scalars are used as given.  ok[j] = 1 / 0, 0xff for a signature with a point off the curve; a public point off
 * the twist poisons every lane (C12381_E_POINT).  When g2, X2 and every Y2_i are elements of G2 other than infinity and
 * nmsg + 2 <= C12381_FIXED_G2_MAX, one (nmsg + 2)-way product over line tables serves the batch; otherwise W_j = X2 + sum m_ij Y2_i
 * is formed as PAIR_G2mul does and paired; the device picks the route. */
int c12381_ps_verify_batch(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                           const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, uint8_t* ok);
int c12381_ps_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                               const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, uint8_t* ok);

/* one base for the whole batch ------------------------------------------------------------------ */
/* out[i] = scalars[i] * base: g^x with one g — the reference's most common call shape (the cached default generators,
 * g1_point.hpp:257 / g2_point.hpp:246; setup / key_gen of examples/bbs-plus/src/bbs+.cpp:7-36), still `multiply`
 * (:122 -> 174-177, :152 -> 202-205) per element there.  Here a subgroup base is served from a device-built table of
 * its multiples (32 additions, no doubling; the table is kept in the context until the base changes); any other base
 * goes through the generic kernels, so the result equals c12381_g1_mul_batch / c12381_g2_mul_batch on n copies of the
 * base for every input. */
int c12381_g1_mul_fixed_batch(c12381_ctx* ctx, size_t n, const uint8_t* base96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g1_mul_fixed_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* base96, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g2_mul_fixed_batch(c12381_ctx* ctx, size_t n, const uint8_t* base192, const uint8_t* scalars32, uint8_t* out, int out_fmt);
int c12381_g2_mul_fixed_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* base192, const uint8_t* scalars32, uint8_t* out, int out_fmt);
/* out[j] = addend + sum_(i < nb) scalars[i n + j] * bases[i]: per-lane products over PUBLIC bases shared by the whole batch — the shape of
 * the reference's credential schemes: B = g1 * h0^r * Π h_i^m_i (examples/bbs-plus/src/bbs+.cpp:51, :72), C_I = g * Π Y_i^a_i and
 * U = C_I^α * A_^β * Π Y_j^δ_j (examples/AC-bbs/src/pres.cpp:16-29, verify.cpp:24), C_hid = Π h[Prv]^z * Π h[Hid_Pub]^z_hid_pub
 * (examples/MHAC-bbs/src/verify_pres.cpp:39-42), Π Y[n - Ip[i]]^q[i] (examples/AC-rps/src/verify.cpp:36).
 * bases96: nb points of 96 B, one set for the batch, 1 <= nb <= C12381_G1_FIXED_SUM_MAX; addend96: one point of 96 B, or NULL for none;
 * scalars32: base-major, nb x n records of 32 B, any value below 2^256; out_fmt = 49 or 96.
 * Value: every lane equals multiply(point1&, const big&) on each term (PAIR_G1mul: scalar mod r, GLV form, with the [r]phi(P) term of
 * k mod r < x^2) followed by add(point1&, point1&), the addend last, for EVERY curve point and every scalar — the contract of
 * c12381_g1_mul_sum_batch and c12381_g1_mul_fixed_batch; nb = 1 with a NULL addend returns the bytes of c12381_g1_mul_fixed_batch.
 * Routes: when every base is a point of G1 other than infinity the batch runs from nb device-built tables of multiples (457 KB per base,
 * 14.6 MB at nb = 32): one accumulator per lane across all bases, up to 32 nb mixed additions, no doubling, one projective result and
 * one affine conversion per lane.  The additions are complete, so RELATED bases (H2 = +-H1, 2 H1, phi(H1)) and sums that cancel to
 * infinity take no other path.  Otherwise the call runs column by column through the generic kernel of c12381_g1_mul_batch and sums
 * the columns: correct for every input, at generic speed.  The device picks the route; the host never waits.
 * Tables live in the context in a workspace of their own (not the slots of c12381_g1_mul_fixed_batch, BBS+ and bbs04), one per base
 * position, each kept until the base at its position changes; a call whose bases are all cached costs one check launch whatever nb.
 * c12381_trim frees them.
 * Status: a base or the addend that is not on the curve makes every output byte 0xff and the call return C12381_E_POINT (the _dev form:
 * the next c12381_sync, once); the context stays usable.  nb = 0, nb > C12381_G1_FIXED_SUM_MAX, a bad out_fmt or a null ctx / bases /
 * scalars / out: C12381_E_ARG, checked before the empty-batch rule; n = 0 returns C12381_OK and touches nothing.
 * Not constant-time: table indices and the additions executed depend on the scalars (as in the signing entries below). */
#define C12381_G1_FIXED_SUM_MAX 32
int c12381_g1_mul_fixed_sum_batch(c12381_ctx* ctx, size_t n, size_t nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* scalars32,
                                  uint8_t* out, int out_fmt);
int c12381_g1_mul_fixed_sum_batch_dev(c12381_ctx* ctx, size_t n, size_t nb, const uint8_t* bases96, const uint8_t* addend96, const uint8_t* scalars32,
                                      uint8_t* out, int out_fmt);
/* The same in G2: out[j] = addend + sum_(i < nb) scalars[i n + j] * bases[i] over PUBLIC G2 bases shared by the whole batch — X2 * Π Y2[i]^m[i]
 * of PS signatures (examples/ps/src/ps.cpp:98, :145), tilde_X * ... * Π tilde_Y[i]^a[i] (examples/AC-rps/src/verify.cpp:30),
 * Π tilde_Y[n-1-i]^q[i] (examples/AC-rbbs/src/verify.cpp:22).
 * bases192: nb points of 192 B, one set for the batch, 1 <= nb <= C12381_G2_FIXED_SUM_MAX; addend192: one point of 192 B, or NULL for none;
 * scalars32: base-major, nb x n records of 32 B, any value below 2^256; out_fmt = 97 or 192.
 * Value: every lane equals multiply(point2&, const big&) on each term (PAIR_G2mul: scalar mod r, the four-way GS form with its [r]psi^i(Q)
 * terms for zero odd digits) followed by add(point2&, point2&), the addend last, for EVERY point of the twist and every scalar — the
 * contract of c12381_g2_mul_fixed_batch; nb = 1 with a NULL addend returns the bytes of c12381_g2_mul_fixed_batch.
 * Routes: when every base is an element of G2 other than infinity the batch runs from nb device-built tables of multiples (2040 entries
 * of 224 B and a header: 457 KB per base, 14.6 MB at nb = 32): one accumulator per lane across all bases, up to 32 nb additions, no
 * doubling, one projective result and one affine conversion per lane.  The additions are complete on the twist (its order is odd), so
 * RELATED bases (H2 = +-H1, 2 H1, psi(H1)) and sums that cancel to infinity take no other path.  Otherwise the call runs column by
 * column through the generic kernel of c12381_g2_mul_batch and sums the columns: correct for every input, at generic speed.  The device
 * picks the route; the host never waits.
 * Tables live in the context in a workspace of their own (not the slot of c12381_g2_mul_fixed_batch, BBS+ and bbs04), one per base
 * position, each kept until the base at its position changes; a call whose bases are all cached costs one check launch whatever nb.
 * c12381_trim frees them.  c12381_ps_verify_batch forms its W with this entry when C12381_FIXED_G2_MAX - 2 < nmsg <= C12381_G2_FIXED_SUM_MAX.
 * Status: a base or the addend that is not on the twist makes every output byte 0xff and the call return C12381_E_POINT (the _dev form:
 * the next c12381_sync, once); the context stays usable.  nb = 0, nb > C12381_G2_FIXED_SUM_MAX, a bad out_fmt or a null ctx / bases /
 * scalars / out: C12381_E_ARG, checked before the empty-batch rule; n = 0 returns C12381_OK and touches nothing.
 * Not constant-time: table indices and the additions executed depend on the scalars (as in the G1 entry above). */
#define C12381_G2_FIXED_SUM_MAX 32
int c12381_g2_mul_fixed_sum_batch(c12381_ctx* ctx, size_t n, size_t nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* scalars32,
                                  uint8_t* out, int out_fmt);
int c12381_g2_mul_fixed_sum_batch_dev(c12381_ctx* ctx, size_t n, size_t nb, const uint8_t* bases192, const uint8_t* addend192, const uint8_t* scalars32,
                                      uint8_t* out, int out_fmt);

/* caller pattern of BASELINE config 5 ------------------------------------------ */
/* ok[j] = [ e(A_j, w + x_j*g2) == e(g1 + r_j*h0 + sum_i m[i*n + j]*h_i, g2) ]: the BBS+ verification equation of the
 * reference's examples/bbs-plus/src/bbs+.cpp:57-73 for n signatures of nmsg message blocks each, evaluated like
 * liner_pair.hpp:339-350 (two Miller loops, ONE final exponentiation, is_unity).  Public parameters are single
 * points (g1 96 B, g2 192 B, h0 96 B, h nmsg x 96 B, w 192 B); per-signature inputs are arrays (A n x 96 B, x and r
 * n x 32 B, m nmsg x n x 32 B message-major).  ok[j] = 1 / 0, 0xff if an input point of lane j is invalid.
 * Message encoding (encode_to<Zp>, zp_number.hpp:1011-1037) and parsing stay on the caller's side. */
int c12381_bbs_plus_verify_batch(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192,
                                 const uint8_t* h0_96, const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96,
                                 const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, uint8_t* ok);
int c12381_bbs_plus_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192,
                                     const uint8_t* h0_96, const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96,
                                     const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, uint8_t* ok);
/* Optional aggregate mode ("random-linear-combination batching ... behind a flag"; the reference has no
 * counterpart, it verifies one signature per call, bbs+.cpp:57-73).  ONE verdict for the batch:
 *   *all_ok = 1  iff g2 and w are elements of G2 and
 *                prod_j [ e(A_j, w) e(x_j A_j - B_j, g2) ]^rho[j] == 1,   B_j = g1 + r_j h0 + sum_i m[i*n + j] h_i,
 * evaluated as inner products mod r, two bucket products over the A_j and ONE product of two pairings.  rho: n x 32 B
 * scalars drawn by the caller, unpredictable to whoever produced the signatures (128 random bits each suffice).
 * If every signature passes c12381_bbs_plus_verify_batch, *all_ok = 1; if one does not, *all_ok = 1 with probability
 * at most 2^-k over rho drawn uniformly from k-bit values (k <= 254).  *all_ok = 0 settles nothing (an invalid signature, or public keys outside G2): run the
 * per-signature entry then.  n = 0 gives 1.  At most 2^26 - nmsg - 2 signatures per call.  The _dev form writes one
 * byte. */
int c12381_bbs_plus_verify_aggregate(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192,
                                     const uint8_t* h0_96, const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96,
                                     const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, const uint8_t* rho_32, int* all_ok);
int c12381_bbs_plus_verify_aggregate_dev(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* g2_192,
                                         const uint8_t* h0_96, const uint8_t* h_96, const uint8_t* w_192, const uint8_t* A_96,
                                         const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, const uint8_t* rho_32,
                                         uint8_t* all_ok);

/* hash-to-G1 ------------------------------------------------------------------- */
/* G1Point::from_hash (include/crypto12381/g1_point.hpp:219-234) from the 64-byte SHA3-512 digest on: the digest as a
 * big-endian integer mod p (fixed_time_mod :55 -> 94-97), residue (:110 -> 149-152 -> FP_nres), map_to_point
 * (:113 -> 154-157 -> ECP_map2point: simplified SWU + 11-isogeny), multiply_cofactor (:116 -> 159-162 -> ECP_cfp),
 * encoded like to_bytes.  Hashing the caller's serialisation (hash_state, set.hpp:317-392): c12381_sha3_512_batch.
 * out_fmt 49 or 96.  Not RFC 9380 hash_to_curve: one field element per digest, as the reference defines it. */
int c12381_g1_from_hash_batch(c12381_ctx* ctx, size_t n, const uint8_t* digests64, uint8_t* out, int out_fmt);
int c12381_g1_from_hash_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* digests64, uint8_t* out, int out_fmt);
/* map_to_point(point1&, const fp&) alone (:113 -> 154-157 -> ECP_map2point): 48-byte field elements (taken mod p, as
 * residue/FP_nres does) -> 96-byte affine points of E, NOT yet multiplied by the cofactor.  For u = 0 and u^2 = -1/11 (a zero
 * SSWU denominator) the result is the reference's pair (x, 0), which is NOT on the curve, and no error is reported; for the u that
 * land on the kernel of the 11-isogeny it is infinity (96 zero bytes).  c12381_g1_from_hash_batch gives infinity for both kinds. */
int c12381_g1_map_to_point_batch(c12381_ctx* ctx, size_t n, const uint8_t* u48, uint8_t* out96);
/* multiply_cofactor(point1&) alone (:116 -> 159-162 -> ECP_cfp): P -> [1 - x]P = [0xd201000000010001]P as a plain
 * multiple.  (Not c12381_g1_mul_batch: `multiply` is PAIR_G1mul, whose GLV evaluation differs from the plain
 * multiple for points outside the subgroup — which is what map_to_point produces.) */
int c12381_g1_clear_cofactor_batch(c12381_ctx* ctx, size_t n, const uint8_t* in96, uint8_t* out96);

/* scalar-field (Zp) batch helpers ----------------------------------------------- */
/* Element-wise arithmetic mod r on canonical 32-byte big-endian values (inputs < 2^256 are reduced first); what
 * zp_number.hpp evaluates per element through multiply(big2&,..) :47 + mod :63 (operator*, :295-380), mod_negate :57,
 * mod_inverse :59 -> 84-87 -> BIG_invmodp (inverse(), zp_number.hpp:420-425; the inverse of 0 is 0).
 * op 0: a*b, 1: a+b, 2: a-b, 3: -a, 4: 1/a (b ignored for 3 and 4, may be NULL). */
int c12381_zp_op_batch(c12381_ctx* ctx, int op, size_t n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32);
int c12381_zp_op_batch_dev(c12381_ctx* ctx, int op, size_t n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32);
/* Zp from_hash (zp_number.hpp:540-548): 64-byte digest as a big-endian integer mod r (fixed_time_mod). */
int c12381_zp_from_hash_batch(c12381_ctx* ctx, size_t n, const uint8_t* digests64, uint8_t* out32);
/* sum over i of a[i]*b[i] mod r (b == NULL: sum of a[i]) — sum()/inner products of zp_number.hpp:549-615; n = 0 -> 0. */
int c12381_zp_inner_product(c12381_ctx* ctx, size_t n, const uint8_t* a32, const uint8_t* b32, uint8_t out32[32]);
int c12381_zp_inner_product_dev(c12381_ctx* ctx, size_t n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32);

/* BBS+ verification from the WIRE formats of the reference's example (bbs+.cpp:57-73 as a whole): pp.g1_g2_h0 = serialize(g1, g2, h0)
 * (49 + 97 + 49 bytes, set.hpp:235-293), pp.h (nh entries of 49 bytes), pk = serialize(w) (97 bytes), signatures =
 * serialize(A, x, r) (49 + 48 + 48 bytes) and raw message bytes — msg_len bytes per message, encoded by encode_to<Zp>
 * (zp_number.hpp:1011-1037) into ceil(msg_len / 31) scalars.  Decoding (ECP_fromOctet / ECP2_fromOctet with the header layer's
 * "leading 0x00 = infinity", g1_point.hpp:87-111; parse<Zp> range check zp_number.hpp:226-236), encoding and verification run
 * on the context's stream.  ok[j] = 1 / 0 = what verify() returns, 0xff = the reference would throw for signature j (malformed
 * A, x or r); public material that does not decode poisons every lane and returns C12381_E_POINT; more message units than
 * h entries ("message is too long") is C12381_E_ARG. */
int c12381_bbs_plus_verify_wire_batch(c12381_ctx* ctx, size_t n, size_t nh, size_t msg_len, const uint8_t* g1_g2_h0_195, const uint8_t* h_49,
                                      const uint8_t* pk_97, const uint8_t* sig_145, const uint8_t* msgs, uint8_t* ok);
int c12381_bbs_plus_verify_wire_batch_dev(c12381_ctx* ctx, size_t n, size_t nh, size_t msg_len, const uint8_t* g1_g2_h0_195, const uint8_t* h_49,
                                          const uint8_t* pk_97, const uint8_t* sig_145, const uint8_t* msgs, uint8_t* ok);
/* BBS+ signing for a batch (examples/bbs-plus/src/bbs+.cpp:38-55): A[j] = (g1 * h0^r[j] * prod_i h_i^m[i*n + j])^(1/(gamma + x[j]))
 * — `^` is multiply (:122), `inverse` is mod_inverse (:59; inverse(0) = 0, so A is then the point at infinity), Π the
 * sum of the columns.  x and r are the caller's random scalars (the reference draws them inside sign()); gamma is the
 * secret key (32 B).  Output 96-byte affine points, message-major m as in the verification entry. */
int c12381_bbs_plus_sign_batch(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* h0_96, const uint8_t* h_96,
                               const uint8_t* gamma_32, const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, uint8_t* A_out96);
int c12381_bbs_plus_sign_batch_dev(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g1_96, const uint8_t* h0_96, const uint8_t* h_96,
                                   const uint8_t* gamma_32, const uint8_t* x_32, const uint8_t* r_32, const uint8_t* m_32, uint8_t* A_out96);

/* SHA3-512 (the hash in front of hash-to-G1 / Zp from_hash) ------------------------------------------------------ */
/* out[i] = SHA3-512(msgs[i*len .. i*len + len)): what hash_state computes over the bytes it is fed (include/crypto12381/set.hpp:317-392
 * -> miracl_core::sha3_init(64) / sha3_process / sha3_hash, MIRACL SHA3_init / SHA3_process / SHA3_hash: FIPS 202 SHA3-512, rate 72
 * bytes, padding 0x06 ... 0x80).  len = 0 is allowed (msgs may then be NULL).  One lane per message.  The device reads each message
 * in aligned 32-bit words: up to 3 bytes either side of a message are read (never used) when it does not start or end on a 4-byte
 * boundary, never beyond the words that hold its bytes. */
int c12381_sha3_512_batch(c12381_ctx* ctx, size_t n, size_t len, const uint8_t* msgs, uint8_t* out64);
int c12381_sha3_512_batch_dev(c12381_ctx* ctx, size_t n, size_t len, const uint8_t* msgs, uint8_t* out64);

/* bbs04 group signatures (examples/bbs04/src/bbs.cpp) from the WIRE formats -------------------------------------------------------- */
/* Wire layouts (examples/bbs04/include/bbs.hpp):
 *   gpk        serialize(g1, g2, h, u, v, w)                        49 + 97 + 49 + 49 + 49 + 97 = 390 bytes
 *   gmsk       serialize(xi1, xi2)                                   2 x 48 = 96 bytes
 *   signature  serialize(T1, T2, T3, c, s_alpha, s_beta, s_x, s_delta1, s_delta2)   3 x 49 + 6 x 48 = 435 bytes
 *   messages   msg_len raw bytes each, contiguous (msg_len = 0 allowed, msgs may then be NULL)
 * Decoding is from_bytes with the header layer's "leading 0x00 = infinity" (g1_point.hpp:87-111; ECP_fromOctet: x taken mod p, no
 * subgroup check) and parse<Zp>'s range check (48 big-endian bytes below r, zp_number.hpp:226-236).
 *
 * c12381_bbs04_verify_batch: ok[j] = verify(gpk, msg_j, sig_j) (bbs.cpp:61-78).  Per signature, `^` being multiply (PAIR_G1mul, the
 * library's G1 kernels, exact for every curve point) and negations Zp negations mod r (-0 = 0):
 *   R1 = u^sa T1^-c   R2 = v^sb T2^-c   R4 = T1^sx u^-sd1   R5 = T2^sx v^-sd2
 *   R3 = e(T3^sx h^(-sd1 + -sd2) / g1^c, g2) * e(h^-(sa + sb) T3^c, w)     (c12381_pair_product_fixed_g2_batch with k = 2)
 *   ok = [ c == SHA3-512(msg | T1 | T2 | T3 | R1 | R2 | R3 | R4 | R5) mod r ]   (hash(...).to(Zp), zp_number.hpp:540-548)
 * The transcript is msg_len + 919 bytes: G1 elements 49-byte compressed (infinity = 49 zeros), R3 576 bytes (FP12_toOctet).  T1..T3 are
 * hashed re-encoded from the parsed points, as hash() serialises them: a leading 0x00 hashes as 49 zeros whatever follows, an x >= p
 * as its residue.
 * Status: ok[j] = 1 / 0 as verify returns; 0xff where the reference would terminate (verify is noexcept): T1, T2 or T3 does not decode
 * (bad tag, x not on the curve) or a Zp field is >= r.  A gpk that does not decode makes every lane 0xff and returns C12381_E_POINT.
 * Workspace (c12381_trim releases it): per signature of a chunk of up to 2^18, 2139 + (msg_len + 919) bytes plus 13 projective G1 points
 * (1872 bytes) in the scalar-multiplication workspace, whose window tables take 2816 bytes per lane of six variable-base columns
 * (at most 2.95 GB); 2^18 signatures with 32-byte messages: about 1.5 GB besides the tables. */
int c12381_bbs04_verify_batch(c12381_ctx* ctx, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* sig_435, const uint8_t* msgs,
                              uint8_t* ok);
int c12381_bbs04_verify_batch_dev(c12381_ctx* ctx, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* sig_435, const uint8_t* msgs,
                                  uint8_t* ok);
/* c12381_bbs04_open_batch: out49[j] = serialize(T3 / (T1^xi1 * T2^xi2)) (open, bbs.cpp:80-86), the signer's A_i for a valid signature.
 * status[j] = 0, or 0xff where the reference would terminate on signature j (parse<G1^3 | Zp^6>: T1, T2 or T3 does not decode, or a
 * Zp field >= r); out49[j] is then unspecified.  xi1 or xi2 >= r sets every status byte to 0xff and returns C12381_E_ARG (the _dev form
 * reports it at the next c12381_sync). */
int c12381_bbs04_open_batch(c12381_ctx* ctx, size_t n, const uint8_t* gmsk_96, const uint8_t* sig_435, uint8_t* out49, uint8_t* status);
int c12381_bbs04_open_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* gmsk_96, const uint8_t* sig_435, uint8_t* out49, uint8_t* status);
/* c12381_bbs04_sign_batch: sig[j] = sign(gpk, gsk_j, msg_j) (bbs.cpp:32-59) with the caller's randomness.  Further layouts:
 *   gsk   n records serialize(A_i, x_i), 49 + 48 = 97 bytes (GroupMemberPrivateKey, bbs.hpp), decoded as above: a leading 0x00 is
 *         infinity, x taken mod p, no subgroup check, parse<Zp> range check on the 48-byte field
 *   rnd   per signature the seven scalars the reference draws inside sign(), in the order of its structured binding: alpha, beta, r_alpha,
 *         r_beta, r_x, r_delta1, r_delta2, 32 big-endian bytes each, 224 bytes per signature; any value below 2^256, reduced mod r first
 *   sig   serialize(T1, T2, T3, c, s_alpha, s_beta, s_x, s_delta1, s_delta2), 435 bytes per signature
 * Per signature, `^` being multiply (PAIR_G1mul, exact for every curve point: gpk and A may lie outside G1 / G2, w may be infinity):
 *   T1 = u^alpha   T2 = v^beta   T3 = A h^(alpha + beta)   R1 = u^ra   R2 = v^rb   R4 = T1^rx u^-rd1   R5 = T2^rx v^-rd2
 *   R3 = e(T3^rx h^-(rd1 + rd2), g2) * e(h^-(ra + rb), w)                  (c12381_pair_product_fixed_g2_batch with k = 2)
 *   c = SHA3-512(msg | T1 | T2 | T3 | R1 | R2 | R3 | R4 | R5) mod r         (the transcript verify hashes, msg_len + 919 bytes)
 *   s_alpha = ra + c alpha   s_beta = rb + c beta   cx = c x   s_x = rx + cx   s_delta1 = rd1 + alpha cx   s_delta2 = rd2 + beta cx
 * Status: status[j] = 0 and 435 signature bytes; 0xff where the reference would terminate (A does not decode, or x >= r): that signature
 * is then 435 bytes of 0xff, the other lanes are unaffected and the call returns C12381_OK.  A gpk that does not decode sets every status
 * and signature byte to 0xff and returns C12381_E_POINT (the _dev form reports it at the next c12381_sync); the context stays usable.
 * n = 0 touches nothing.
 * NOT constant-time: the scalar multiplications, the pairing and the table look-ups take data-dependent paths and addresses.  The secrets
 * the call is given (gsk, alpha ... r_delta2) and values derived from them stay in the context's device workspaces (and, for the host
 * form, its staging buffer) until a later call overwrites them or c12381_trim frees them; nothing is wiped.
 * Workspace: per signature of a chunk of up to 2^18, 1929 + (msg_len + 919) bytes (A 49 + 96 + 1, twelve scalar columns 384, T records
 * 147 + 288, R records 196, P points 192, R3 576, transcript) plus 9 projective G1 points (1296 bytes) in the scalar-multiplication
 * workspace, whose window tables take 2816 bytes per lane of three variable-base columns; 2^18 signatures with 32-byte messages: about
 * 1.1 GB besides 2.2 GB of tables. */
int c12381_bbs04_sign_batch(c12381_ctx* ctx, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* gsk_97, const uint8_t* msgs,
                            const uint8_t* rnd_224, uint8_t* sig_435, uint8_t* status);
int c12381_bbs04_sign_batch_dev(c12381_ctx* ctx, size_t n, size_t msg_len, const uint8_t* gpk_390, const uint8_t* gsk_97, const uint8_t* msgs,
                                const uint8_t* rnd_224, uint8_t* sig_435, uint8_t* status);
/* c12381_bbs04_issue_batch: the member keys of key_gen (bbs.cpp:17-23): gsk[i] = serialize(g1^inverse(gamma + x_i), x_i), 97 bytes each.
 * gamma (one scalar) and x_i are 32 big-endian bytes, any value below 2^256, reduced mod r first.  inverse(0) = 0, so A is then g1^0:
 * infinity (49 zero bytes) for a g1 in G1; for a g1 outside G1 it is whatever PAIR_G1mul makes of the scalar 0, which need not be infinity
 * (a g1 with a point of order 3 added gives the order-3 point at x = 0, bytes 03 | 00..00).  g1 is gpk's, by its fixed-base table, or the
 * generic kernel when it lies outside G1.  A gpk that does not decode makes every output byte 0xff and returns C12381_E_POINT.  Not
 * constant-time; gamma and its inverses stay in the workspaces as above (32 + 49 bytes per key of a chunk of up to 2^18, one projective
 * point). */
int c12381_bbs04_issue_batch(c12381_ctx* ctx, size_t n, const uint8_t* gpk_390, const uint8_t* gamma_32, const uint8_t* x_32, uint8_t* gsk_97);
int c12381_bbs04_issue_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* gpk_390, const uint8_t* gamma_32, const uint8_t* x_32, uint8_t* gsk_97);

/* PS signatures (examples/ps/src/ps.cpp) from the WIRE formats ----------------------------------------------------------------------- */
/* Wire layouts (examples/ps/include/ps.hpp):
 *   signature   serialize(σ1, σ2)                                   49 + 49 = 98 bytes
 *   public key  g2 97 B, X2 97 B, Y2 nY x 97 B, as three pointers    (the single-message PublicKey, 291 B, is these fields laid out contiguously:
 *                                                                    pass pk, pk + 97, pk + 194)
 *   secret key  x 48 B, y nY x 48 B, as two pointers                 (the single-message PrivateKey, 96 B: sk, sk + 48); parse<Zp>'s range check
 *                                                                    (48 big-endian bytes below r, zp_number.hpp:226-236)
 *   messages    msg_len raw bytes each, contiguous (msg_len = 0 allowed, msgs may then be NULL)
 * Points decode as everywhere in this library (from_bytes with the header layer's "leading 0x00 = infinity", g1_point.hpp:87-111 /
 * g2_point.hpp:73-77; x taken mod p; no subgroup check).
 * msg_mode, shared by verify and sign:
 *   C12381_PS_MSG_HASH    m = SHA3-512(message bytes) mod r: hash(message).to(Zp) of ps.cpp:20, :29 (hash_state feeds a span<const char> byte by
 *                         byte with no length prefix, set.hpp:355-384).  Requires nY = 1.
 *   C12381_PS_MSG_ENCODE  m = encode_to<Zp>(message) (zp_number.hpp:1011-1037): ceil(msg_len / 31) units (ps.cpp:70, :86).  More units than nY is
 *                         the reference's "message is too long": C12381_E_ARG.  Only the first ceil(msg_len / 31) entries of Y2 / y take part:
 *                         the others are neither decoded nor range-checked.
 * Message reads: C12381_PS_MSG_HASH reads the messages as c12381_sha3_512_batch does (aligned 32-bit words: up to 3 bytes either side of a
 * message are read, never used, never beyond the words that hold its bytes); C12381_PS_MSG_ENCODE reads them bytewise.  Signatures, keys and
 * secrets are read bytewise: no alignment requirement on them.
 * Argument errors (C12381_E_ARG) are checked before the empty-batch rule: a null pointer (Y2 / y may be NULL when nY = 0), an unknown
 * msg_mode, C12381_PS_MSG_HASH with nY != 1, a message too long for nY.  n = 0 then returns C12381_OK and touches nothing. */
#define C12381_PS_MSG_HASH 0
#define C12381_PS_MSG_ENCODE 1
/* c12381_ps_verify_wire_batch: ok[j] = verify(pk, msg_j, sig_j) (ps.cpp:26-33; :84-99): parse, hash or encode, and c12381_ps_verify_batch in one
 * call.  ok[j] = 1 / 0 as verify returns; 0xff where the reference would throw on signature j (σ1 or σ2 does not decode: a bad tag, an x with
 * no point on the curve).  A public point in use that does not decode makes every lane 0xff and returns C12381_E_POINT. */
int c12381_ps_verify_wire_batch(c12381_ctx* ctx, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* g2_97, const uint8_t* X2_97,
                                const uint8_t* Y2_97, const uint8_t* sig_98, const uint8_t* msgs, uint8_t* ok);
int c12381_ps_verify_wire_batch_dev(c12381_ctx* ctx, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* g2_97, const uint8_t* X2_97,
                                    const uint8_t* Y2_97, const uint8_t* sig_98, const uint8_t* msgs, uint8_t* ok);
/* c12381_ps_sign_batch: sig[j] = sign(sk, msg_j) (ps.cpp:17-24; :68-82) with the caller's randomness: t_32[j] is the scalar the reference draws for
 * h = random-select_in<*G1>, which is the default generator G raised to it (g1_point.hpp:355-369); any value below 2^256, reduced mod r first.
 * Value: the bytes of serialize(G^t, (G^t)^e), e = x + sum_i y_i m_i mod r, as the reference evaluates them with multiply (G^t lies in G1, so
 * (G^t)^e = G^(t e): two multiples of one fixed base per signature, from its table).  For t = 0 mod r both components, for e = 0 mod r the second
 * one, are the point at infinity: 49 zero bytes.
 * Status: there is no per-signature failure and no status array.  x or a used y_i >= r is where the reference's parse<Zp> throws: every output
 * byte is then 0xff and the call returns C12381_E_ARG (the _dev form reports it at the next c12381_sync, as c12381_bbs04_open_batch does for
 * gmsk); the context stays usable.
 * The generator's table has a fixed-base slot of its own: the call never evicts the table c12381_g1_mul_fixed_batch (or BBS+, bbs04) holds.
 * NOT constant-time: the table look-ups take data-dependent addresses.  The secrets the call is given (x, y, t) and values derived from them
 * (t e) stay in the context's device workspaces (and, for the host form, its staging buffer) until a later call overwrites them or c12381_trim
 * frees them; nothing is wiped. */
int c12381_ps_sign_batch(c12381_ctx* ctx, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* x_48, const uint8_t* y_48, const uint8_t* msgs,
                         const uint8_t* t_32, uint8_t* sig_98);
int c12381_ps_sign_batch_dev(c12381_ctx* ctx, size_t n, size_t nY, size_t msg_len, int msg_mode, const uint8_t* x_48, const uint8_t* y_48, const uint8_t* msgs,
                             const uint8_t* t_32, uint8_t* sig_98);
/* c12381_ps_randomize_batch: out[j] = randomnize(sig_j) (ps.cpp:35-40) = serialize(σ1^r, σ2^r) with the caller's r_32[j] (any value below 2^256).
 * `^` is multiply (PAIR_G1mul), exact for every curve point: each component is what c12381_g1_mul_batch returns on the decoded point.
 * status[j] = 0, or 0xff with 98 bytes of 0xff where σ1 or σ2 does not decode; the other lanes are unaffected and the call returns C12381_OK.
 * out_98 may be sig_98. */
int c12381_ps_randomize_batch(c12381_ctx* ctx, size_t n, const uint8_t* sig_98, const uint8_t* r_32, uint8_t* out_98, uint8_t* status);
int c12381_ps_randomize_batch_dev(c12381_ctx* ctx, size_t n, const uint8_t* sig_98, const uint8_t* r_32, uint8_t* out_98, uint8_t* status);
/* Optional aggregate mode of c12381_ps_verify_batch (decoded inputs as there; the reference has no counterpart, it verifies one signature per
 * call, ps.cpp:84-99), the random-linear-combination form BBS+ has above.  ONE verdict for the batch:
 *   *all_ok = 1  iff g2, X2 and every Y2_i are elements of G2 other than infinity and
 *                e(-sum_j rho_j σ2_j, g2) * e(sum_j rho_j σ1_j, X2) * prod_i e(sum_j (rho_j m[i*n + j]) σ1_j, Y2_i) == 1,
 * evaluated as nmsg scalar columns mod r, nmsg + 2 bucket products over the signature points and ONE product of nmsg + 2 pairings.
 * rho: n x 32 B scalars drawn by the caller, unpredictable to whoever produced the signatures (128 random bits each suffice).
 * If c12381_ps_verify_batch accepts every lane, *all_ok = 1: the product is prod_j [e(σ2_j, g2)^-1 e(σ1_j, X2 + sum_i m_ij Y2_i)]^rho_j, and the
 * cofactor components of points outside G1 — those of the σ and those the bucket products' GLV form adds off the subgroup — pair to 1
 * against elements of G2.  If it rejects a lane, *all_ok = 1 with probability at most 2^-k over rho drawn uniformly from k-bit values
 * (k <= 254).  *all_ok = 0 settles nothing (an invalid signature, or keys outside G2): run the per-signature entry then.
 * nmsg + 2 <= C12381_FIXED_G2_MAX, otherwise C12381_E_ARG.  n = 0 gives 1.  A signature point off the curve gives *all_ok = 0 and C12381_E_POINT
 * (the _dev form: the next c12381_sync; it also writes 0 when an earlier _dev call on the context left that status unread).  The _dev form
 * writes one byte. */
int c12381_ps_verify_aggregate(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                               const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, const uint8_t* rho_32, int* all_ok);
int c12381_ps_verify_aggregate_dev(c12381_ctx* ctx, size_t n, size_t nmsg, const uint8_t* g2_192, const uint8_t* X2_192, const uint8_t* Y2_192,
                                   const uint8_t* s1_96, const uint8_t* s2_96, const uint8_t* m_32, const uint8_t* rho_32, uint8_t* all_ok);

#ifdef __cplusplus
}
#endif
#endif /* C12381_HIP_H */
