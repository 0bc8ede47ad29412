// The PS-shaped kernels around the library's point arithmetic (examples/ps/src/ps.cpp of the reference), one signature per lane; the per-lane
// scalar routines are ps.hpp's:
//   ps_wire_prep_kernel         verify: serialize(σ1, σ2) -> two columns of 49-byte records, message bytes -> message-major scalars
//   ps_wire_finish_kernel       verify: ok[j] <- 0xff where the reference would throw (σ1 / σ2 or a public point does not decode)
//   ps_generator_kernel         the default generator of G1 (consts.hpp) as a 96-byte affine record: the base of sign's fixed-base column
//   ps_sign_prep_kernel         sign: the two fixed-base scalars t, t e of every signature, interleaved, and parse<Zp>'s check of the secret key
//   ps_sign_finish_kernel       sign: every output byte 0xff when the secret key failed that check
//   ps_randomize_prep_kernel    randomnize: r_j for both components of signature j
//   ps_randomize_finish_kernel  randomnize: status bytes, 98 bytes of 0xff where σ1 or σ2 does not decode
//   ps_aggregate_finish_kernel  aggregate verdict: 0 when a signature point was off the curve
// c12381_hip.hip (c12381_ps_*) launches them; decompression, scalar multiplication, affine conversion, the bucket products and the pairing
// product are the library's existing kernels.
#include "kernels_common.hpp"
#include "ps.hpp"

using namespace c12381;

namespace c12381 {

// s49: σ1 of signature j at record j, σ2 at record n + j (the columns c12381_ps_verify_batch takes once decoded); m32[32 (i n + j)] = message
// scalar i of signature j, nmsg = ps_msg_scalars(mode, msg_len) of them.  Message reads: ps.hpp ps_msg_scalar.
__global__ void __launch_bounds__(BLOCK, 2) ps_wire_prep_kernel(size_t n, size_t msg_len, int mode, size_t nmsg, const uint8_t* sig98, const uint8_t* msgs,
                                                             uint8_t* s49, uint8_t* m32) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    ps_split_sig(s49 + 49 * j, s49 + 49 * (n + j), sig98 + 98 * j);
    const uint8_t* msg = msgs + msg_len * j;
#pragma unroll 1
    for (size_t i = 0; i < nmsg; ++i) ps_store_msg(m32 + 32 * (i * n + j), mode, msg, msg_len, i);
}
// st_sig: 2 n decoding statuses (σ1 column, σ2 column), st_pub: npub statuses of g2, X2 and the Y2 in use.  A public point that does not
// decode makes every lane 0xff and raises bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) ps_wire_finish_kernel(size_t n, size_t npub, const uint8_t* st_sig, const uint8_t* st_pub, uint8_t* ok, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    bool pub = true;
#pragma unroll 1
    for (size_t i = 0; i < npub; ++i) pub = pub && st_pub[i] != 0;
    if (!pub) { ok[j] = 0xff; if (j == 0) *bad_flag = 1; }
    else if (!st_sig[j] || !st_sig[n + j]) ok[j] = 0xff;
}

__global__ void __launch_bounds__(BLOCK, 2) ps_generator_kernel(uint8_t* out96) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fp x, y;
    uint32_t raw[12];
    fp_set_const(x, G1_GX); fp_set_const(y, G1_GY);
    fp_to_raw48(raw, x); store_raw48(out96, raw);
    fp_to_raw48(raw, y); store_raw48(out96 + 48, raw);
}
// sc[32 (2 j)] = t_j mod r, sc[32 (2 j + 1)] = t_j e_j mod r: lane 2 j of the fixed-base column is σ1, lane 2 j + 1 is σ2, so its 49-byte
// output IS the 98-byte signature.  key_ok[0] = 1 when x and the nused y_i are below r; otherwise bad_flag[2] is raised (C12381_E_ARG), the
// scalars are zero and ps_sign_finish_kernel overwrites the signatures.
__global__ void __launch_bounds__(BLOCK, 2) ps_sign_prep_kernel(size_t n, size_t nused, size_t msg_len, int mode, const uint8_t* x48, const uint8_t* y48,
                                                             const uint8_t* msgs, const uint8_t* t32, uint8_t* sc, uint8_t* key_ok, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr t, te;
    const bool ok = ps_sign_scalars(t, te, x48, y48, nused, mode, msgs + msg_len * j, msg_len, t32 + 32 * j);
    store_be32(sc + 64 * j, t);
    store_be32(sc + 64 * j + 32, te);
    if (j == 0) { key_ok[0] = ok ? 1 : 0; if (!ok) bad_flag[2] = 1; }
}
__global__ void __launch_bounds__(BLOCK, 2) ps_sign_finish_kernel(size_t n, const uint8_t* key_ok, uint8_t* sig98) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n || key_ok[0]) return;
#pragma unroll 1
    for (int b = 0; b < 98; ++b) sig98[98 * j + b] = 0xff;
}

__global__ void __launch_bounds__(BLOCK, 2) ps_randomize_prep_kernel(size_t n, const uint8_t* r32, uint8_t* sc) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
#pragma unroll 1
    for (int b = 0; b < 32; ++b) { const uint8_t v = r32[32 * j + b]; sc[64 * j + b] = v; sc[64 * j + 32 + b] = v; }
}
// st: the decoding statuses of the 2 n records of sig98 in order (σ1 of signature j at 2 j, σ2 at 2 j + 1)
__global__ void __launch_bounds__(BLOCK, 2) ps_randomize_finish_kernel(size_t n, const uint8_t* st, uint8_t* out98, uint8_t* status) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool ok = st[2 * j] != 0 && st[2 * j + 1] != 0;
    status[j] = ok ? 0 : 0xff;
    if (ok) return;
#pragma unroll 1
    for (int b = 0; b < 98; ++b) out98[98 * j + b] = 0xff;
}

// the bucket products leave a point that is not on the curve out of their sum and raise bad_flag[0]: the verdict over the rest means nothing
__global__ void __launch_bounds__(BLOCK, 2) ps_aggregate_finish_kernel(uint8_t* all_ok, const int* bad_flag) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && bad_flag[0]) all_ok[0] = 0;
}

}  // namespace c12381
