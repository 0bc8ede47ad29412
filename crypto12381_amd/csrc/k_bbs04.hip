// SHA3-512 and the bbs04 group-signature kernels (examples/bbs04/src/bbs.cpp of the reference), one signature / message per lane:
//   sha3_512_kernel          out[i] = SHA3-512(msgs[i * len .. i * len + len))   (sha3.hpp; hash_state, set.hpp:317-392)
//   bbs04_pub_kernel         gpk = serialize(g1, g2, h, u, v, w) -> the 49- / 97-byte records the decompression kernels read
//   bbs04_prep_kernel        signature -> T1, T2, T3 records, parse<Zp> range checks, the thirteen scalar columns of verify
//   bbs04_combine_kernel     the complete additions of verify over the thirteen scalar-multiplication columns
//   bbs04_transcript_kernel  msg || T1 || T2 || T3 || R1 || R2 || R3 || R4 || R5, one thread per byte
//   bbs04_check_kernel       SHA3-512 of the transcript mod r == c, and the status bytes
//   bbs04_open_*             open: T3 - (T1^xi1 + T2^xi2)
//   bbs04_sign_*             sign: member key and randomness -> scalar columns (bbs04_sign.hpp), T3 = A + h^(alpha + beta), the additions
//                            behind R1..R5 / P1, P2, and c, the five responses and the 435-byte record from the transcript
//   bbs04_issue_pack_kernel  key_gen's member keys: serialize(A_i, x_i)
// c12381_hip.hip (c12381_sha3_512_batch*, c12381_bbs04_*) launches them; the scalar multiplications, the affine conversions and the
// pairing product are the library's existing kernels.
#include "kernels_common.hpp"
#include "fr.hpp"
#include "sha3.hpp"
#include "bbs04_sign.hpp"

using namespace c12381;

namespace {

// signature j: T1, T2, T3 into three 49-byte columns, the six Zp fields (c, s_alpha, s_beta, s_x, s_delta1, s_delta2) as numeric values;
// returns whether every field is below r (parse<G1^3 | Zp^6>, zp_number.hpp:226-236)
__device__ __forceinline__ bool bbs04_parse_sig(size_t n, size_t j, const uint8_t* sig435, uint8_t* t49, fr (&z)[6]) {
    const uint8_t* s = sig435 + 435 * j;
#pragma unroll 1
    for (int k = 0; k < 3; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) t49[49 * (k * n + j) + b] = s[49 * k + b];
    bool ok = true;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        uint8_t v[32];
        ok = wire_zp(v, s + 147 + 48 * f) && ok;
        uint32_t k[8];
        words_from_be32(k, v);
        fr_set_words(z[f], k);
    }
    return ok;
}
__device__ __forceinline__ void g1_load_affine(g1p& p, const uint8_t* p96) {
    bool inf, ok;
    g1p inf_pt;
    g1_parse96(p.x, p.y, inf, ok, p96); fp_one(p.z);
    g1_set_inf(inf_pt);
    fp_select(p.x, inf, inf_pt.x, p.x); fp_select(p.y, inf, inf_pt.y, p.y); fp_select(p.z, inf, inf_pt.z, p.z);
}
__device__ __forceinline__ void g1_negate(g1p& p) {
    fp ny;
    fp_neg(ny, p.y);
    fp_norm1(p.y, ny);
}
__device__ __forceinline__ void g1_store_norm(int32_t* proj, size_t stride, size_t idx, const g1p& p) {
    g1p o;
    g1_norm1(o, p);
    soa_store_g1(proj, stride, idx, o);
}

}  // namespace

namespace c12381 {

__global__ void __launch_bounds__(BLOCK, 2) sha3_512_kernel(size_t n, size_t len, const uint8_t* msgs, uint8_t* out64) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t h[8];
    sha3_512(h, msgs + len * i, len);
    uint4* o = reinterpret_cast<uint4*>(out64 + 64 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = make_uint4((uint32_t)h[2 * k], (uint32_t)(h[2 * k] >> 32), (uint32_t)h[2 * k + 1], (uint32_t)(h[2 * k + 1] >> 32));
}

// gpk = g1 (49) | g2 (97) | h (49) | u (49) | v (49) | w (97)  ->  g1s49 = g1, h, u, v;  g2s97 = g2, w
__global__ void __launch_bounds__(BLOCK, 2) bbs04_pub_kernel(const uint8_t* gpk390, uint8_t* g1s49, uint8_t* g2s97) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < 4 * 49) {
        const size_t e = t / 49, b = t % 49;
        g1s49[t] = gpk390[(e == 0 ? 0 : 146 + 49 * (e - 1)) + b];
    } else if (t < 4 * 49 + 2 * 97) {
        const size_t u = t - 4 * 49, e = u / 97, b = u % 97;
        g2s97[u] = gpk390[(e == 0 ? 49 : 293) + b];
    }
}

// The scalar columns of verify (column k of the scalar-multiplication slab multiplies by sc[k * n + j]):
//   0 -c (T1)   1 -c (T2)   2 sx (T3)   3 sx (T1)   4 sx (T2)   5 c (T3)                               variable bases
//   6 sa (u)    7 sb (v)    8 -sd1 (u)  9 -sd2 (v)  10 -sd1 + -sd2 (h)  11 c (g1)  12 -(sa + sb) (h)   fixed bases
// Negations are mod r with -0 = 0 (mod_negate).  c32[j] = c; st[j] = 1 when every Zp field is below r.
__global__ void __launch_bounds__(BLOCK, 2) bbs04_prep_kernel(size_t n, const uint8_t* sig435, uint8_t* t49, uint8_t* sc, uint8_t* c32, uint8_t* st) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr z[6];
    st[j] = bbs04_parse_sig(n, j, sig435, t49, z) ? 1 : 0;
    const fr &c = z[0], &sa = z[1], &sb = z[2], &sx = z[3], &d1 = z[4], &d2 = z[5];
    fr negc, nd1, nd2, nd12, sab, nab;
    fr_neg(negc, c); fr_neg(nd1, d1); fr_neg(nd2, d2);
    fr_add(nd12, nd1, nd2);
    fr_add(sab, sa, sb); fr_neg(nab, sab);
    const fr* col[13] = {&negc, &negc, &sx, &sx, &sx, &c, &sa, &sb, &nd1, &nd2, &nd12, &c, &nab};
#pragma unroll
    for (int k = 0; k < 13; ++k) store_be32(sc + 32 * (k * n + j), *col[k]);
    store_be32(c32 + 32 * j, c);
}

// In place over the thirteen projective columns of bbs04_prep_kernel's scalars (stride = coordinate stride of proj):
//   col 0 R1 = u^sa T1^-c   1 R2 = v^sb T2^-c   2 R4 = T1^sx u^-sd1   3 R5 = T2^sx v^-sd2
//   col 4 P1 = T3^sx h^(-sd1 - sd2) / g1^c      5 P2 = h^-(sa + sb) T3^c        (R3 = e(P1, g2) e(P2, w))
// Every column is read before it is written (P1 waits in column 10).
__global__ void __launch_bounds__(BLOCK, 2) bbs04_combine_kernel(size_t n, int32_t* proj, size_t stride) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g1p a, b;
    soa_load_g1(a, proj, stride, 2 * n + j);
    soa_load_g1(b, proj, stride, 10 * n + j);
    g1_add(a, b);
    soa_load_g1(b, proj, stride, 11 * n + j);
    g1_negate(b);
    g1_add(a, b);
    g1_store_norm(proj, stride, 10 * n + j, a);
#pragma unroll 1
    for (size_t k = 0; k < 4; ++k) {                  // R1 = col 0 + col 6, R2 = 1 + 7, R4 = 3 + 8, R5 = 4 + 9
        soa_load_g1(a, proj, stride, (k < 2 ? k : k + 1) * n + j);
        soa_load_g1(b, proj, stride, (6 + k) * n + j);
        g1_add(a, b);
        g1_store_norm(proj, stride, k * n + j, a);
    }
    soa_load_g1(a, proj, stride, 10 * n + j);
    g1_store_norm(proj, stride, 4 * n + j, a);
    soa_load_g1(a, proj, stride, 5 * n + j);
    soa_load_g1(b, proj, stride, 12 * n + j);
    g1_add(a, b);
    g1_store_norm(proj, stride, 5 * n + j, a);
}

// Transcript of lane j (L = msg_len + 919 bytes): msg | T1 | T2 | T3 | R1 | R2 | R3 (576) | R4 | R5, G1 elements 49-byte encoded.
// T_k is hashed as `hash` serialises the parsed point: its wire tag (02 / 03; 00 = infinity) and the canonical x of the decoded point
// (t96: 96 zero bytes for infinity), so a leading 0x00 with other bytes behind it becomes 49 zeros and an x >= p is re-encoded mod p.
// r49: R1, R2, R4, R5 as columns of n records.
__global__ void __launch_bounds__(BLOCK, 2) bbs04_transcript_kernel(size_t n, size_t msg_len, const uint8_t* msgs, const uint8_t* t49, const uint8_t* t96,
                                                                  const uint8_t* r49, const uint8_t* gt576, uint8_t* out) {
    const size_t L = msg_len + 919;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n * L) return;
    const size_t j = t / L, b = t % L;
    uint8_t v;
    if (b < msg_len) v = msgs[msg_len * j + b];
    else {
        const size_t q = b - msg_len;
        if (q < 147) {
            const size_t k = q / 49, e = q % 49;
            v = e == 0 ? t49[49 * (k * n + j)] : t96[96 * (k * n + j) + e - 1];
        } else if (q < 245) {
            const size_t k = (q - 147) / 49, e = (q - 147) % 49;
            v = r49[49 * (k * n + j) + e];
        } else if (q < 821) {
            v = gt576[576 * j + q - 245];
        } else {
            const size_t k = 2 + (q - 821) / 49, e = (q - 821) % 49;
            v = r49[49 * (k * n + j) + e];
        }
    }
    out[t] = v;
}

// ok[j] = [c_j == SHA3-512(transcript_j) mod r] (Zp from_hash, zp_number.hpp:540-548), or 0xff where the reference would terminate: a
// Zp field >= r (st_sig), T1 / T2 / T3 not decodable (st_t, three columns), or public material not decodable (st_pub: 4 G1 + 2 G2
// statuses; every lane, and bad_flag[0] -> C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) bbs04_check_kernel(size_t n, size_t L, const uint8_t* tr, const uint8_t* c32, const uint8_t* st_sig,
                                                             const uint8_t* st_t, const uint8_t* st_pub, uint8_t* ok, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    bool pub = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) pub = pub && st_pub[i] != 0;
    if (!pub) { ok[j] = 0xff; if (j == 0) *bad_flag = 1; return; }
    if (!st_sig[j] || !st_t[j] || !st_t[n + j] || !st_t[2 * n + j]) { ok[j] = 0xff; return; }
    uint64_t h[8];
    sha3_512(h, tr + L * j, L);
    uint32_t w[16], got[8], want[8];
    sha3_digest_words_be(w, h);
    fr r;
    fr_from_digest_words(r, w);
    fr_to_words(got, r);
    words_from_be32(want, c32 + 32 * j);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= got[i] ^ want[i];
    ok[j] = diff == 0 ? 1 : 0;
}

// open: T columns as in verify, sc = xi1 (column 0), xi2 (column 1) for every lane; st[j] = 1 when the six Zp fields of the signature
// are below r.  gmsk = serialize(xi1, xi2): a value >= r raises bad_flag[2] (C12381_E_ARG) and zeroes every st.
__global__ void __launch_bounds__(BLOCK, 2) bbs04_open_prep_kernel(size_t n, const uint8_t* gmsk96, const uint8_t* sig435, uint8_t* t49, uint8_t* sc,
                                                                 uint8_t* st, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    fr z[6];
    const bool sig_ok = bbs04_parse_sig(n, j, sig435, t49, z);
    const bool xi_ok = wire_zp(sc + 32 * j, gmsk96) && wire_zp(sc + 32 * (n + j), gmsk96 + 48);
    if (!xi_ok && j == 0) bad_flag[2] = 1;
    st[j] = sig_ok && xi_ok ? 1 : 0;
}
// proj column 0 <- T3 - (column 0 + column 1)
__global__ void __launch_bounds__(BLOCK, 2) bbs04_open_combine_kernel(size_t n, int32_t* proj, size_t stride, const uint8_t* t3_96) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g1p a, b;
    soa_load_g1(a, proj, stride, j);
    soa_load_g1(b, proj, stride, n + j);
    g1_add(a, b);
    g1_negate(a);
    g1_load_affine(b, t3_96 + 96 * j);
    g1_add(b, a);
    g1_store_norm(proj, stride, j, b);
}
__global__ void __launch_bounds__(BLOCK, 2) bbs04_open_status_kernel(size_t n, const uint8_t* st_sig, const uint8_t* st_t, uint8_t* status) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    status[j] = (st_sig[j] && st_t[j] && st_t[n + j] && st_t[2 * n + j]) ? 0 : 0xff;
}

// ---- sign (bbs.cpp:32-59)
// gsk_j = serialize(A, x) -> a49[j] = A's wire bytes; rnd_j -> the twelve scalar columns sc[k * n + j] (bbs04_sign.hpp numbers the fixed ones):
//   0 alpha (u)  1 beta (v)  2 alpha + beta (h)  |  3, 4, 5 r_x (T1, T2, T3)  |  6 r_alpha (u)  7 r_beta (v)  8 -r_delta1 (u)  9 -r_delta2 (v)
//   10 -(r_delta1 + r_delta2) (h)  11 -(r_alpha + r_beta) (h)
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_prep_kernel(size_t n, const uint8_t* gsk97, const uint8_t* rnd224, uint8_t* a49, uint8_t* sc) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
#pragma unroll 1
    for (int b = 0; b < 49; ++b) a49[49 * j + b] = gsk97[97 * j + b];
    fr s[BBS04_SIGN_SCALARS], col[BBS04_SIGN_COLS];
    bbs04_sign_reduce(s, rnd224 + 224 * j);
    bbs04_sign_columns(col, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        store_be32(sc + 32 * (k * n + j), col[k]);
        store_be32(sc + 32 * ((3 + k) * n + j), s[BBS04_RX]);
    }
#pragma unroll
    for (int k = 3; k < BBS04_SIGN_COLS; ++k) store_be32(sc + 32 * ((3 + k) * n + j), col[k]);
}
// proj column 2 (h^(alpha + beta)) += A: T3
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_t3_kernel(size_t n, int32_t* proj, size_t stride, const uint8_t* a96) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g1p a, b;
    g1_load_affine(a, a96 + 96 * j);
    soa_load_g1(b, proj, stride, 2 * n + j);
    g1_add(a, b);
    g1_store_norm(proj, stride, 2 * n + j, a);
}
// In place over the nine projective columns of phase 2 (0 T1^rx  1 T2^rx  2 T3^rx  3 u^ra  4 v^rb  5 u^-rd1  6 v^-rd2  7 h^-(rd1 + rd2)
// 8 h^-(ra + rb)) -> 0 R1  1 R2  2 R4 = T1^rx u^-rd1  3 R5 = T2^rx v^-rd2  4 P1 = T3^rx h^-(rd1 + rd2)  5 P2 = h^-(ra + rb), the order verify's
// transcript and pairing product take.  Every column is read before it is written (R4 waits in column 5).
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_combine_kernel(size_t n, int32_t* proj, size_t stride) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    g1p a, b;
    soa_load_g1(a, proj, stride, j);
    soa_load_g1(b, proj, stride, 5 * n + j);
    g1_add(a, b);
    g1_store_norm(proj, stride, 5 * n + j, a);              // R4, parked
    soa_load_g1(a, proj, stride, 3 * n + j);
    g1_store_norm(proj, stride, j, a);                      // R1
    soa_load_g1(a, proj, stride, n + j);
    soa_load_g1(b, proj, stride, 6 * n + j);
    g1_add(a, b);
    g1_store_norm(proj, stride, 3 * n + j, a);              // R5
    soa_load_g1(a, proj, stride, 4 * n + j);
    g1_store_norm(proj, stride, n + j, a);                  // R2
    soa_load_g1(a, proj, stride, 2 * n + j);
    soa_load_g1(b, proj, stride, 7 * n + j);
    g1_add(a, b);
    g1_store_norm(proj, stride, 4 * n + j, a);              // P1
    soa_load_g1(a, proj, stride, 5 * n + j);
    g1_store_norm(proj, stride, 2 * n + j, a);              // R4
    soa_load_g1(a, proj, stride, 8 * n + j);
    g1_store_norm(proj, stride, 5 * n + j, a);              // P2
}
// sig_j = T1 | T2 | T3 (t49 columns) | c | s_alpha | s_beta | s_x | s_delta1 | s_delta2 with c = SHA3-512(transcript_j) mod r; status[j] = 0.
// Where the reference would terminate — A does not decode (st_a), x >= r — status[j] = 0xff and the record is 435 bytes of 0xff; public
// material that does not decode (st_pub: 4 G1 + 2 G2 statuses) does that to every lane and raises bad_flag[0] (C12381_E_POINT).
__global__ void __launch_bounds__(BLOCK, 2) bbs04_sign_finish_kernel(size_t n, size_t L, const uint8_t* tr, const uint8_t* gsk97, const uint8_t* rnd224,
                                                                   const uint8_t* t49, const uint8_t* st_a, const uint8_t* st_pub, uint8_t* sig435,
                                                                   uint8_t* status, int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    bool pub = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) pub = pub && st_pub[i] != 0;
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t x32[32];
    const bool x_ok = wire_zp(x32, gsk97 + 97 * j + 49);
    uint8_t* o = sig435 + 435 * j;
    if (!pub || !x_ok || !st_a[j]) {
#pragma unroll 1
        for (int b = 0; b < 435; ++b) o[b] = 0xff;
        status[j] = 0xff;
        return;
    }
    uint64_t h[8];
    sha3_512(h, tr + L * j, L);
    uint32_t w[16], xw[8];
    sha3_digest_words_be(w, h);
    fr c, x, s[BBS04_SIGN_SCALARS], f[6];
    fr_from_digest_words(c, w);
    words_from_be32(xw, x32);
    fr_set_words(x, xw);
    bbs04_sign_reduce(s, rnd224 + 224 * j);
    bbs04_sign_responses(f, c, x, s);
#pragma unroll 1
    for (int k = 0; k < 3; ++k)
#pragma unroll 1
        for (int b = 0; b < 49; ++b) o[49 * k + b] = t49[49 * (k * n + j) + b];
#pragma unroll
    for (int k = 0; k < 6; ++k) store_be48(o + 147 + 48 * k, f[k]);
    status[j] = 0;
}

// key_gen's member keys (bbs.cpp:17-23): gsk_j = a49[j] | x_j mod r as 48 bytes; public material that does not decode: every byte 0xff and
// bad_flag[0] (C12381_E_POINT)
__global__ void __launch_bounds__(BLOCK, 2) bbs04_issue_pack_kernel(size_t n, const uint8_t* a49, const uint8_t* x32, const uint8_t* st_pub, uint8_t* gsk97,
                                                                  int* bad_flag) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    bool pub = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) pub = pub && st_pub[i] != 0;
    if (!pub && j == 0) *bad_flag = 1;
    uint8_t* o = gsk97 + 97 * j;
    if (!pub) {
#pragma unroll 1
        for (int b = 0; b < 97; ++b) o[b] = 0xff;
        return;
    }
#pragma unroll 1
    for (int b = 0; b < 49; ++b) o[b] = a49[49 * j + b];
    uint32_t w[8];
    fr x;
    words_from_be32(w, x32 + 32 * j);
    fr_reduce_words(x, w);
    store_be48(o + 49, x);
}

}  // namespace c12381
