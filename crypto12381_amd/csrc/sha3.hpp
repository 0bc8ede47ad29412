// SHA3-512 (FIPS 202) for one message per lane: Keccak-f[1600] on 25 64-bit lanes (50 32-bit registers on the device), rate 72
// bytes, padding 0x06 ... 0x80, 64-byte output.  The same digest as MIRACL's SHA3_init(64) / SHA3_process / SHA3_hash, which the
// reference's hash_state drives byte by byte (include/crypto12381/set.hpp:317-392 -> miracl_core::sha3_*).
//
// Message reads: the full 72-byte blocks are read as ALIGNED 32-bit words and shifted into place, 19 loads per block instead of 72 byte
// loads.  Every word read holds at least one byte of the message, so no read leaves the pages the message occupies; the host build
// (tests/host_sim/sha3.cpp) therefore reads up to 3 bytes past the end of the message inside that word, and its callers pad their buffers.
// The tail (< 72 bytes) and the padding are assembled bytewise.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fp.hpp"          // C12381_HD / C12381_CONST

namespace c12381 {

constexpr int SHA3_512_RATE = 72;              // bytes: 200 - 2 * 64
constexpr int SHA3_512_LANES = SHA3_512_RATE / 8;

C12381_CONST uint64_t KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
// rho offsets of lane x + 5 y
C12381_CONST int KECCAK_RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

C12381_HD uint64_t keccak_rotl(uint64_t x, int n) { return n == 0 ? x : (x << n) | (x >> (64 - n)); }

// Keccak-f[1600]: every index below is a compile-time constant once the inner loops are unrolled, so the state never leaves registers;
// chi's a ^ (~b & c) becomes one v_bitop3_b32 per 32-bit half on gfx950
C12381_HD void keccak_f1600(uint64_t (&a)[25]) {
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t d = c[(x + 4) % 5] ^ keccak_rotl(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
        }
        // rho and pi: B[y, 2x + 3y] = rot(A[x, y], rho[x, y])
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rotl(a[x + 5 * y], KECCAK_RHO[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; ++y)
#pragma unroll
            for (int x = 0; x < 5; ++x) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= KECCAK_RC[r];
    }
}

// the aligned 32-bit word at p (p % 4 == 0), little-endian
C12381_HD uint32_t sha3_word(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t*>(p);
#else
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
#endif
}

// absorb one full block at msg (any alignment): lanes are little-endian 64-bit words of the message
C12381_HD void sha3_512_absorb_block(uint64_t (&a)[25], const uint8_t* msg) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(msg);
    const uint8_t* base = msg - (addr & 3);
    const unsigned s = (unsigned)(addr & 3) * 8;
    uint32_t d[19];
#pragma unroll
    for (int k = 0; k < 18; ++k) d[k] = sha3_word(base + 4 * k);
    d[18] = s ? sha3_word(base + 72) : 0u;            // only a misaligned block reaches into the 19th word
#pragma unroll
    for (int w = 0; w < SHA3_512_LANES; ++w) {
        const uint32_t lo = (uint32_t)((((uint64_t)d[2 * w + 1] << 32) | d[2 * w]) >> s);
        const uint32_t hi = (uint32_t)((((uint64_t)d[2 * w + 2] << 32) | d[2 * w + 1]) >> s);
        a[w] ^= ((uint64_t)hi << 32) | lo;
    }
    keccak_f1600(a);
}

// the last block: rem < 72 message bytes, then 0x06, zeros, 0x80 (one byte 0x86 when rem = 71)
C12381_HD void sha3_512_absorb_last(uint64_t (&a)[25], const uint8_t* msg, size_t rem) {
#pragma unroll
    for (int w = 0; w < SHA3_512_LANES; ++w) {
        uint64_t v = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const size_t idx = (size_t)(8 * w + b);
            uint64_t byte = idx < rem ? msg[idx] : 0u;
            if (idx == rem) byte ^= 0x06u;
            if (idx == SHA3_512_RATE - 1) byte ^= 0x80u;
            v |= byte << (8 * b);
        }
        a[w] ^= v;
    }
    keccak_f1600(a);
}

// SHA3-512 of len bytes at msg; out = the first 8 lanes of the state: digest byte j is byte j % 8 of lane j / 8
C12381_HD void sha3_512(uint64_t (&out)[8], const uint8_t* msg, size_t len) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = 0;
    size_t off = 0;
#pragma unroll 1
    for (; len - off >= (size_t)SHA3_512_RATE; off += SHA3_512_RATE) sha3_512_absorb_block(a, msg + off);
    sha3_512_absorb_last(a, msg + off, len - off);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = a[i];
}

// the digest as 16 numeric big-endian words (w[0] most significant), the form fr_from_digest_words takes
C12381_HD void sha3_digest_words_be(uint32_t (&w)[16], const uint64_t (&h)[8]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t raw = (uint32_t)(h[j / 2] >> (32 * (j % 2)));      // bytes 4j .. 4j + 3 as they lie in memory
        w[j] = __builtin_bswap32(raw);
    }
}

}  // namespace c12381
