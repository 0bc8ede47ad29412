// TEST HARNESS (CPU): the per-signature scalar work of bbs04 sign (csrc/bbs04_sign.hpp) compiled for the host with C12381_CHECK_BOUNDS.
// Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/bbs04_sign.hpp"

using namespace c12381;

// Per lane: rnd224 (7 x 32 B, any values), c32 and x32 (32 big-endian bytes, below r) ->
//   cols   9 x 32 B fixed-base scalar columns (bbs04_sign_columns), lane-major
//   rx32   r_x mod r
//   f288   c, s_alpha, s_beta, s_x, s_delta1, s_delta2 as serialize(Zp) writes them, 6 x 48 B
extern "C" int sim_bbs04_sign(size_t n, const uint8_t* rnd224, const uint8_t* c32, const uint8_t* x32, uint8_t* cols, uint8_t* rx32, uint8_t* f288) {
    for (size_t j = 0; j < n; ++j) {
        fr s[BBS04_SIGN_SCALARS], col[BBS04_SIGN_COLS], f[6], c, x;
        uint32_t w[8];
        bbs04_sign_reduce(s, rnd224 + 224 * j);
        bbs04_sign_columns(col, s);
        for (int k = 0; k < BBS04_SIGN_COLS; ++k) store_be32(cols + 32 * (BBS04_SIGN_COLS * j + k), col[k]);
        store_be32(rx32 + 32 * j, s[BBS04_RX]);
        words_from_be32(w, c32 + 32 * j);
        fr_from_words(c, w);                        // Montgomery form, as fr_from_digest_words hands c over
        words_from_be32(w, x32 + 32 * j);
        fr_set_words(x, w);
        bbs04_sign_responses(f, c, x, s);
        for (int k = 0; k < 6; ++k) store_be48(f288 + 48 * (6 * j + k), f[k]);
    }
    return 0;
}
// c as the device obtains it: 64 digest bytes -> fr_from_digest_words -> canonical 32 bytes
extern "C" int sim_bbs04_c_from_digest(const uint8_t* digest64, uint8_t* c32) {
    uint32_t w[16], k[8];
    for (int i = 0; i < 16; ++i)
        w[i] = ((uint32_t)digest64[4 * i] << 24) | ((uint32_t)digest64[4 * i + 1] << 16) | ((uint32_t)digest64[4 * i + 2] << 8) | (uint32_t)digest64[4 * i + 3];
    fr c, o;
    fr_from_digest_words(c, w);
    fr_to_words(k, c);
    fr_set_words(o, k);
    store_be32(c32, o);
    return 0;
}
