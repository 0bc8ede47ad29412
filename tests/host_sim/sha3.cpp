// TEST HARNESS (CPU): the device SHA3-512 of csrc/sha3.hpp compiled for the host with C12381_CHECK_BOUNDS.  Not a product path.
// Full blocks are read as aligned 32-bit words (sha3.hpp): callers pass buffers with at least 3 bytes of slack behind the last message.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/sha3.hpp"

using namespace c12381;

extern "C" int sim_sha3_512(size_t n, size_t len, const uint8_t* msgs, uint8_t* out64) {
    for (size_t i = 0; i < n; ++i) {
        uint64_t h[8];
        sha3_512(h, msgs + len * i, len);
        std::memcpy(out64 + 64 * i, h, 64);          // little-endian host: lane bytes in digest order
    }
    return 0;
}
// the digest words handed to the scalar reduction (fr_from_digest_words): big-endian numeric words of the digest
extern "C" int sim_sha3_512_words(size_t len, const uint8_t* msg, uint32_t* w16) {
    uint64_t h[8];
    uint32_t w[16];
    sha3_512(h, msg, len);
    sha3_digest_words_be(w, h);
    std::memcpy(w16, w, 64);
    return 0;
}
