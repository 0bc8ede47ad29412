// TEST HARNESS (CPU): the per-lane scalar work of the PS wire entries (csrc/ps.hpp) compiled for the host with C12381_CHECK_BOUNDS.
// Not a product path.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../crypto12381_amd/csrc/ps.hpp"

using namespace c12381;

namespace {
// sha3.hpp reads the full blocks of a message in aligned 32-bit words: every message gets a 4-byte-aligned copy with 4 bytes either side
struct padded_msg {
    std::vector<uint32_t> buf;
    const uint8_t* p;
    padded_msg(const uint8_t* msg, size_t len, size_t shift) : buf((len + 16) / 4 + 2, 0u) {
        uint8_t* b = reinterpret_cast<uint8_t*>(buf.data()) + 4 + (shift & 3);
        if (len) std::memcpy(b, msg, len);
        p = b;
    }
};
}  // namespace

// n signatures of 98 bytes -> s49: σ1 of signature j at record j, σ2 at record n + j (the layout of ps_wire_prep_kernel)
extern "C" int sim_ps_split(size_t n, const uint8_t* sig98, uint8_t* s49) {
    for (size_t j = 0; j < n; ++j) ps_split_sig(s49 + 49 * j, s49 + 49 * (n + j), sig98 + 98 * j);
    return 0;
}
// n messages of msg_len bytes -> message-major scalars m32[32 (i n + j)]; returns the number of scalars per message.  Message j is read at
// byte offset j mod 4 of an aligned word, so every alignment of sha3.hpp's block reads is exercised.
extern "C" int sim_ps_messages(int mode, size_t n, size_t msg_len, const uint8_t* msgs, uint8_t* m32) {
    const size_t nmsg = ps_msg_scalars(mode, msg_len);
    for (size_t j = 0; j < n; ++j) {
        padded_msg m(msgs + msg_len * j, msg_len, j);
        for (size_t i = 0; i < nmsg; ++i) ps_store_msg(m32 + 32 * (i * n + j), mode, m.p, msg_len, i);
    }
    return (int)nmsg;
}
// Per lane j its OWN key (x48 + 48 j, y48 + 48 nY j), message and t32 -> sc[64 j] = t, sc[64 j + 32] = t e (the interleaved layout of
// ps_sign_prep_kernel); ok[j] = 1 when x and the used y_i passed parse<Zp>'s range check
extern "C" int sim_ps_sign_scalars(int mode, size_t n, size_t nY, size_t msg_len, const uint8_t* x48, const uint8_t* y48, const uint8_t* msgs,
                                   const uint8_t* t32, uint8_t* sc, uint8_t* ok) {
    const size_t nused = ps_msg_scalars(mode, msg_len);
    if (nused > nY) return -1;
    for (size_t j = 0; j < n; ++j) {
        padded_msg m(msgs + msg_len * j, msg_len, j);
        fr t, te;
        ok[j] = ps_sign_scalars(t, te, x48 + 48 * j, y48 + 48 * nY * j, nused, mode, m.p, msg_len, t32 + 32 * j) ? 1 : 0;
        store_be32(sc + 64 * j, t);
        store_be32(sc + 64 * j + 32, te);
    }
    return 0;
}
// parse<Zp>: returns the range check, out32 = the low 32 bytes as the routine read them
extern "C" int sim_zp_parse48(const uint8_t* b48, uint8_t* out32) {
    fr v;
    const bool ok = zp_parse48(v, b48);
    store_be32(out32, v);
    return ok ? 1 : 0;
}
