// Per-lane scalar work of the PS signature entries (examples/ps/src/ps.cpp of the reference), host- and device-compilable like fr.hpp,
// sha3.hpp and bbs04_sign.hpp (tests/host_sim/ps_wire.cpp runs it on the CPU under C12381_CHECK_BOUNDS):
//   encode_zp_unit     unit i of encode_to<Zp>(message) as a 32-byte scalar — the ONE statement of the unit rule, shared with the BBS+ wire
//                      kernel (k_hash_zp.hip bbs_wire_prep_kernel)
//   ps_split_sig       serialize(σ1, σ2), 98 bytes -> two 49-byte records
//   zp_parse48         parse<Zp> of a 48-byte field with its range check (the host-compilable form of kernels_common.hpp wire_zp)
//   ps_msg_scalar      message scalar i of a lane: hash(message).to(Zp) (C12381_PS_MSG_HASH) or unit i of encode_to<Zp> (..._ENCODE)
//   ps_store_msg       the same as the canonical 32 bytes c12381_ps_verify_batch takes
//   ps_sign_scalars    the two fixed-base scalars of a signature: t and t * (x + sum_i y_i m_i) mod r
// Values travel as CANONICAL residues (fr words, not Montgomery form) unless a name or a comment says otherwise, as in bbs04_sign.hpp.
#pragma once
#include "bbs04_sign.hpp"       // words_from_be32, store_be32, fr_reduce_words
#include "fr.hpp"
#include "sha3.hpp"

namespace c12381 {

enum { PS_MSG_HASH = 0, PS_MSG_ENCODE = 1 };     // C12381_PS_MSG_HASH / C12381_PS_MSG_ENCODE (include/c12381_hip.h)
constexpr size_t ZP_UNIT_BYTES = 31;             // message bytes per unit of encode_to<Zp>

// encode_to<Zp> (zp_number.hpp:1011-1037): ceil(msg_len / 31) units
C12381_HD size_t encode_zp_units(size_t msg_len) { return (msg_len + ZP_UNIT_BYTES - 1) / ZP_UNIT_BYTES; }
// unit i (i < encode_zp_units(msg_len)) as 32 big-endian bytes: 0x01, then the 31 message bytes of the unit, a short last unit left-aligned
// and zero-filled.  The value is below 2^249, so it is a canonical residue.  Message bytes are read one at a time.
C12381_HD void encode_zp_unit(uint8_t* o32, const uint8_t* msg, size_t msg_len, size_t i) {
    const size_t len = (i + 1) * ZP_UNIT_BYTES <= msg_len ? ZP_UNIT_BYTES : msg_len - i * ZP_UNIT_BYTES;
    o32[0] = 1;
#pragma unroll 1
    for (size_t b = 0; b < ZP_UNIT_BYTES; ++b) o32[1 + b] = b < len ? msg[ZP_UNIT_BYTES * i + b] : 0;
}

// signature = serialize(σ1, σ2) (examples/ps/include/ps.hpp: serialized_field<G1^2>): 49 + 49 bytes
C12381_HD void ps_split_sig(uint8_t* s1_49, uint8_t* s2_49, const uint8_t* sig98) {
#pragma unroll 1
    for (int b = 0; b < 49; ++b) { s1_49[b] = sig98[b]; s2_49[b] = sig98[49 + b]; }
}

// parse<Zp> of a 48-byte wire field (zp_number.hpp:226-236): v = its low 32 bytes as words; returns whether the 384-bit value is below r
// (v is a canonical residue exactly then)
C12381_HD bool zp_parse48(fr& v, const uint8_t* b48) {
    uint32_t hi = 0, w[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) hi |= b48[i];
    words_from_be32(w, b48 + 16);
    fr_set_words(v, w);
    return hi == 0 && !fr_geq_r(w);
}

// number of message scalars of a lane: one digest, or the units of the encoding
C12381_HD size_t ps_msg_scalars(int mode, size_t msg_len) { return mode == PS_MSG_HASH ? 1 : encode_zp_units(msg_len); }
// message scalar i in MONTGOMERY form.  PS_MSG_HASH: SHA3-512 over the msg_len bytes alone (hash_state feeds a span<const char> byte by byte,
// no length prefix, set.hpp:355-384) as a big-endian integer mod r (ps.cpp:20, :29); the full 72-byte blocks are read in aligned 32-bit
// words (sha3.hpp).  PS_MSG_ENCODE: unit i of encode_to<Zp> (ps.cpp:70, :86), read bytewise.
C12381_HD void ps_msg_scalar(fr& m_mont, int mode, const uint8_t* msg, size_t msg_len, size_t i) {
    if (mode == PS_MSG_HASH) {
        uint64_t h[8];
        uint32_t w[16];
        sha3_512(h, msg, msg_len);
        sha3_digest_words_be(w, h);
        fr_from_digest_words(m_mont, w);
    } else {
        uint8_t u[32];
        uint32_t k[8];
        encode_zp_unit(u, msg, msg_len, i);
        words_from_be32(k, u);
        fr_from_words(m_mont, k);
    }
}
// the same as 32 canonical big-endian bytes
C12381_HD void ps_store_msg(uint8_t* o32, int mode, const uint8_t* msg, size_t msg_len, size_t i) {
    if (mode == PS_MSG_HASH) {
        fr m, c;
        uint32_t k[8];
        ps_msg_scalar(m, mode, msg, msg_len, i);
        fr_to_words(k, m);
        fr_set_words(c, k);
        store_be32(o32, c);
    } else {
        encode_zp_unit(o32, msg, msg_len, i);
    }
}

// sign (ps.cpp:17-24, :68-82): h = G^t and σ2 = h^e with e = x + sum_(i < nused) y_i m_i mod r, so σ2 = G^(t e).  t32: the scalar the reference
// draws for h, any value below 2^256, reduced mod r.  x48, y48: serialize(Zp) fields; returns false — t and te are then zero — when x or one
// of the nused y_i fails parse<Zp>'s range check.  nused = ps_msg_scalars(mode, msg_len).
C12381_HD bool ps_sign_scalars(fr& t, fr& te, const uint8_t* x48, const uint8_t* y48, size_t nused, int mode, const uint8_t* msg, size_t msg_len,
                               const uint8_t* t32) {
    fr e, yi;
    bool ok = zp_parse48(e, x48);
#pragma unroll 1
    for (size_t i = 0; i < nused; ++i) ok = zp_parse48(yi, y48 + 48 * i) && ok;
#pragma unroll
    for (int i = 0; i < 8; ++i) { t.w[i] = 0; te.w[i] = 0; }
    if (!ok) return false;
#pragma unroll 1
    for (size_t i = 0; i < nused; ++i) {
        fr m, p;
        zp_parse48(yi, y48 + 48 * i);
        ps_msg_scalar(m, mode, msg, msg_len, i);
        fr_mul(p, m, yi);                            // Montgomery x canonical = canonical
        fr_add(e, e, p);
    }
    uint32_t w[8];
    fr r2, t_mont;
    words_from_be32(w, t32);
    fr_reduce_words(t, w);
    fr_set_words(r2, FR_R2);
    fr_mul(t_mont, t, r2);
    fr_mul(te, t_mont, e);
    return true;
}

}  // namespace c12381
