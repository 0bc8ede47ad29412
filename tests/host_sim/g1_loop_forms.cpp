// TEST HARNESS (CPU): the forms of the G1 window loop — fp_sqr2 (fp.hpp: a square times two), g1j_dbl with G = 2Y^2 from it, and the
// g1j_madd beside it (g1.hpp) — compiled for the host with C12381_CHECK_BOUNDS.  Not a product path.
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/fp.hpp"
#include "../../crypto12381_amd/csrc/codec.hpp"
#include "../../crypto12381_amd/csrc/g1.hpp"

using namespace c12381;

namespace {

void load48(fp& r, const uint8_t* b) {
    uint32_t w[12];
    std::memcpy(w, b, 48);
    fp_from_raw48(r, w);
}
void store48(uint8_t* b, const fp& a) {
    uint32_t w[12];
    fp_to_raw48(w, a);
    std::memcpy(b, w, 48);
}
// Jacobian (X : Y : Z) -> 96 affine bytes (X / Z^2, Y / Z^3), all-zero for Z = 0
void jac_out(uint8_t* o, const g1j& p) {
    if (fp_is_zero(p.z)) { std::memset(o, 0, 96); return; }
    fp zi, zi2, zi3, ax, ay;
    fp_inv(zi, p.z);
    fp_sqr(zi2, zi);
    fp_mul(zi3, zi2, zi);
    fp_mul(ax, p.x, zi2);
    fp_mul(ay, p.y, zi3);
    store48(o, ax); store48(o + 48, ay);
}
// the affine point (x, y) of p96 on the Jacobian Z of z48 (X = x Z^2, Y = y Z^3: reduction outputs); Z = 0 keeps X = x, Y = y
void jac_in(g1j& a, const uint8_t* p96, const uint8_t* z48) {
    fp x, y, z, z2, z3;
    load48(x, p96); load48(y, p96 + 48); load48(z, z48);
    if (fp_is_zero(z)) { a.x = x; a.y = y; a.z = z; return; }
    fp_sqr(z2, z); fp_mul(z3, z2, z);
    fp_mul(a.x, x, z2); fp_mul(a.y, y, z3); a.z = z;
}
void limbs_out(int32_t* o, const g1j& p) {
    for (int j = 0; j < NL; ++j) { o[j] = p.x.l[j]; o[NL + j] = p.y.l[j]; o[2 * NL + j] = p.z.l[j]; }
}

// The doubling as it stood before G = 2Y^2 came from fp_sqr2: G as the general product Y (2Y).  The comparison of the raw-limb test.
void g1j_dbl_parent(g1j& p) {
    fp a, g, d, e, x3, y3, z3, y2;
    const int32_t cm4 = fp_opaque_const(-4);
    fp_raw_dbl(y2, p.y);
    fp_mul(z3, y2, p.z);
    fp_sqr(a, p.x);
    fp_mul(g, p.y, y2);
    fp_mul(d, p.x, g);
    fp_mul_small(e, a, 3);
    fp_sqr_inj(x3, e, [&](int i, int64_t& acc) { fp_inj(acc, d, i, cm4); }, C12381_BV(4 * d.vb), C12381_BV(4 * d.lb));
    fp_raw_dbl(d, d);
    fp_sub(d, d, x3);
    fp_mul_msqr2(y3, e, d, g);
    p.x = x3; p.y = y3; p.z = z3;
}

}  // namespace

extern "C" {

// fp_sqr2 on raw limbs: in [n][14] = a with its DECLARED bounds in_b [n][2] = (lb, vb); out_s [n][14] the limbs of fp_sqr2(a), out_m [n][14]
// those of fp_mul(a, fp_raw_dbl(a)), out_b [n][4] the bounds (lb, vb) each declares.  Nothing is checked here first: a lane outside the
// precondition aborts the process (bounds_fail).
int sim_lf_sqr2(size_t n, const int32_t* in, const double* in_b, int32_t* out_s, int32_t* out_m, double* out_b) {
    for (size_t i = 0; i < n; ++i) {
        fp a, d, rs, rm;
        for (int j = 0; j < NL; ++j) a.l[j] = in[i * NL + j];
        a.lb = in_b[2 * i]; a.vb = in_b[2 * i + 1];
        fp_sqr2(rs, a);
        fp_raw_dbl(d, a);
        fp_mul(rm, a, d);
        for (int j = 0; j < NL; ++j) { out_s[i * NL + j] = rs.l[j]; out_m[i * NL + j] = rm.l[j]; }
        out_b[4 * i] = rs.lb; out_b[4 * i + 1] = rs.vb; out_b[4 * i + 2] = rm.lb; out_b[4 * i + 3] = rm.vb;
    }
    return 0;
}

// n lanes through g1j_dbl and through the parent form: raw limbs X | Y | Z (42 words a lane) of each, and g1j_dbl's result as 96 affine bytes
int sim_lf_dbl_cmp(size_t n, const uint8_t* pts96, const uint8_t* zs48, int32_t* out_new, int32_t* out_parent, uint8_t* out96) {
    for (size_t i = 0; i < n; ++i) {
        g1j a, b;
        jac_in(a, pts96 + 96 * i, zs48 + 48 * i);
        b = a;
        g1j_dbl(a);
        g1j_dbl_parent(b);
        limbs_out(out_new + 42 * i, a);
        limbs_out(out_parent + 42 * i, b);
        jac_out(out96 + 96 * i, a);
    }
    return 0;
}

// n lanes: acc (affine acc96 on the Jacobian Z of zs48) + q (affine) by g1j_madd -> out1 as 96 affine bytes (all-zero = Z3 is 0 mod p),
// then a doubling and the addition of q2 -> out2 likewise
int sim_lf_madd(size_t n, const uint8_t* acc96, const uint8_t* zs48, const uint8_t* q96, const uint8_t* q2_96, uint8_t* out1, uint8_t* out2) {
    for (size_t i = 0; i < n; ++i) {
        g1j a, r;
        fp qx, qy;
        jac_in(a, acc96 + 96 * i, zs48 + 48 * i);
        load48(qx, q96 + 96 * i); load48(qy, q96 + 96 * i + 48);
        g1j_madd(r, a, qx, qy);
        jac_out(out1 + 96 * i, r);
        g1j_dbl(r);
        load48(qx, q2_96 + 96 * i); load48(qy, q2_96 + 96 * i + 48);
        g1j_madd(a, r, qx, qy);
        jac_out(out2 + 96 * i, a);
    }
    return 0;
}

// The window loop's chain on one lane: acc = P (Z = 1), then `windows` times five doublings and the mixed additions of Q0 and Q1, as
// g1_scalar_mul runs them.  acc -> 96 affine bytes.
int sim_lf_chain(const uint8_t* p96, const uint8_t* q0_96, const uint8_t* q1_96, int windows, uint8_t* out96) {
    fp x0, y0, x1, y1;
    g1j a, r;
    load48(a.x, p96); load48(a.y, p96 + 48); fp_one(a.z);
    load48(x0, q0_96); load48(y0, q0_96 + 48);
    load48(x1, q1_96); load48(y1, q1_96 + 48);
    for (int w = 0; w < windows; ++w) {
        g1j_dbl_window(a);
        g1j_madd(r, a, x0, y0);
        g1j_madd(a, r, x1, y1);
    }
    jac_out(out96, a);
    return 0;
}

}  // extern "C"
