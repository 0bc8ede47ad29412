// TEST HARNESS (CPU): the Jacobian doubling of g1.hpp (g1j_dbl: Y^4 folded into the reduction of Y3) and its primitive fp_mul_msqr2
// (fp.hpp), compiled for the host with C12381_CHECK_BOUNDS.  Not a product path.
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
// homogeneous (X : Y : Z) -> 96 affine bytes, all-zero for Z = 0
void hom_out(uint8_t* o, const g1p& p) {
    if (fp_is_zero(p.z)) { std::memset(o, 0, 96); return; }
    fp zn, zi, ax, ay;
    fp_norm1(zn, p.z);
    fp_inv(zi, zn);
    g1_to_affine(ax, ay, p, zi);
    store48(o, ax); store48(o + 48, ay);
}

}  // namespace

extern "C" {

// n lanes: the affine point (x, y) of pts96 on the Jacobian Z of zs48 (X = x Z^2, Y = y Z^3: reduction outputs; Z = 0 keeps X = x,
// Y = y so that the doubling sees arbitrary coordinates beside it) through g1j_dbl -> out_j, and (x : y : 1) through the complete
// g1_dbl -> out_c, both as 96 affine bytes (all-zero = Z3 is 0 mod p).
int sim_dblfold_cmp(size_t n, const uint8_t* pts96, const uint8_t* zs48, uint8_t* out_j, uint8_t* out_c) {
    for (size_t i = 0; i < n; ++i) {
        fp x, y, z, z2, z3;
        load48(x, pts96 + 96 * i); load48(y, pts96 + 96 * i + 48); load48(z, zs48 + 48 * i);
        g1j a;
        if (fp_is_zero(z)) {
            a.x = x; a.y = y; a.z = z;
        } else {
            fp_sqr(z2, z); fp_mul(z3, z2, z);
            fp_mul(a.x, x, z2); fp_mul(a.y, y, z3); a.z = z;
        }
        g1j_dbl(a);
        jac_out(out_j + 96 * i, a);
        g1p c;
        c.x = x; c.y = y; fp_one(c.z);
        g1_dbl(c);
        hom_out(out_c + 96 * i, c);
    }
    return 0;
}

// The window loop's chain on one lane: acc = P (Z = 1), then `windows` times five doublings and one mixed addition of Q, so that the
// doublings read reduction outputs and g1j_madd outputs as they do in g1_scalar_mul.  acc -> 96 affine bytes.
int sim_dblfold_chain(const uint8_t* p96, const uint8_t* q96, int windows, uint8_t* out96) {
    fp qx, qy;
    g1j a;
    load48(a.x, p96); load48(a.y, p96 + 48); fp_one(a.z);
    load48(qx, q96); load48(qy, q96 + 48);
    for (int w = 0; w < windows; ++w) {
        g1j_dbl_window(a);
        g1j r;
        g1j_madd(r, a, qx, qy);
        a = r;
    }
    jac_out(out96, a);
    return 0;
}

// fp_mul_msqr2 on raw limbs: in [n][3][14] = a, b, c with their DECLARED bounds in_b [n][3][2] = (lb, vb); out [n][14] raw result limbs,
// out_b [n][2] the bounds the primitive declares.  Nothing is checked here first: a lane outside the precondition aborts the process
// (bounds_fail), which is what the caller of such a lane wants to see.
int sim_dblfold_msqr2(size_t n, const int32_t* in, const double* in_b, int32_t* out, double* out_b) {
    for (size_t i = 0; i < n; ++i) {
        fp v[3], r;
        for (int e = 0; e < 3; ++e) {
            for (int j = 0; j < NL; ++j) v[e].l[j] = in[(3 * i + e) * NL + j];
            v[e].lb = in_b[(3 * i + e) * 2]; v[e].vb = in_b[(3 * i + e) * 2 + 1];
        }
        fp_mul_msqr2(r, v[0], v[1], v[2]);
        for (int j = 0; j < NL; ++j) out[i * NL + j] = r.l[j];
        out_b[2 * i] = r.lb; out_b[2 * i + 1] = r.vb;
    }
    return 0;
}

}  // extern "C"
