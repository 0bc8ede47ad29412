// TEST HARNESS (CPU): the Fp / Fp2 leaf routines (fp.hpp, fp2.hpp, and fp2h.hpp in its host form) on RAW limbs under C12381_CHECK_BOUNDS, one op
// code per routine (csrc/fp_raw_ops.hpp, shared with the device kernels fp_raw_kernel and fp2h_raw_kernel).  Operands come with their DECLARED bounds (lb = max |limb|,
// vb = |value| / p) and results go back with the bounds the routines declare.  bounds_fail aborts the process, so every precondition is
// checked here first and a lane outside one is reported (return 1, *bad_lane) instead of run.  Not a product path.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../crypto12381_amd/csrc/fp_raw_ops.hpp"

using namespace c12381;

namespace {
constexpr double T28 = 268435456.0, T31 = 2147483648.0, T56 = 72057594037927936.0, T40 = 1099511627776.0, T63 = 9223372036854775808.0, T62 = 4611686018427387904.0;
bool act(const fp& a) {
    for (int i = 0; i < NL; ++i) if (std::fabs((double)a.l[i]) > a.lb) return false;
    return fp_actual_vb(a) <= a.vb * 1.0000001 + 1e-9 && a.lb <= T31;
}
bool col(double ll, double inj = 0) { return 14.0 * ll + 14.0 * T56 + T40 + inj < T63; }
bool val(double vv) { return vv <= 1.0e6; }
bool topok(double vb) { return vb * TOP_PER_P + 2.0 <= T31; }
double ab(int32_t k) { return fp_raw_abs(k); }

bool precondition(int op, const fp (&x)[FR_MAX_IN], const int32_t (&k)[FR_MAX_K]) {
    const int ar = fp_raw_arity(op);
    for (int i = 0; i < ar; ++i) if (!act(x[i])) return false;
    auto L = [&](int i) { return x[i].lb; };
    auto V = [&](int i) { return x[i].vb; };
    switch (op) {
        case FR_MUL: case FR_RED1: case FR_REDS1: return col(L(0) * L(1)) && val(V(0) * V(1));
        case FR_SQR: return col(L(0) * L(0)) && val(V(0) * V(0)) && 2 * L(0) < T31;
        case FR_MUL2_ADD: case FR_MUL2_SUB: case FR_RED2: case FR_REDS2: return col(L(0) * L(1) + L(2) * L(3)) && val(V(0) * V(1) + V(2) * V(3));
        case FR_RED3: case FR_REDS3: return col(L(0) * L(1) + L(2) * L(3) + L(4) * L(5)) && val(V(0) * V(1) + V(2) * V(3) + V(4) * V(5));
        case FR_RED4: case FR_REDS4: return col(L(0) * L(1) + L(2) * L(3) + L(4) * L(5) + L(6) * L(7)) && val(V(0) * V(1) + V(2) * V(3) + V(4) * V(5) + V(6) * V(7));
        case FR_INJ: return col(L(0) * L(1), ab(k[0]) * L(2) + ab(k[1]) * L(3) + ab(k[2]) * T28) && val(V(0) * V(1))
                            && topok(V(0) * V(1) * P_OVER_R + 1 + ab(k[0]) * V(2) + ab(k[1]) * V(3) + ab(k[2]));
        case FR_INJ_CONST: return col(L(0) * L(1), L(2) + 2 * L(3) + 3 * T28) && val(V(0) * V(1)) && topok(V(0) * V(1) * P_OVER_R + 1 + V(2) + 2 * V(3) + 3);
        case FR_INJ_LIT: return col(L(0) * L(1), 3 * L(2) + L(3) + 2 * T28) && val(V(0) * V(1)) && topok(V(0) * V(1) * P_OVER_R + 1 + 3 * V(2) + V(3) + 2);
        case FR_SQR_INJ_CONST: return col(L(0) * L(0), L(1) + 2 * L(2) + 3 * T28) && val(V(0) * V(0)) && 2 * L(0) < T31 && topok(V(0) * V(0) * P_OVER_R + 1 + V(1) + 2 * V(2) + 3);
        case FR_QUOT_TOP: return true;
        case FR_NORM1: return V(0) * TOP_PER_P + 4.0 + std::floor(L(0) / T28) <= T31;
        case FR_NORM1_DBL: return 2 * V(0) * TOP_PER_P + 6.0 + std::floor(2 * L(0) / T28) <= T31 && std::fabs((double)x[0].l[NL - 1]) < T31 / 2 - 16;
        case FR_MUL_SMALL: return k[0] >= 0 && topok(V(0) * k[0]);
        case FR_WEAK_REDUCE: return V(0) <= 2400.0 && V(0) * TOP_PER_P + 4.0 + std::floor(L(0) / T28) <= T31;
        case FR_LINCOMB3P: return topok(ab(k[0]) * V(0) + ab(k[1]) * V(1) + ab(k[2]) * V(2) + ab(k[3]))
                                  && ab(k[0]) * L(0) + ab(k[1]) * L(1) + ab(k[2]) * L(2) + ab(k[3]) * T28 < T62;
        case FR_CANON: case FR_IS_ZERO: case FR_SIGN: case FR_TO_WORDS: case FR_INV: return col(L(0)) && val(V(0) * 1e-100);
        case FR_EQUAL: return L(0) + L(1) <= T31 && col(L(0) + L(1));
        case FR_ADD: case FR_SUB: case FR2_MUL_IP: return L(0) + L(1) <= T31;
        case FR_NEG: return true;
        case FR2_MUL: return col(L(0) * L(2) + L(1) * L(3)) && val(V(0) * V(2) + V(1) * V(3)) && col(L(0) * L(3) + L(1) * L(2)) && val(V(0) * V(3) + V(1) * V(2));
        case FR2_MUL_INJ: return col(L(0) * L(2) + L(1) * L(3), ab(k[0]) * L(4) + ab(k[2]) * T28) && val(V(0) * V(2) + V(1) * V(3))
                                 && col(L(0) * L(3) + L(1) * L(2), ab(k[1]) * L(5) + ab(k[3]) * T28) && val(V(0) * V(3) + V(1) * V(2))
                                 && topok((V(0) * V(2) + V(1) * V(3)) * P_OVER_R + 1 + ab(k[0]) * V(4) + ab(k[2]))
                                 && topok((V(0) * V(3) + V(1) * V(2)) * P_OVER_R + 1 + ab(k[1]) * V(5) + ab(k[3]));
        case FR2_SQR: return col(L(0) * L(0) + L(1) * L(1)) && val(V(0) * V(0) + V(1) * V(1)) && col(2 * L(0) * L(1)) && val(2 * V(0) * V(1)) && 2 * L(0) < T31 && 2 * L(1) < T31;
        case FR2_MUL2_ADD: case FR2_MUL2_SUB:
            return col(L(0) * L(2) + L(1) * L(3) + L(4) * L(6) + L(5) * L(7)) && val(V(0) * V(2) + V(1) * V(3) + V(4) * V(6) + V(5) * V(7))
                   && col(L(0) * L(3) + L(1) * L(2) + L(4) * L(7) + L(5) * L(6)) && val(V(0) * V(3) + V(1) * V(2) + V(4) * V(7) + V(5) * V(6));
        case FR2_IS_ZERO: case FR2_SIGN: return col(L(0)) && col(L(1));
        case FR2_INV: return col(L(0) * L(0) + L(1) * L(1)) && val(V(0) * V(0) + V(1) * V(1)) && 2 * L(0) < T31 && 2 * L(1) < T31
                             && col(L(0) * T28) && col(L(1) * T28) && val(V(0) * 1.001) && val(V(1) * 1.001);
        case FR_SQR2: return col(2 * L(0) * L(0)) && val(2 * V(0) * V(0)) && 2 * L(0) < T31;                   // fp_mul(a, 2a)
        case FR_MUL_MSQR2: return col(L(0) * L(1) + 2 * L(2) * L(2)) && val(V(0) * V(1) + 2 * V(2) * V(2)) && 4 * L(2) < T31;   // -4c is formed as raw limbs
        case FR2_CONJ: case FR2_CONJ_MUL_NEG_I: case FH2_NEG: case FH2_SELECT: case FH2_CONJ: case FH2_CONJ_MUL_NEG_I: case FH2_ONE: return true;
        case FR2_MUL_FP: case FR2_CONJ_MUL_CI: case FH2_MUL_FP: case FH2_CONJ_MUL_CI: return col(L(0) * L(2)) && col(L(1) * L(2)) && val(V(0) * V(2)) && val(V(1) * V(2));
        // the product operand is y.a -+ y.b, limb bound LB(y.a) + LB(y.b)
        case FR2_CONJ_MUL_A1MI: case FH2_CONJ_MUL_A1MI: return L(0) + L(1) <= T31 && col((L(0) + L(1)) * L(2)) && val((V(0) + V(1)) * V(2));
        case FR2_NORM1_DBL:
            for (int e = 0; e < 2; ++e)
                if (!(2 * V(e) * TOP_PER_P + 6.0 + std::floor(2 * L(e) / T28) <= T31 && std::fabs((double)x[e].l[NL - 1]) < T31 / 2 - 16)) return false;
            return true;
        case FH2_ADD: case FH2_SUB: return L(0) + L(2) <= T31 && L(1) + L(3) <= T31;
        case FH2_DBL: return 2 * L(0) <= T31 && 2 * L(1) <= T31;
        case FH2_NORM1: return V(0) * TOP_PER_P + 4.0 + std::floor(L(0) / T28) <= T31 && V(1) * TOP_PER_P + 4.0 + std::floor(L(1) / T28) <= T31;
        case FH2_MUL_SMALL: return k[0] >= 0 && topok(V(0) * k[0]) && topok(V(1) * k[0]);
        case FH2_MUL_IP: return L(0) + L(1) <= T31;
        case FH2_IS_ZERO: return col(L(0)) && col(L(1));
        // fp2h_lane_uv takes U and V by fp_select, whose declared bounds are the larger of the two halves of y: own * U + partner * V is
        // (LBx.a + LBx.b) max(LBy.a, LBy.b) on both lanes
        case FH2_MUL: return col((L(0) + L(1)) * std::fmax(L(2), L(3))) && val((V(0) + V(1)) * std::fmax(V(2), V(3)));
        // (a + b)(a - b) on the real lane, (2a) b on the imaginary lane, the left factor by fp_select: max(2 LB partner, LBa + LBb) (LBa + LBb)
        case FH2_SQR: {
            const double sl = L(0) + L(1), sv = V(0) + V(1);
            return sl <= T31 && 2 * L(0) <= T31 && 2 * L(1) <= T31 && col(std::fmax(2 * L(0), sl) * sl) && col(std::fmax(2 * L(1), sl) * sl)
                   && val(std::fmax(2 * V(0), sv) * sv) && val(std::fmax(2 * V(1), sv) * sv);
        }
        case FH2_MUL2_ADD: case FH2_MUL2_SUB:
            return col((L(0) + L(1)) * std::fmax(L(2), L(3)) + (L(4) + L(5)) * std::fmax(L(6), L(7)))
                   && val((V(0) + V(1)) * std::fmax(V(2), V(3)) + (V(4) + V(5)) * std::fmax(V(6), V(7)));
        default: return false;
    }
}
}  // namespace

extern "C" {

// in [n][arity][14] limbs, in_b [n][arity][2] = (lb, vb) declared, k [n][4]; out [n][outputs][14], out_b [n][outputs][2] = the bounds the
// routine declares for its result (0, 0 for predicates).  Returns 0; 1 when lane *bad_lane is outside the op's precondition (nothing
// is run from that lane on); -1 for an unknown op.
int sim_fp_raw_batch(int op, size_t n, const int32_t* in, const double* in_b, const int32_t* kk, int32_t* out, double* out_b, long long* bad_lane) {
    const int ar = fp_raw_arity(op), no = fp_raw_outputs(op);
    if (!fp_raw_is_op(op)) return -1;
    for (size_t i = 0; i < n; ++i) {
        fp x[FR_MAX_IN], r[FR_MAX_OUT];
        int32_t k[FR_MAX_K];
        for (int e = 0; e < FR_MAX_IN; ++e) fp_zero(x[e]);
        for (int e = 0; e < ar; ++e) {
            std::memcpy(x[e].l, in + (i * ar + e) * NL, sizeof(int32_t) * NL);
            x[e].lb = in_b[(i * ar + e) * 2]; x[e].vb = in_b[(i * ar + e) * 2 + 1];
        }
        std::memcpy(k, kk + i * FR_MAX_K, sizeof k);
        if (!precondition(op, x, k)) { *bad_lane = (long long)i; return 1; }
        if (fp_raw_is_two_lane(op)) {            // the host form of fp2h: both halves in one object, the per-lane routines once per role
            fp2h h; fp2 t;
            fp2h_raw_apply(op, x, k, h);
            fp2h_to(t, h);
            r[0] = t.a; r[1] = t.b;
        } else {
            fp_raw_apply(op, x, k, r);
        }
        for (int e = 0; e < no; ++e) {
            std::memcpy(out + (i * no + e) * NL, r[e].l, sizeof(int32_t) * NL);
            out_b[(i * no + e) * 2] = r[e].lb; out_b[(i * no + e) * 2 + 1] = r[e].vb;
        }
    }
    return 0;
}

// max over top in [lo, hi) of |top 2^364 - fp_quot_top(top) p| / p, with p / 2^364 taken to 56 fractional bits (relative error below 2^-72)
double sim_fp_quot_top_worst(long long lo, long long hi, int32_t* worst_top) {
    const __int128 U = ((__int128)FP_P[13] << 56) + ((__int128)FP_P[12] << 28) + FP_P[11];
    __int128 worst = -1;
    for (long long t = lo; t < hi; ++t) {
        const int32_t q = fp_quot_top((int32_t)t);
        __int128 e = ((__int128)t << 56) - (__int128)q * U;
        if (e < 0) e = -e;
        if (e > worst) { worst = e; *worst_top = (int32_t)t; }
    }
    return (double)((long double)worst / (long double)U);
}

}  // extern "C"
