// TEST HARNESS (host simulation and experiments library only; no product path includes this file): the Fp / Fp2 leaf routines of fp.hpp,
// fp2.hpp and fp2h.hpp behind one op code, on operands given as RAW limbs — the caller chooses the representation (negative limbs, limbs
// above 2^28, values outside [0, p)), not just the residue.  tests/host_sim/fp_raw.cpp runs it on the host under C12381_CHECK_BOUNDS,
// fp_raw_kernel (k_fp_raw.hip) one lane per element and fp2h_raw_kernel two lanes per element on the device; tests/fp_raw_vectors.py holds
// the op table, the vectors and the expected values.
//   x[0..7]  operands (an Fp2 operand is two consecutive elements a, b),  k[0..3] per-lane integers,  r[0..1] results.
//   A predicate or an integer result is returned in r[0].l[0], the 12 words of fp_to_words_be in r[0].l[0..11].
//   FH2_*: the two-lane type of fp2h.hpp (host: both halves in one object; device: one half per lane, partner by DPP), packed as the FR2_* ops;
//   the result is always two elements, and the predicate FH2_IS_ZERO returns the flag of each lane in r[0].l[0] and r[1].l[0].
#pragma once
#include "fp.hpp"
#include "fp2.hpp"
#include "fp2h.hpp"

namespace c12381 {

enum fp_raw_op : int {
    FR_MUL = 0, FR_SQR = 1, FR_MUL2_ADD = 2, FR_MUL2_SUB = 3,
    FR_RED1 = 4, FR_RED2 = 5, FR_RED3 = 6, FR_RED4 = 7,                 // fp_reduce_cols: x0 x1 - x2 x3 + x4 x5 - x6 x7, the first T products
    FR_REDS1 = 8, FR_REDS2 = 9, FR_REDS3 = 10, FR_REDS4 = 11,           // the same through fp_reduce_cols_static
    FR_INJ = 12,                                                       // x0 x1 / R + k0 x2 + k1 x3 + k2 p, multipliers in per-lane registers
    FR_INJ_CONST = 13,                                                 // x0 x1 / R + x2 - 2 x3 + 3 p   (fp_opaque_const multipliers)
    FR_SQR_INJ_CONST = 14,                                             // x0^2 / R - x1 + 2 x2 - 3 p    (fp_opaque_const multipliers)
    FR_INJ_LIT = 15,                                                   // x0 x1 / R + 3 x2 - x3 + 2 p   (literal multipliers)
    FR_QUOT_TOP = 16,                                                  // fp_quot_top(k0)
    FR_NORM1 = 17, FR_NORM1_DBL = 18, FR_MUL_SMALL = 19, FR_WEAK_REDUCE = 20, FR_LINCOMB3P = 21,
    FR_CANON = 22, FR_IS_ZERO = 23, FR_EQUAL = 24, FR_SIGN = 25, FR_TO_WORDS = 26, FR_INV = 27,
    FR_ADD = 28, FR_SUB = 29, FR_NEG = 30,
    FR2_MUL = 32, FR2_SQR = 33, FR2_MUL2_ADD = 34, FR2_MUL2_SUB = 35,
    FR2_MUL_INJ = 36,                                                  // x y + (k0 c.a + k2 p) + (k1 c.b + k3 p) i, c = (x4, x5)
    FR2_MUL_IP = 37, FR2_IS_ZERO = 38, FR2_INV = 39, FR2_SIGN = 40,
    FR_SQR2 = 41, FR_MUL_MSQR2 = 42,                                   // 2 x0^2 / R,  (x0 x1 - 2 x2^2) / R
    FR2_CONJ = 43, FR2_CONJ_MUL_CI = 44, FR2_CONJ_MUL_NEG_I = 45,      // the psi helpers of fp2.hpp: x = (x0, x1), the Fp constant x2
    FR2_CONJ_MUL_A1MI = 46,                                            // neg = k0 != 0
    FR2_MUL_FP = 47, FR2_NORM1_DBL = 48,
    FR_OP_COUNT = 49,                                                  // end of the whole-element codes (fp_raw_kernel)
    // two lanes per element (fp2h.hpp): x = (x0, x1), y = (x2, x3), ...; an Fp operand is x2
    FH2_ADD = 64, FH2_SUB = 65, FH2_NEG = 66, FH2_DBL = 67, FH2_NORM1 = 68,
    FH2_MUL_SMALL = 69,                                                // k0 x
    FH2_SELECT = 70,                                                   // k0 != 0 ? x : y
    FH2_CONJ = 71, FH2_MUL_IP = 72, FH2_IS_ZERO = 73, FH2_MUL = 74, FH2_SQR = 75,
    FH2_MUL2_ADD = 76, FH2_MUL2_SUB = 77,                              // x y +- z w, (z, w) = ((x4, x5), (x6, x7))
    FH2_MUL_FP = 78, FH2_CONJ_MUL_CI = 79, FH2_CONJ_MUL_NEG_I = 80,
    FH2_CONJ_MUL_A1MI = 81,                                            // neg = k0 != 0
    FH2_ONE = 82,                                                      // no operand
    FH2_OP_END = 83
};
constexpr int FR_MAX_IN = 8, FR_MAX_K = 4, FR_MAX_OUT = 2;
C12381_HD bool fp_raw_is_two_lane(int op) { return op >= FH2_ADD && op < FH2_OP_END; }
// operands per lane of each op (0 for QUOT_TOP, FH2_ONE and the unused codes 31 and 49..63)
C12381_HD int fp_raw_arity(int op) {
    switch (op) {
        case FR_MUL: case FR_RED1: case FR_REDS1: case FR_EQUAL: case FR_ADD: case FR_SUB: case FR2_SQR: case FR2_MUL_IP: case FR2_IS_ZERO: case FR2_INV: case FR2_SIGN:
        case FR2_CONJ: case FR2_CONJ_MUL_NEG_I: case FR2_NORM1_DBL: case FH2_NEG: case FH2_DBL: case FH2_NORM1: case FH2_MUL_SMALL: case FH2_CONJ: case FH2_MUL_IP:
        case FH2_IS_ZERO: case FH2_SQR: case FH2_CONJ_MUL_NEG_I: return 2;
        case FR_SQR: case FR_NORM1: case FR_NORM1_DBL: case FR_MUL_SMALL: case FR_WEAK_REDUCE: case FR_CANON: case FR_IS_ZERO: case FR_SIGN: case FR_TO_WORDS: case FR_INV: case FR_NEG: case FR_SQR2: return 1;
        case FR_MUL2_ADD: case FR_MUL2_SUB: case FR_RED2: case FR_REDS2: case FR_INJ: case FR_INJ_CONST: case FR_INJ_LIT: case FR2_MUL: case FH2_ADD: case FH2_SUB: case FH2_SELECT: case FH2_MUL: return 4;
        case FR_RED3: case FR_REDS3: case FR2_MUL_INJ: return 6;
        case FR_RED4: case FR_REDS4: case FR2_MUL2_ADD: case FR2_MUL2_SUB: case FH2_MUL2_ADD: case FH2_MUL2_SUB: return 8;
        case FR_SQR_INJ_CONST: case FR_LINCOMB3P: case FR_MUL_MSQR2: case FR2_CONJ_MUL_CI: case FR2_CONJ_MUL_A1MI: case FR2_MUL_FP:
        case FH2_MUL_FP: case FH2_CONJ_MUL_CI: case FH2_CONJ_MUL_A1MI: return 3;
        default: return 0;
    }
}
C12381_HD bool fp_raw_is_op(int op) { return fp_raw_arity(op) != 0 || op == FR_QUOT_TOP || op == FH2_ONE; }
C12381_HD int fp_raw_outputs(int op) { return (op >= FR2_MUL && op <= FR2_MUL_IP) || op == FR2_INV || (op >= FR2_CONJ && op <= FR2_NORM1_DBL) || fp_raw_is_two_lane(op) ? 2 : 1; }

C12381_HD void fp_raw_flag(fp& r, int32_t v) { fp_zero(r); r.l[0] = v; }
C12381_HD double fp_raw_abs(int32_t k) { return k < 0 ? -(double)k : (double)k; }

template <int T, bool STATIC>
C12381_HD void fp_raw_red(fp& r, const fp (&x)[FR_MAX_IN]) {
    fp t, n2, n6;
    fp_raw_neg(n2, x[2]); fp_raw_neg(n6, x[6]);
    auto col = [&](int k, int64_t& acc) {
        fp_col_acc(acc, x[0], x[1], k);
        if constexpr (T >= 2) fp_col_acc(acc, n2, x[3], k);
        if constexpr (T >= 3) fp_col_acc(acc, x[4], x[5], k);
        if constexpr (T >= 4) fp_col_acc(acc, n6, x[7], k);
    };
    if constexpr (STATIC) fp_reduce_cols_static(t, col); else fp_reduce_cols(t, col);
    C12381_BOUNDS({ double ll = 0, vv = 0;
                    for (int i = 0; i < T; ++i) { check_actual(x[2 * i], "fp_raw_red"); check_actual(x[2 * i + 1], "fp_raw_red");
                                                  ll += x[2 * i].lb * x[2 * i + 1].lb; vv += x[2 * i].vb * x[2 * i + 1].vb; }
                    set_lazy_bounds(t, ll, vv, "fp_raw_red"); })
    r = t;
}

C12381_HD void fp_raw_apply(int op, const fp (&x)[FR_MAX_IN], const int32_t (&k)[FR_MAX_K], fp (&r)[FR_MAX_OUT]) {
    fp_zero(r[0]); fp_zero(r[1]);
    fp2 u, v, w, z, o;
    u.a = x[0]; u.b = x[1]; v.a = x[2]; v.b = x[3]; w.a = x[4]; w.b = x[5]; z.a = x[6]; z.b = x[7];
    switch (op) {
        case FR_MUL: fp_mul(r[0], x[0], x[1]); break;
        case FR_SQR: fp_sqr(r[0], x[0]); break;
        case FR_MUL2_ADD: fp_mul2<false>(r[0], x[0], x[1], x[2], x[3]); break;
        case FR_MUL2_SUB: fp_mul2<true>(r[0], x[0], x[1], x[2], x[3]); break;
        case FR_RED1: fp_raw_red<1, false>(r[0], x); break;
        case FR_RED2: fp_raw_red<2, false>(r[0], x); break;
        case FR_RED3: fp_raw_red<3, false>(r[0], x); break;
        case FR_RED4: fp_raw_red<4, false>(r[0], x); break;
        case FR_REDS1: fp_raw_red<1, true>(r[0], x); break;
        case FR_REDS2: fp_raw_red<2, true>(r[0], x); break;
        case FR_REDS3: fp_raw_red<3, true>(r[0], x); break;
        case FR_REDS4: fp_raw_red<4, true>(r[0], x); break;
        case FR_INJ: {
            const int32_t k0 = k[0], k1 = k[1], k2 = k[2];
            fp_mul_inj(r[0], x[0], x[1], [&](int i, int64_t& acc) { fp_inj(acc, x[2], i, k0); fp_inj(acc, x[3], i, k1); fp_inj_p(acc, i, k2); },
                       C12381_BV(fp_raw_abs(k0) * x[2].vb + fp_raw_abs(k1) * x[3].vb + fp_raw_abs(k2)),
                       C12381_BV(fp_raw_abs(k0) * x[2].lb + fp_raw_abs(k1) * x[3].lb + fp_raw_abs(k2) * 268435456.0));
            break;
        }
        case FR_INJ_CONST: {
            const int32_t c1 = fp_opaque_const(1), cm2 = fp_opaque_const(-2), c3 = fp_opaque_const(3);
            fp_mul_inj(r[0], x[0], x[1], [&](int i, int64_t& acc) { fp_inj(acc, x[2], i, c1); fp_inj(acc, x[3], i, cm2); fp_inj_p(acc, i, c3); },
                       C12381_BV(x[2].vb + 2 * x[3].vb + 3), C12381_BV(x[2].lb + 2 * x[3].lb + 3 * 268435456.0));
            break;
        }
        case FR_SQR_INJ_CONST: {
            const int32_t cm1 = fp_opaque_const(-1), c2 = fp_opaque_const(2), cm3 = fp_opaque_const(-3);
            fp_sqr_inj(r[0], x[0], [&](int i, int64_t& acc) { fp_inj(acc, x[1], i, cm1); fp_inj(acc, x[2], i, c2); fp_inj_p(acc, i, cm3); },
                       C12381_BV(x[1].vb + 2 * x[2].vb + 3), C12381_BV(x[1].lb + 2 * x[2].lb + 3 * 268435456.0));
            break;
        }
        case FR_INJ_LIT:
            fp_mul_inj(r[0], x[0], x[1], [&](int i, int64_t& acc) { fp_inj(acc, x[2], i, 3); fp_inj(acc, x[3], i, -1); fp_inj_p(acc, i, 2); },
                       C12381_BV(3 * x[2].vb + x[3].vb + 2), C12381_BV(3 * x[2].lb + x[3].lb + 2 * 268435456.0));
            break;
        case FR_QUOT_TOP: fp_raw_flag(r[0], fp_quot_top(k[0])); break;
        case FR_NORM1: fp_norm1(r[0], x[0]); break;
        case FR_NORM1_DBL: fp_norm1_dbl(r[0], x[0]); break;
        case FR_MUL_SMALL: fp_mul_small(r[0], x[0], k[0]); break;
        case FR_WEAK_REDUCE: fp_weak_reduce(r[0], x[0]); break;
        case FR_LINCOMB3P:
            fp_lincomb3p(r[0], x[0], k[0], x[1], k[1], x[2], k[2], k[3],
                         C12381_BV(fp_raw_abs(k[0]) * x[0].vb + fp_raw_abs(k[1]) * x[1].vb + fp_raw_abs(k[2]) * x[2].vb + fp_raw_abs(k[3])));
            break;
        case FR_CANON: fp_from_mont_canonical(r[0], x[0]); break;
        case FR_IS_ZERO: fp_raw_flag(r[0], fp_is_zero(x[0]) ? 1 : 0); break;
        case FR_EQUAL: fp_raw_flag(r[0], fp_equal(x[0], x[1]) ? 1 : 0); break;
        case FR_SIGN: fp_raw_flag(r[0], fp_sign(x[0])); break;
        case FR_TO_WORDS: {
            uint32_t wd[12];
            fp_to_words_be(wd, x[0]);
#pragma unroll
            for (int j = 0; j < 12; ++j) r[0].l[j] = (int32_t)wd[j];
            break;
        }
        case FR_INV: fp_inv(r[0], x[0]); break;
        case FR_ADD: fp_add(r[0], x[0], x[1]); break;
        case FR_SUB: fp_sub(r[0], x[0], x[1]); break;
        case FR_NEG: fp_neg(r[0], x[0]); break;
        case FR2_MUL: fp2_mul(o, u, v); r[0] = o.a; r[1] = o.b; break;
        case FR2_SQR: fp2_sqr(o, u); r[0] = o.a; r[1] = o.b; break;
        case FR2_MUL2_ADD: fp2_mul2<false>(o, u, v, w, z); r[0] = o.a; r[1] = o.b; break;
        case FR2_MUL2_SUB: fp2_mul2<true>(o, u, v, w, z); r[0] = o.a; r[1] = o.b; break;
        case FR2_MUL_INJ: {
            const int32_t k0 = k[0], k1 = k[1], k2 = k[2], k3 = k[3];
            fp2_mul_inj(o, u, v, [&](int i, int64_t& acc) { fp_inj(acc, w.a, i, k0); fp_inj_p(acc, i, k2); },
                        [&](int i, int64_t& acc) { fp_inj(acc, w.b, i, k1); fp_inj_p(acc, i, k3); },
                        C12381_INJB(fp_raw_abs(k0) * w.a.vb + fp_raw_abs(k2), fp_raw_abs(k0) * w.a.lb + fp_raw_abs(k2) * 268435456.0),
                        C12381_INJB(fp_raw_abs(k1) * w.b.vb + fp_raw_abs(k3), fp_raw_abs(k1) * w.b.lb + fp_raw_abs(k3) * 268435456.0));
            r[0] = o.a; r[1] = o.b;
            break;
        }
        case FR2_MUL_IP: fp2_mul_ip(o, u); r[0] = o.a; r[1] = o.b; break;
        case FR2_IS_ZERO: fp_raw_flag(r[0], fp2_is_zero(u) ? 1 : 0); break;
        case FR2_INV: fp2_inv(o, u); r[0] = o.a; r[1] = o.b; break;
        case FR2_SIGN: fp_raw_flag(r[0], fp2_sign(u)); break;
        case FR_SQR2: fp_sqr2(r[0], x[0]); break;
        case FR_MUL_MSQR2: fp_mul_msqr2(r[0], x[0], x[1], x[2]); break;
        case FR2_CONJ: fp2_conj(o, u); r[0] = o.a; r[1] = o.b; break;
        case FR2_CONJ_MUL_CI: fp2_conj_mul_ci(o, u, x[2]); r[0] = o.a; r[1] = o.b; break;
        case FR2_CONJ_MUL_NEG_I: fp2_conj_mul_neg_i(o, u); r[0] = o.a; r[1] = o.b; break;
        case FR2_CONJ_MUL_A1MI: fp2_conj_mul_a1mi(o, u, x[2], k[0] != 0); r[0] = o.a; r[1] = o.b; break;
        case FR2_MUL_FP: fp2_mul_fp(o, u, x[2]); r[0] = o.a; r[1] = o.b; break;
        case FR2_NORM1_DBL: fp2_norm1_dbl(o, u); r[0] = o.a; r[1] = o.b; break;
        default: break;
    }
}

// The two-lane ops, written once for both forms of fp2h: the host object holds both halves (the caller takes them out with fp2h_to), a device
// lane holds its own (the caller stores r.v to out[role]).  Every lane is given the whole operands and takes its half with fp2h_from.
#if defined(__HIPCC__)
#define C12381_FH2 __device__ __forceinline__
C12381_FH2 void fp2h_raw_flag(fp2h& r, int32_t v) { fp_raw_flag(r.v, v); }
#else
#define C12381_FH2 inline
C12381_FH2 void fp2h_raw_flag(fp2h& r, int32_t v) { fp_raw_flag(r.h[0], v); fp_raw_flag(r.h[1], v); }
#endif
C12381_FH2 void fp2h_raw_apply(int op, const fp (&x)[FR_MAX_IN], const int32_t (&k)[FR_MAX_K], fp2h& r) {
    fp2 t;
    fp2h u, v, w, z;
    t.a = x[0]; t.b = x[1]; fp2h_from(u, t);
    t.a = x[2]; t.b = x[3]; fp2h_from(v, t);
    t.a = x[4]; t.b = x[5]; fp2h_from(w, t);
    t.a = x[6]; t.b = x[7]; fp2h_from(z, t);
    fp2_zero(r);
    switch (op) {
        case FH2_ADD: fp2_add(r, u, v); break;
        case FH2_SUB: fp2_sub(r, u, v); break;
        case FH2_NEG: fp2_neg(r, u); break;
        case FH2_DBL: fp2_dbl(r, u); break;
        case FH2_NORM1: fp2_norm1(r, u); break;
        case FH2_MUL_SMALL: fp2_mul_small(r, u, k[0]); break;
        case FH2_SELECT: fp2_select(r, k[0] != 0, u, v); break;
        case FH2_CONJ: fp2_conj(r, u); break;
        case FH2_MUL_IP: fp2_mul_ip(r, u); break;
        case FH2_IS_ZERO: fp2h_raw_flag(r, fp2_is_zero(u) ? 1 : 0); break;
        case FH2_MUL: fp2_mul(r, u, v); break;
        case FH2_SQR: fp2_sqr(r, u); break;
        case FH2_MUL2_ADD: fp2_mul2<false>(r, u, v, w, z); break;
        case FH2_MUL2_SUB: fp2_mul2<true>(r, u, v, w, z); break;
        case FH2_MUL_FP: fp2_mul_fp(r, u, x[2]); break;
        case FH2_CONJ_MUL_CI: fp2_conj_mul_ci(r, u, x[2]); break;
        case FH2_CONJ_MUL_NEG_I: fp2_conj_mul_neg_i(r, u); break;
        case FH2_CONJ_MUL_A1MI: fp2_conj_mul_a1mi(r, u, x[2], k[0] != 0); break;
        case FH2_ONE: fp2_one(r); break;
        default: break;
    }
}

}  // namespace c12381
