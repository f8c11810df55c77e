// dct_quant.hpp -- the 8-point Arai butterfly and the quantisers of the front
// kernels (kernels.hip: k_front, k_front_surf, k_dct_blocks; front_ycc.hip:
// k_front_ycc).  Every including file is compiled with -ffp-contract=off (see
// kernels.hip's header comment on floating point).  Device code, and compiled for
// the host by a CPU unit check (tests/native/quant_check.cpp: both quantisers
// against quantize() around every half-integer), which needs the same flag.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DMMT_DQ_FN __device__ __forceinline__
#define DMMT_DQ_FRACT(a) __builtin_amdgcn_fractf(a)
#else
#include <math.h>
#define DMMT_DQ_FN inline
// v_fract_f32 for the host.  Only ever applied to a finite a >= 0 (the operand is
// tested `a < 2^22` first and a NaN fails that test), where a - floor(a) is exact
// and is what the instruction returns.
#define DMMT_DQ_FRACT(a) ((a) - floorf(a))
#endif
#include <stdint.h>

// The two safety margins of the shortcut quantisers below (the literals their
// comments derive).  Overridable only so that the CPU unit check can be built once
// more without them and must then find wrong coefficients.
#ifndef DMMT_QUANT_F32_BAND
#define DMMT_QUANT_F32_BAND 0x1p-20f  // quantize_col8: distance from a half-integer, relative to |t|
#endif
#ifndef DMMT_QUANT_SCALED_BAND
#define DMMT_QUANT_SCALED_BAND 0x1p-21f  // quantize_col8_scaled: the same, added to |t - rint(t)|
#endif
#ifndef DMMT_QUANT_SCALED_HALF
#define DMMT_QUANT_SCALED_HALF 0.49999905f  // 1/2 - 2^-20
#endif
// the unit check's view of which lanes were redone with the division
#ifndef DMMT_QUANT_ON_REDO
#define DMMT_QUANT_ON_REDO(r) ((void)0)
#endif

namespace dmmt {

// quantizer.rs:60: round(d / q) half away from zero, Rust's saturating `as i16`
DMMT_DQ_FN int16_t quantize(float d, float q) {
    float x = roundf(d / q);
    if (x != x) return 0;
    x = fminf(fmaxf(x, -32768.0f), 32767.0f);
    return (int16_t)(int)x;
}

// Image<f32> dots: quantize(d, q) over the 8 rows of one column (row r scaled by
// q[8r], rq[8r] = 1/q) without the division in the common case, branch-free on
// the fast path.  t = d * (1/q) is within 1.5 * 2^-23 * |t| of the correctly
// rounded quotient, so both round alike unless t lies within a * 2^-20 of a
// half-integer.  Round half away from zero of a = |t| is
// trunc(a + 0.5) there, exactly: a < 2^22 and a's fraction is farther than
// a * 2^-20 > ulp(a + 0.5) / 2 from 1/2, so the addition cannot round across an
// integer -- and the rare lanes outside it redone with the division afterwards.
DMMT_DQ_FN void quantize_col8(const float (&v)[8], const float* q, const float* rq, int (&x)[8]) {
    bool slow = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float t = v[r] * rq[8 * r];
        const float a = fabsf(t);
        slow |= !(a < 4194304.0f && fabsf(DMMT_DQ_FRACT(a) - 0.5f) > a * DMMT_QUANT_F32_BAND);
        const float n = copysignf(fminf(truncf(a + 0.5f), 32768.0f), t);  // saturating `as i16` below
        x[r] = (int)fminf(n, 32767.0f);
    }
    if (slow) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float a = fabsf(v[r] * rq[8 * r]);
            if (!(a < 4194304.0f && fabsf(DMMT_DQ_FRACT(a) - 0.5f) > a * DMMT_QUANT_F32_BAND)) {
                DMMT_QUANT_ON_REDO(r);
                x[r] = quantize(v[r], q[8 * r]);
            }
        }
    }
}

// arai.rs:7-26 constants, f32 literals as written in the reference
#define DMMT_A1 0.70710678118654752440f
#define DMMT_A2 0.5411961f
#define DMMT_A3 DMMT_A1
#define DMMT_A4 1.3065629f
#define DMMT_A5 0.3826834f

// arai.rs:85-92 output scaling, by output index
#define DMMT_S0 0.3535533f
#define DMMT_S1 0.2548978f
#define DMMT_S2 0.27059805f
#define DMMT_S3 0.30067244f
#define DMMT_S4 0.35355338f
#define DMMT_S5 0.4499881f
#define DMMT_S6 0.6532815f
#define DMMT_S7 1.2814577f
#ifdef __HIPCC__
static __constant__ float c_arai_scale[8] = {DMMT_S0, DMMT_S1, DMMT_S2, DMMT_S3, DMMT_S4, DMMT_S5, DMMT_S6, DMMT_S7};
#else
static const float c_arai_scale[8] = {DMMT_S0, DMMT_S1, DMMT_S2, DMMT_S3, DMMT_S4, DMMT_S5, DMMT_S6, DMMT_S7};
#endif

// arai.rs:29-84: 8-point AAN butterfly, output k before its scaling factor
DMMT_DQ_FN void arai8_unscaled(float (&v)[8]) {
    const float v10 = v[0] + v[7], v11 = v[1] + v[6], v12 = v[2] + v[5], v13 = v[3] + v[4];
    const float v14 = v[3] - v[4], v15 = v[2] - v[5], v16 = v[1] - v[6], v17 = v[0] - v[7];
    const float v20 = v10 + v13, v21 = v11 + v12, v22 = v11 - v12, v23 = v10 - v13;
    const float v24 = (-v14) - v15, v25 = v15 + v16, v26 = v16 + v17;
    const float v30 = v20 + v21, v31 = v20 - v21, v32 = v22 + v23;
    const float v42 = v32 * DMMT_A1;
    const float v44 = ((-v24) * DMMT_A2) - ((v24 + v26) * DMMT_A5);
    const float v45 = v25 * DMMT_A3;
    const float v46 = (v26 * DMMT_A4) - ((v26 + v24) * DMMT_A5);
    const float v52 = v42 + v23, v53 = v23 - v42, v55 = v45 + v17, v57 = v17 - v45;
    const float v64 = v44 + v57, v65 = v55 + v46, v66 = v55 - v46, v67 = v57 - v44;
    v[0] = v30;
    v[4] = v31;
    v[2] = v52;
    v[6] = v53;
    v[5] = v64;
    v[1] = v65;
    v[7] = v66;
    v[3] = v67;
}

// arai.rs:29-92: the butterfly with its output scaling
DMMT_DQ_FN void arai8(float (&v)[8]) {
    arai8_unscaled(v);
    v[0] = v[0] * DMMT_S0;
    v[1] = v[1] * DMMT_S1;
    v[2] = v[2] * DMMT_S2;
    v[3] = v[3] * DMMT_S3;
    v[4] = v[4] * DMMT_S4;
    v[5] = v[5] * DMMT_S5;
    v[6] = v[6] * DMMT_S6;
    v[7] = v[7] * DMMT_S7;
}

// Quantisation for integer samples, whose coefficients are bounded: the samples
// normalise into [0, 1] (a larger one is an error, color.rs:63-65), so Y, Cb, Cr
// lie in [-128, 128] and every FDCT output in [-2048, 2048] (DC = sum / 8, AC at
// most (1/4) * 64 * 128), to within a few ulps; with q >= 1, |d/q| <= 2049 and
// the saturation of `as i16` cannot trigger.
// The column pass's output scaling is folded into the reciprocal: u = the
// unscaled column outputs (arai8_unscaled, the reference's butterfly values),
// crq[8r] = fl(scale_r * fl(1/q)).  t = fl(u * crq) and the reference's
// fl(fl(u * scale_r) / q) are both the exact quotient u * scale_r / q times at
// most three, resp. two, factors (1 + d), |d| <= 2^-24, so they lie within
// 5.0001 * 2^-24 * |t| < 2^-21 * |t| of each other.  Where
// |t - rint(t)| + 2^-21 * |t| < 1/2 the reference's quotient therefore lies in the
// same open interval (n - 1/2, n + 1/2) around n = rint(t): no tie, and round half
// away from zero gives n.  Both terms are exact in f32 (Sterbenz; a power-of-two
// scaling; one fma) and their sum rounds by at most 2^-25, covered by testing against
// 1/2 - 2^-20.  The margin scales with |t|: small coefficients -- nearly all of
// them -- take the exact path only within ~|t| * 2^-20 of a half-integer, so a wave
// almost never has a lane there.  The other lanes (and NaN: maxval 0, q 0) redo d
// and the division afterwards.
// The eight distances are folded with max before one compare; a NaN (only from
// 0/0, maxval 0: `nan_possible`) would vanish in the max, so that case always
// takes the exact path.
DMMT_DQ_FN float quant_margin(float t, float n) {
    return __builtin_fmaf(fabsf(t), DMMT_QUANT_SCALED_BAND, fabsf(t - n));  // (the product is exact: one rounding)
}
// FOLD: also `mag` = the eight results as floats folded row by row, mag = fold(mag,
// r, result) from 0 -- k_front's narrow store tests the column's range on it
// (coef_format.hpp: coef_hi_mag_row).  The rintf results are in registers before
// their conversion, and the rare exact path folds its own results again.
template <bool FOLD, class Fold>
DMMT_DQ_FN void quantize_col8_scaled_impl(const float (&u)[8], const float* q, const float* crq, bool nan_possible,
                                          int (&x)[8], const Fold& fold, float& mag) {
    float dist = 0.0f;
    if constexpr (FOLD) mag = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float t = u[r] * crq[8 * r];
        const float n = __builtin_rintf(t);
        dist = fmaxf(dist, quant_margin(t, n));
        x[r] = (int)n;
        if constexpr (FOLD) mag = fold(mag, r, n);
    }
#ifdef __HIP_DEVICE_COMPILE__
    // (the fold stays here: sunk past the branch below, as the compiler would have it,
    // it keeps the eight floats alive beside x and u across the exact path)
    if constexpr (FOLD) asm volatile("" : "+v"(mag));
#endif
    if (nan_possible || !(dist < DMMT_QUANT_SCALED_HALF)) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float t = u[r] * crq[8 * r];
            if (!(quant_margin(t, __builtin_rintf(t)) < DMMT_QUANT_SCALED_HALF)) {
                DMMT_QUANT_ON_REDO(r);
                x[r] = quantize(u[r] * c_arai_scale[r], q[8 * r]);
            }
        }
        if constexpr (FOLD) {
            mag = 0.0f;
#pragma unroll
            for (int r = 0; r < 8; ++r) mag = fold(mag, r, (float)x[r]);
        }
    }
}
DMMT_DQ_FN void quantize_col8_scaled(const float (&u)[8], const float* q, const float* crq, bool nan_possible,
                                     int (&x)[8]) {
    float mag;
    quantize_col8_scaled_impl<false>(u, q, crq, nan_possible, x, 0, mag);
}
template <class Fold>
DMMT_DQ_FN void quantize_col8_scaled_fold(const float (&u)[8], const float* q, const float* crq, bool nan_possible,
                                          int (&x)[8], const Fold& fold, float& mag) {
    quantize_col8_scaled_impl<true>(u, q, crq, nan_possible, x, fold, mag);
}

}  // namespace dmmt
