// CPU unit check of the front kernels' shortcut quantisers (csrc/dct_quant.hpp,
// compiled for the host from the kernel's own header): quantize_col8_scaled
// (integer samples, the YCbCr front) and quantize_col8 (Image<f32> dots) against
// quantizer.rs:60, round(d / q) half away from zero with the saturating cast, at
// the inputs where the shortcut and the division can part: a few ulps either side
// of every half-integer quotient, for every q in 1..255 and every row scaling, plus
// random inputs and -- for the f32 path, whose input is any float -- the ends of the
// i16 range, the 2^22 limit of the fast path, zeros, denormals, FLT_MAX, Inf and NaN.
//
// The reference value is computed here, in double: a double quotient of two floats
// rounds to the correctly rounded f32 quotient (53 >= 2 * 24 + 2 bits), and the
// header's own quantize() (the kernels' exact path) is held against it too.
//
// Build with -ffp-contract=off (as every file that includes the header).  Built once
// more with the margins removed (-DDMMT_QUANT_F32_BAND=0.0f
// -DDMMT_QUANT_SCALED_BAND=0.0f -DDMMT_QUANT_SCALED_HALF=0.5f) it must find wrong
// coefficients and exit 1.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned g_redo;  // bit r: the header redid lane r with the division
#define DMMT_QUANT_ON_REDO(r) (g_redo |= 1u << (r))
#include "../../dmmt-jpeg-encoder_amd/csrc/dct_quant.hpp"

namespace {

// quantizer.rs:60 `(d / q as f32).round() as i16`
int ref_quantize(float d, float q) {
    const float quot = (float)((double)d / (double)q);  // the correctly rounded f32 division
    if (quot != quot) return 0;
    const double a = fabs((double)quot);
    double n = floor(a);
    if (a - n >= 0.5) n += 1.0;  // half away from zero (a - n is exact)
    if (quot < 0) n = -n;
    if (n > 32767.0) return 32767;
    if (n < -32768.0) return -32768;
    return (int)n;
}

float from_bits(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
uint32_t to_bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}
// k ulps from a finite positive x, towards larger magnitude for k > 0 (never across 0)
float step_ulps(float x, int k) {
    const int64_t b = (int64_t)to_bits(x) + k;
    return from_bits((uint32_t)(b < 0 ? 0 : b));
}

struct Rng {  // xorshift64*
    uint64_t s;
    uint32_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    }
    double unit() { return next() * (1.0 / 4294967296.0); }
};

struct Counts {
    const char* name;
    long long lanes = 0, fast = 0, redone = 0, fast_differs = 0, fast_differs_not_redone = 0, mismatches = 0;
    long long exact_path_wrong = 0;  // the header's quantize() against the double reference
    void lane(int got, int fastv, bool redo, int want, int hdr_exact, float in, float q, int r) {
        ++lanes;
        if (redo) ++redone; else ++fast;
        if (fastv != want) {
            ++fast_differs;
            if (!redo) ++fast_differs_not_redone;
        }
        if (hdr_exact != want) ++exact_path_wrong;
        if (got != want) {
            if (mismatches < 8)
                printf("  %s mismatch: in=%a q=%g row=%d got=%d want=%d fast=%d redone=%d\n", name, (double)in, (double)q,
                       r, got, want, fastv, (int)redo);
            ++mismatches;
        }
    }
    bool report() const {
        printf("%s: lanes=%lld fast=%lld redone=%lld fast_differs=%lld fast_differs_not_redone=%lld mismatches=%lld "
               "exact_path_wrong=%lld\n",
               name, lanes, fast, redone, fast_differs, fast_differs_not_redone, mismatches, exact_path_wrong);
        return mismatches == 0 && fast_differs_not_redone == 0 && exact_path_wrong == 0;
    }
};

Counts cs{"scaled"}, cf{"f32"};
int qstep = 1;  // `quant_check N`: every N-th q only (the build without margins fails on any of them)

// ---- quantize_col8_scaled: row r holds u[r], the column pass's unscaled output
void scaled_call(const float (&u)[8], const float* q, const float* crq, bool nan_possible) {
    int x[8];
    g_redo = 0;
    dmmt::quantize_col8_scaled(u, q, crq, nan_possible, x);
    for (int r = 0; r < 8; ++r) {
        const float d = u[r] * dmmt::c_arai_scale[r];  // the reference's coefficient
        const int fastv = (int)__builtin_rintf(u[r] * crq[8 * r]);
        cs.lane(x[r], fastv, (g_redo >> r) & 1, ref_quantize(d, q[8 * r]), dmmt::quantize(d, q[8 * r]), u[r], q[8 * r], r);
    }
}

void sweep_scaled(Rng& rng) {
    float q[64], crq[64];
    for (int qi = 1; qi <= 255; qi += qstep) {
        for (int r = 0; r < 8; ++r) {
            q[8 * r] = (float)qi;
            crq[8 * r] = dmmt::c_arai_scale[r] * (1.0f / (float)qi);  // as kernels.hip fills sRQ
        }
        // every half-integer to 256.5, one in seven (another residue per q) up to 2049.5
        for (int n = 0; n <= 2049; ++n) {
            if (n > 256 && (n + qi) % 7) continue;
            float u0[8];
            for (int r = 0; r < 8; ++r) u0[r] = (float)(((double)n + 0.5) * qi / (double)dmmt::c_arai_scale[r]);
            for (int k = -24; k <= 24; ++k) {
                float u[8];
                for (int r = 0; r < 8; ++r) u[r] = step_ulps(u0[r], k);
                scaled_call(u, q, crq, false);
                for (int r = 0; r < 8; ++r) u[r] = -u[r];
                scaled_call(u, q, crq, false);
            }
        }
        for (int i = 0; i < 2048; ++i) {
            float u[8];
            for (int r = 0; r < 8; ++r) u[r] = (float)((2.0 * rng.unit() - 1.0) * 2100.0 / (double)dmmt::c_arai_scale[r]);
            scaled_call(u, q, crq, (i & 1) != 0);  // (nan_possible only forces the per-lane test)
        }
    }
}

// ---- quantize_col8: row r holds the coefficient itself
void f32_call(const float (&v)[8], const float* q, const float* rq) {
    int x[8];
    g_redo = 0;
    dmmt::quantize_col8(v, q, rq, x);
    for (int r = 0; r < 8; ++r) {
        const float t = v[r] * rq[8 * r], a = fabsf(t);
        const int fastv = (int)fminf(copysignf(fminf(truncf(a + 0.5f), 32768.0f), t), 32767.0f);
        cf.lane(x[r], fastv, (g_redo >> r) & 1, ref_quantize(v[r], q[8 * r]), dmmt::quantize(v[r], q[8 * r]), v[r], q[8 * r], r);
    }
}

void sweep_f32(Rng& rng) {
    float q[64], rq[64];
    const float specials[] = {0.0f,     -0.0f,    FLT_TRUE_MIN, -FLT_TRUE_MIN, 1e-40f,   -1e-40f,  FLT_MIN,
                              -FLT_MIN, FLT_MAX,  -FLT_MAX,     INFINITY,      -INFINITY, NAN,      -NAN,
                              0.5f,     -0.5f,    0.49999997f,  -0.49999997f,  8388607.5f, -8388607.5f, 8388608.0f,
                              2147483648.0f, -2147483648.0f, 4294967296.0f};
    const int nspecial = (int)(sizeof specials / sizeof specials[0]);
    for (int qi = 1; qi <= 32; qi += qstep > 1 ? 4 : 1) {
        int qr[8];  // the rows are alike here, so each takes another q: 32 rounds cover 1..255 (255 twice)
        for (int r = 0; r < 8; ++r) {
            qr[r] = qi + 32 * r > 255 ? 255 : qi + 32 * r;
            q[8 * r] = (float)qr[r];
            rq[8 * r] = 1.0f / (float)qr[r];  // as kernels.hip fills sRQ for SB == 4
        }
        for (int pass = 0; pass < 3; ++pass) {
            const long long lo = pass == 0 ? 0 : pass == 1 ? 32765 : 4194304 - 3;
            const long long hi = pass == 0 ? 4096 : pass == 1 ? 32769 : 4194304;
            for (long long n = lo; n <= hi; ++n) {
                float v0[8];
                for (int r = 0; r < 8; ++r) v0[r] = (float)(((double)n + 0.5) * qr[r]);
                for (int k = -24; k <= 24; ++k) {
                    float v[8];
                    for (int r = 0; r < 8; ++r) v[r] = step_ulps(v0[r], k);
                    f32_call(v, q, rq);
                    for (int r = 0; r < 8; ++r) v[r] = -v[r];
                    f32_call(v, q, rq);
                }
            }
        }
        // each special in each row, next to ordinary lanes and next to other specials
        for (int s = 0; s < nspecial; ++s) {
            float v[8];
            for (int r = 0; r < 8; ++r) v[r] = (float)((2.0 * rng.unit() - 1.0) * 300.0);
            v[s & 7] = specials[s];
            f32_call(v, q, rq);
            for (int r = 0; r < 8; ++r) v[r] = specials[(s + r) % nspecial];
            f32_call(v, q, rq);
        }
        for (int i = 0; i < 16384; ++i) {  // any bit pattern
            float v[8];
            for (int r = 0; r < 8; ++r) v[r] = from_bits(rng.next());
            f32_call(v, q, rq);
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && atoi(argv[1]) > 1) qstep = atoi(argv[1]);
    Rng rng{0x9E3779B97F4A7C15ull};
    sweep_scaled(rng);
    sweep_f32(rng);
    const bool a = cs.report(), b = cf.report();
    if (!(a && b)) {
        printf("FAIL: a shortcut quantiser departs from round(d / q)\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
