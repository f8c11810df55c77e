// front_ycc_common.hpp -- what the YCbCr front kernels' translation units share
// (front_ycc.hip: the planes at the file's sampling; front_ycc_sub.hip: planes at a
// finer sampling, box-averaged): the kernels' first argument per kind of input, the
// transfer from a code to the DCT's input, and the host code that fills the argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "front_common.hpp"
#include "jpeg_common.hpp"
#include "kernels.hpp"
#include "ycc_load.hpp"

namespace dmmt {

enum { YCC_IN_PLAIN = 0, YCC_IN_LEVELS = 1, YCC_IN_MATRIX = 2 };

// The kernel's first argument, one struct per kind: the planes of frame 0 (three
// pointers as values: an indexed read of a kernel argument would put it into
// scratch) and their description; the sample levels; the matrix.
struct YccArgs {
    static constexpr int IN = YCC_IN_PLAIN;
    const uint8_t *p0, *p1, *p2;  // Y; Cb or the pairs; Cr (planar only)
    YccDesc d;
};
struct YccCodes {
    uint32_t luma_fill, chroma_fill;  // the pad codes << shift, in every sample of a word
    uint32_t shift;                   // unused low bits of a uint16 sample
    uint32_t max_code;                // 2^B - 1
};
struct YccLvArgs : YccArgs {
    static constexpr int IN = YCC_IN_LEVELS;
    YccTransfer t;
    YccCodes c;
};
struct YccMxArgs : YccArgs {
    static constexpr int IN = YCC_IN_MATRIX;
    YccTransfer t;
    YccMatrix m;
    YccCodes c;
};
struct YccMems {
    const uint8_t *p0, *p1, *p2;
    __device__ __forceinline__ PlaneMem plane(int p) const { return PlaneMem{p == 0 ? p0 : (p == 1 ? p1 : p2)}; }
};

// a code -> the level-shifted full-range value (plain: the code is the sample)
template <int IN>
__device__ __forceinline__ float ycc_luma_in(uint32_t v, const YccTransfer& t) {
    if constexpr (IN == YCC_IN_PLAIN) return (float)v - 128.0f;
    return fminf(fmaxf(((float)v - t.off_y) * t.k_y, 0.0f), 255.0f) - 128.0f;
}
template <int IN>
__device__ __forceinline__ float ycc_chroma_in(uint32_t v, const YccTransfer& t) {
    if constexpr (IN == YCC_IN_PLAIN) return (float)v - 128.0f;
    return fminf(fmaxf(((float)v - t.off_c) * t.k_c, -128.0f), 127.0f);
}
__device__ __forceinline__ float ycc_clamp(float v) { return fminf(fmaxf(v, -128.0f), 127.0f); }

// the kernel's first argument for frames yf whose chroma planes are sampled at
// (hr, vr) (lv: null for YccArgs; else valid)
template <class Args>
static Args ycc_args(const YccFrames& yf, const YccLevels* lv, const Geom& g, int hr, int vr) {
    const int sb = lv ? lv->sample_bytes : 1;
    Args ya{};
    ya.p0 = (const uint8_t*)yf.plane[0];
    ya.p1 = (const uint8_t*)yf.plane[1];
    ya.p2 = (const uint8_t*)yf.plane[yf.format == YCC_PLANAR ? 2 : 1];
    ya.d.luma_pitch = (long long)yf.luma_pitch;
    ya.d.chroma_pitch = (long long)yf.chroma_pitch;
    ya.d.luma_span = (long long)ycc_plane_span_levels(yf.format, 0, g.width, g.height, hr, vr, yf.luma_pitch,
                                                      yf.chroma_pitch, sb);
    ya.d.chroma_span = (long long)ycc_plane_span_levels(yf.format, 1, g.width, g.height, hr, vr, yf.luma_pitch,
                                                        yf.chroma_pitch, sb);
    ya.d.width = g.width, ya.d.height = g.height;
    ya.d.cw = (g.width + hr - 1) / hr, ya.d.ch = (g.height + vr - 1) / vr;
    if constexpr (Args::IN != YCC_IN_PLAIN) {
        ya.t = ycc_levels_transfer(*lv);
        // the pad codes: offY and offC are integers below 2^B, so << shift stays inside 16 (8) bits
        const uint32_t py = (uint32_t)ya.t.off_y << lv->shift, pc = (uint32_t)ya.t.off_c << lv->shift;
        ya.c.luma_fill = sb == 1 ? py * 0x01010101u : py * 0x00010001u;
        ya.c.chroma_fill = sb == 1 ? pc * 0x01010101u : pc * 0x00010001u;
        ya.c.shift = (uint32_t)lv->shift;
        ya.c.max_code = (1u << lv->bit_depth) - 1u;
    }
    return ya;
}

}  // namespace dmmt
