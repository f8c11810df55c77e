// front_ycc_levels.hip -- k_front_ycc_lv: the front kernel for YCbCr frames whose
// samples are not 8-bit JFIF full range (dmmt_encode_device_ycc_levels): limited
// ("video") range, and 8 to 16 significant bits in a uint16 -- P010 / P012 / P016
// (the bits at the top, `shift` unused low bits) and I010 / yuv420p10le (the bits at
// the bottom) -- planar or semi-planar as k_front_ycc's (front_ycc.hip).
//
// The contract is dmmt_encode_device_ycc's with one step in front: the code
// v = s >> shift of a sample s becomes the JFIF full-range value in f32, every
// operation rounded once (-ffp-contract=off, the Makefile's HIPFLAGS), and is never
// rounded to 8 bits:
//   luma    min(max(((float)v - offY) * kY, 0), 255) - 128
//   chroma  min(max(((float)v - offC) * kC, -128), 127)
// with the four constants computed on the host (ycc_levels_transfer).  The chroma
// planes are taken as they lie; the padding is black after the transfer -- the
// loader stages the codes offY << shift and offC << shift past the rectangle
// (ycc_load.hpp) -- and from the row pass on everything is k_front_ycc's: the same
// LDS layout, front_column_pass, the same coefficients in HBM.
//
// Compiled with -ffp-contract=off like kernels.hip, the host side too.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dct_quant.hpp"
#include "device_common.hpp"
#include "front_common.hpp"
#include "front_launch.hpp"
#include "jpeg_common.hpp"
#include "kernels.hpp"
#include "ycc_load.hpp"

namespace dmmt {

// B = 8 + e: m = 2^e.  Everything here is exact but the two divisions, which IEEE
// f32 rounds once (2^B - 1 <= 65535 and 219 m, 224 m < 2^24 are exact floats).
YccTransfer ycc_levels_transfer(const YccLevels& lv) {
    const int B = lv.bit_depth;
    const float m = (float)(1 << (B - 8));
    YccTransfer t;
    if (lv.range == YCC_RANGE_LIMITED) {
        t.off_y = 16.0f * m;
        t.k_y = 255.0f / (219.0f * m);
        t.off_c = 128.0f * m;
        t.k_c = 255.0f / (224.0f * m);
    } else {
        t.off_y = 0.0f;
        t.k_y = 255.0f / (float)((1 << B) - 1);
        t.off_c = (float)(1 << (B - 1));
        t.k_c = t.k_y;
    }
    return t;
}

// the planes of frame 0 (three pointers as values: an indexed read of a kernel
// argument would put it into scratch), their description and the sample levels
struct YccLvArgs {
    const uint8_t *p0, *p1, *p2;  // Y; Cb or the pairs; Cr (planar only)
    YccDesc d;
    YccTransfer t;
    uint32_t luma_fill, chroma_fill;  // the pad codes << shift, in every sample of a word
    uint32_t shift;                   // unused low bits of a uint16 sample
    uint32_t max_code;                // 2^B - 1
};
struct YccLvMems {
    const uint8_t *p0, *p1, *p2;
    __device__ __forceinline__ PlaneMem plane(int p) const { return PlaneMem{p == 0 ? p0 : (p == 1 ? p1 : p2)}; }
};

__device__ __forceinline__ float ycc_luma_in(uint32_t v, const YccTransfer& t) {
    return fminf(fmaxf(((float)v - t.off_y) * t.k_y, 0.0f), 255.0f) - 128.0f;
}
__device__ __forceinline__ float ycc_chroma_in(uint32_t v, const YccTransfer& t) {
    return fminf(fmaxf(((float)v - t.off_c) * t.k_c, -128.0f), 127.0f);
}

// k_front_ycc's body (front_ycc.hip: the tile, the thread's jobs of phase A, the
// column pass) with SB bytes per sample and the transfer above.
//  staging  YccTile<.., SB>: a uint16 luma tile row is 512 bytes, 33 chunks; the
//     largest tile (4:2:0 NV and 4:4:4, uint16) is 792 chunks, four per thread
//  A  uint8: the row's words from LDS, funnel-shifted, a byte each
//     (v_cvt_f32_ubyteN); uint16: twice the words -- the misalignment is even -- a
//     half each, shifted right by `shift` (the low bits never count); NV pairs are
//     4-byte positions, one word each after the funnel shift.  Where a code can
//     exceed 2^B - 1 (uint16 with shift < 16 - B: wave-uniform), the largest code of
//     the job's rows is compared with it: status bit 1, raised once per wave after
//     the tile loop.  Only samples of the rectangle and pad codes are unpacked.
//  C, D  front_column_pass, the integer-sample path: the DCT's inputs lie in
//     [-128, 127] like k_front_ycc's, no longer integers -- quantize_col8_scaled's
//     bound needs the range only (k_front feeds it the f32 YCbCr of RGB pixels) --
//     no NaN can arise (nan_possible = false).
template <int HR, int VR, int FMT, int SB, bool NARROW>
__device__ __forceinline__ void front_ycc_lv_body(const YccLvArgs& ya, size_t frame_stride, const Geom& g,
                                                  const float* __restrict__ qtab,  // [2][64] natural, as f32
                                                  int16_t* __restrict__ coef, int* __restrict__ status,
                                                  int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    constexpr bool NV = FMT != YCC_PLANAR;
    constexpr int VU = FMT == YCC_NV_VU ? 1 : 0;
    using T = YccTile<HR, VR, NV, SB>;
    using G = FrontGeom<HR, VR>;  // the tile's blocks (front_common.hpp)
    constexpr int NYB = G::NYB, CB = G::CB;
    constexpr int SP = HR;  // threads per (chroma row, chroma block): one per luma block column
    static_assert(8 * CB * SP == 256, "one phase-A job per thread");

    __shared__ __attribute__((aligned(16))) float sT[G::ST_FLOATS];
    __shared__ __attribute__((aligned(16))) uint8_t sRaw[T::BYTES + 16];  // (+ 16: lds_words reads 3 bytes past a row)
    __shared__ float sQ[128];
    __shared__ float sRQ[128];

    const int tid = threadIdx.x;
    const int frame = blockIdx.y;
    const size_t foff = (size_t)frame * frame_stride;  // the same offset in every plane
    const YccLvMems ms{ya.p0 + foff, ya.p1 + foff, ya.p2 + foff};  // (NV: p2 = p1)
    const YccDesc& d = ya.d;
    const YccTransfer t = ya.t;
    const uint32_t shift = SB == 2 ? ya.shift : 0u;
    const bool check_range = SB == 2 && (0xFFFFu >> shift) > ya.max_code;  // (uniform)
    uint32_t vmax = 0;  // the largest code this thread unpacked
    front_fill_qtabs<G, true>(qtab, sQ, sRQ, tid);

    // sample k of a row's words: uint8 a byte, uint16 a half >> shift
    auto code = [&](const uint32_t* w, int k) -> uint32_t {
        if constexpr (SB == 1) return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        return ((w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) >> shift;
    };

    uint4 raw[T::NQ];
    auto load_tile = [&](int tx0, int ty0) {
        const bool interior = ycc_tile_interior<T>(d, tx0, ty0);  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < T::NQ; ++i) {
            const int q = tid + 256 * i;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (q < T::NCHUNK) ycc_tile_chunk<T>(ms, d, tx0, ty0, interior, q, w, ya.luma_fill, ya.chroma_fill);
            raw[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };
    const int tiles_per_row = (g.mcux + G::TM - 1) / G::TM;
    const int ntiles = tiles_per_row * g.mcuy;
    if ((int)blockIdx.x < ntiles) {
        const int my = blockIdx.x / tiles_per_row;
        load_tile((blockIdx.x - my * tiles_per_row) * 256, my * G::ROWS);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int my = tile / tiles_per_row;
        const int mx0 = (tile - my * tiles_per_row) * G::TM;
        const int x0 = mx0 * 8 * G::HR, y0 = my * G::ROWS;
        front_stage<T::NCHUNK>(sRaw, tid, raw);
        __syncthreads();
        {  // prefetch the next tile's bytes; they land while this tile computes
            const int nt = tile + gridDim.x;
            if (nt < ntiles) {
                const int ny = nt / tiles_per_row;
                load_tile((nt - ny * tiles_per_row) * 256, ny * G::ROWS);
            }
        }
        // ---- A: code -> full-range value, level shift, row pass (arai.rs:97-99)
        {
            const int h = tid % SP, job = tid / SP;
            const int c = job % CB, r = job / CB;  // chroma block, chroma row
            const int lx0 = c * 8 * HR + 8 * h;    // first luma column of the job
#pragma unroll
            for (int dy = 0; dy < VR; ++dy) {
                const int ly = r * VR + dy;
                const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p0, (uint32_t)d.luma_pitch, SB, x0, y0 + ly);
                uint32_t w[2 * SB];
                lds_words<2 * SB>(sRaw, T::luma_row(ly) + mis + SB * lx0, w);
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t s = code(w, k);
                    if constexpr (SB == 2) vmax = max(vmax, s);
                    v[k] = ycc_luma_in(s, t);
                }
                arai8(v);
                float4* o = reinterpret_cast<float4*>(sT + G::blk_base((ly >> 3) * 32 + c * HR + h) + (ly & 7) * 8);
                o[0] = make_float4(v[0], v[1], v[2], v[3]);
                o[1] = make_float4(v[4], v[5], v[6], v[7]);
            }
            const int cx0 = x0 / HR, cy = y0 / VR + r;
#pragma unroll
            for (int pass = 0; pass < (SP == 1 ? 2 : 1); ++pass) {
                const int comp = SP == 1 ? pass : h;  // 0: Cb, 1: Cr
                float v[8];
                if constexpr (NV) {
                    const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p1, (uint32_t)d.chroma_pitch, 2 * SB, cx0, cy);
                    uint32_t w[4 * SB];
                    lds_words<4 * SB>(sRaw, T::chroma_row(0, r) + mis + 16 * SB * c, w);
                    const int first = comp ^ VU;  // the component's place in a pair
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        uint32_t s;
                        if constexpr (SB == 1)
                            s = ((w[k >> 1] >> (8 * first)) >> (16 * (k & 1))) & 0xFFu;
                        else  // a pair is one word
                            s = ((w[k] >> (16 * first)) & 0xFFFFu) >> shift;
                        if constexpr (SB == 2) vmax = max(vmax, s);
                        v[k] = ycc_chroma_in(s, t);
                    }
                } else {
                    const uint8_t* pb = comp ? ms.p2 : ms.p1;
                    const int mis = surf_misalign32((uint32_t)(uintptr_t)pb, (uint32_t)d.chroma_pitch, SB, cx0, cy);
                    uint32_t w[2 * SB];
                    lds_words<2 * SB>(sRaw, T::chroma_row(comp, r) + mis + 8 * SB * c, w);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const uint32_t s = code(w, k);
                        if constexpr (SB == 2) vmax = max(vmax, s);
                        v[k] = ycc_chroma_in(s, t);
                    }
                }
                arai8(v);
                float4* o = reinterpret_cast<float4*>(sT + G::blk_base(NYB + comp * CB + c) + r * 8);
                o[0] = make_float4(v[0], v[1], v[2], v[3]);
                o[1] = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        __syncthreads();
        front_column_pass<G, NARROW, false>(sT, sQ, sRQ, tid, false, g, frame, mx0, my, coef, coef_lo, coef_hi);
    }
    if constexpr (SB == 2) {
        // a code above 2^B - 1 (color.rs:63-65's panic): one vote per wave, its leader stores
        const bool bad = check_range && vmax > ya.max_code;
        if (__ballot(bad)) raise_status(status, bad ? 1 : 0);
    }
}

template <int HR, int VR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_lv(YccLvArgs ya, size_t frame_stride, Geom g,
                                                          const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                          int* __restrict__ status) {
    front_ycc_lv_body<HR, VR, FMT, SB, false>(ya, frame_stride, g, qtab, coef, status, nullptr, nullptr);
}
template <int HR, int VR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_lv_n(YccLvArgs ya, size_t frame_stride, Geom g,
                                                            const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                            int* __restrict__ status, int16_t* __restrict__ coef_lo,
                                                            int8_t* __restrict__ coef_hi) {
    front_ycc_lv_body<HR, VR, FMT, SB, true>(ya, frame_stride, g, qtab, coef, status, coef_lo, coef_hi);
}

// ============================================================== launcher

// Waves per SIMD the kernel is compiled for (register budget 512 / WPE).  uint8
// tiles take k_front_ycc's LDS and registers: 4, four workgroups per CU and more.
// uint16 tiles stage twice the bytes: 27 KiB of LDS with 4:2:2 -- 4 again: 104 to
// 113 registers, so four workgroups per CU although the LDS would hold five -- and
// 41 KiB with 4:4:4 and 4:2:0, where three workgroups fit a CU's 160 KiB whatever the
// registers: 3, a budget of 168.  DESIGN.md section 13 lists what each instantiation
// takes; none spills.
template <int HR, int VR, int SB>
constexpr int front_ycc_lv_wpe() {
    return SB == 2 && !(HR == 2 && VR == 1) ? 3 : 4;
}

template <int FMT, int SB>
static void front_ycc_lv_sub(const YccLvArgs& ya, size_t frame_stride, int n_frames, const Geom& g, const Work& w,
                             hipStream_t st, int per_cu_cap) {
    front_with_sampling(g, [&](auto hr, auto vr) {
        constexpr int HR = decltype(hr)::value, VR = decltype(vr)::value, WPE = front_ycc_lv_wpe<HR, VR, SB>();
        front_launch<k_front_ycc_lv<HR, VR, FMT, SB, WPE>, k_front_ycc_lv_n<HR, VR, FMT, SB, WPE>>(
            g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ya, frame_stride, g, w.qtab, w.coef, w.status);
    });
}
template <int SB>
static void front_ycc_lv_fmt(int format, const YccLvArgs& ya, size_t frame_stride, int n_frames, const Geom& g,
                             const Work& w, hipStream_t st, int per_cu_cap) {
    if (format == YCC_PLANAR)
        front_ycc_lv_sub<YCC_PLANAR, SB>(ya, frame_stride, n_frames, g, w, st, per_cu_cap);
    else if (format == YCC_NV)
        front_ycc_lv_sub<YCC_NV, SB>(ya, frame_stride, n_frames, g, w, st, per_cu_cap);
    else
        front_ycc_lv_sub<YCC_NV_VU, SB>(ya, frame_stride, n_frames, g, w, st, per_cu_cap);
}

bool ycc_levels_valid(const YccLevels& lv) {
    if (lv.range != YCC_RANGE_FULL && lv.range != YCC_RANGE_LIMITED) return false;
    if (lv.sample_bytes == 1) return lv.bit_depth == 8 && lv.shift == 0;
    if (lv.sample_bytes != 2) return false;
    return lv.bit_depth >= 8 && lv.bit_depth <= 16 && lv.shift >= 0 && lv.shift <= 16 - lv.bit_depth;
}

size_t ycc_plane_span_levels(int format, int plane, int width, int height, int hr, int vr, size_t luma_pitch,
                             size_t chroma_pitch, int sample_bytes) {
    if (format < YCC_PLANAR || format > YCC_NV_VU || width <= 0 || height <= 0) return 0;
    if (sample_bytes != 1 && sample_bytes != 2) return 0;
    const size_t sb = (size_t)sample_bytes;
    if (plane == 0) return (size_t)(height - 1) * luma_pitch + (size_t)width * sb;
    if (plane != 1 && !(plane == 2 && format == YCC_PLANAR)) return 0;
    const size_t cw = (size_t)((width + hr - 1) / hr), ch = (size_t)((height + vr - 1) / vr);
    return (ch - 1) * chroma_pitch + cw * (format == YCC_PLANAR ? 1 : 2) * sb;
}

hipError_t launch_front_ycc_levels(const YccFrames& yf, const YccLevels& lv, size_t frame_stride_bytes, int n_frames,
                                   const Geom& g, const Work& w, hipStream_t st, int per_cu_cap) {
    if (yf.format < YCC_PLANAR || yf.format > YCC_NV_VU || !ycc_levels_valid(lv)) return hipErrorInvalidValue;
    const int sb = lv.sample_bytes;
    YccLvArgs ya{};
    ya.p0 = (const uint8_t*)yf.plane[0];
    ya.p1 = (const uint8_t*)yf.plane[1];
    ya.p2 = (const uint8_t*)yf.plane[yf.format == YCC_PLANAR ? 2 : 1];
    ya.d.luma_pitch = (long long)yf.luma_pitch;
    ya.d.chroma_pitch = (long long)yf.chroma_pitch;
    ya.d.luma_span = (long long)ycc_plane_span_levels(yf.format, 0, g.width, g.height, g.hr, g.vr, yf.luma_pitch,
                                                      yf.chroma_pitch, sb);
    ya.d.chroma_span = (long long)ycc_plane_span_levels(yf.format, 1, g.width, g.height, g.hr, g.vr, yf.luma_pitch,
                                                        yf.chroma_pitch, sb);
    ya.d.width = g.width, ya.d.height = g.height;
    ya.d.cw = (g.width + g.hr - 1) / g.hr, ya.d.ch = (g.height + g.vr - 1) / g.vr;
    ya.t = ycc_levels_transfer(lv);
    // the pad codes: offY and offC are integers below 2^B, so << shift stays inside 16 (8) bits
    const uint32_t py = (uint32_t)ya.t.off_y << lv.shift, pc = (uint32_t)ya.t.off_c << lv.shift;
    ya.luma_fill = sb == 1 ? py * 0x01010101u : py * 0x00010001u;
    ya.chroma_fill = sb == 1 ? pc * 0x01010101u : pc * 0x00010001u;
    ya.shift = (uint32_t)lv.shift;
    ya.max_code = (1u << lv.bit_depth) - 1u;
    if (sb == 1)
        front_ycc_lv_fmt<1>(yf.format, ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    else
        front_ycc_lv_fmt<2>(yf.format, ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    return hipGetLastError();
}

}  // namespace dmmt
