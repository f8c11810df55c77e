// front_ycc.hip -- k_front_ycc: the front kernel for frames that already are
// YCbCr (dmmt_encode_device_ycc): planar I444 / I422 / I420 and semi-planar
// NV24 / NV16 / NV12 (and their Cr,Cb twins), uint8, JFIF full range.
//
// The reference has no such input (Image<f32> is always RGB); the contract is
// stated in its stages.  A sample s enters the DCT as (float)s - 128, exactly the
// value range color.rs:75-100 produces for the level-shifted Y and for Cb and Cr;
// the chroma planes are taken as they lie, ceil(W / HR) x ceil(H / VR), never
// resampled or averaged; the padding is padder.rs:12-42's black in YCbCr: luma
// -128 (sample 0) up to the MCU multiple, chroma 0 (sample 128).  From there on
// k_front's path: arai.rs:29-104 rows then columns, quantizer.rs:53-62 with the luma
// table for Y and the chroma table for Cb and Cr, block_entangler.rs:69-77's
// emission order, and the same coefficient layout in HBM, so k_hist and every
// kernel after it run unchanged.
//
// Compiled with -ffp-contract=off like kernels.hip (the Makefile's HIPFLAGS).

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

// the planes of frame 0 (three pointers as values: an indexed read of a kernel
// argument would put it into scratch) and their description
struct YccArgs {
    const uint8_t *p0, *p1, *p2;  // Y; Cb or the pairs; Cr (planar only)
    YccDesc d;
};
struct YccMems {
    const uint8_t *p0, *p1, *p2;
    __device__ __forceinline__ PlaneMem plane(int p) const { return PlaneMem{p == 0 ? p0 : (p == 1 ? p1 : p2)}; }
};

// One workgroup (256 threads) per tile = TM horizontally adjacent MCUs of one MCU
// row (256 luma columns, 8 * VR luma rows), a grid-stride loop over the frame's
// tiles (blockIdx.y = frame) with the next tile's bytes prefetched into registers
// while this one computes -- k_front's shape, from the same pieces
// (front_common.hpp): FrontGeom's LDS layout of the row-transformed blocks (sT,
// blk_base), front_stage, and front_column_pass with its emission-order index, so
// the coefficients land where k_front puts them.
//  staging  YccTile / ycc_tile_chunk (ycc_load.hpp): 8 * VR luma tile rows and 8
//     chroma tile rows per chroma plane, each at its own pitch and misalignment;
//     past the rectangle luma stages as 0 and chroma as 0x80
//  A  one thread per (chroma row r, chroma block c, luma block column h): its VR
//     luma rows of 8 samples -- bytes from LDS, s - 128, the row pass -- and a
//     chroma row pass of 8 samples: both components with 4:4:4; with 4:2:x thread
//     h = 0 takes the block's Cb row and h = 1 its Cr row.  (k_front's pair
//     exchanges four averaged samples over DPP because each thread had computed
//     half of both rows; here the samples are bytes in LDS and each thread reads
//     the row it transforms.)  NV: a row of pairs, de-interleaved while unpacking;
//     VU (Cr first) is a template parameter
//  C, D  front_column_pass, k_front's integer-sample path.  Samples are integers in
//     [0, 255], the DCT's inputs integers in [-128, 127]: the bound of
//     dct_quant.hpp's integer-sample argument holds with room to spare (|DC| =
//     |sum| / 8 <= 1024, |AC| <= (1/4) * 64 * 128 = 2048, to within a few ulps), so with q >= 1 `as i16` cannot saturate; no NaN
//     can arise (nan_possible = false), and no sample can exceed a maxval: the
//     kernel raises no status.
// WPE: see front_ycc_wpe below.
// NARROW: the 80-byte block form (coef_format.hpp), as front_body's.
template <int HR, int VR, int FMT, bool NARROW>
__device__ __forceinline__ void front_ycc_body(const YccArgs& ya, size_t frame_stride, const Geom& g,
                                               const float* __restrict__ qtab,  // [2][64] natural, as f32
                                               int16_t* __restrict__ coef, int16_t* __restrict__ coef_lo,
                                               int8_t* __restrict__ coef_hi) {
    constexpr bool NV = FMT != YCC_PLANAR;
    constexpr int VU = FMT == YCC_NV_VU ? 1 : 0;
    using T = YccTile<HR, VR, NV>;
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
    const YccMems ms{ya.p0 + foff, ya.p1 + foff, ya.p2 + foff};  // (NV: p2 = p1)
    const YccDesc& d = ya.d;
    front_fill_qtabs<G, true>(qtab, sQ, sRQ, tid);

    uint4 raw[T::NQ];
    auto load_tile = [&](int tx0, int ty0) {
        const bool interior = ycc_tile_interior<T>(d, tx0, ty0);  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < T::NQ; ++i) {
            const int q = tid + 256 * i;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (q < T::NCHUNK) ycc_tile_chunk<T>(ms, d, tx0, ty0, interior, q, w);
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
        // ---- A: level shift + row pass (arai.rs:97-99)
        {
            const int h = tid % SP, job = tid / SP;
            const int c = job % CB, r = job / CB;  // chroma block, chroma row
            const int lx0 = c * 8 * HR + 8 * h;    // first luma column of the job
#pragma unroll
            for (int dy = 0; dy < VR; ++dy) {
                const int ly = r * VR + dy;
                const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p0, (uint32_t)d.luma_pitch, 1, x0, y0 + ly);
                uint32_t w[2];
                lds_words<2>(sRaw, T::luma_row(ly) + mis + lx0, w);
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) - 128.0f;
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
                    const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p1, (uint32_t)d.chroma_pitch, 2, cx0, cy);
                    uint32_t w[4];
                    lds_words<4>(sRaw, T::chroma_row(0, r) + mis + 16 * c, w);
                    const int sh = 8 * (comp ^ VU);  // the component's byte of a pair
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = (float)(((w[k >> 1] >> sh) >> (16 * (k & 1))) & 0xFFu) - 128.0f;
                } else {
                    const uint8_t* pb = comp ? ms.p2 : ms.p1;
                    const int mis = surf_misalign32((uint32_t)(uintptr_t)pb, (uint32_t)d.chroma_pitch, 1, cx0, cy);
                    uint32_t w[2];
                    lds_words<2>(sRaw, T::chroma_row(comp, r) + mis + 8 * c, w);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) - 128.0f;
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
}

template <int HR, int VR, int FMT, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc(YccArgs ya, size_t frame_stride, Geom g,
                                                       const float* __restrict__ qtab, int16_t* __restrict__ coef) {
    front_ycc_body<HR, VR, FMT, false>(ya, frame_stride, g, qtab, coef, nullptr, nullptr);
}
template <int HR, int VR, int FMT, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_n(YccArgs ya, size_t frame_stride, Geom g,
                                                         const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                         int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    front_ycc_body<HR, VR, FMT, true>(ya, frame_stride, g, qtab, coef, coef_lo, coef_hi);
}

// ============================================================== launcher

// Waves per SIMD the kernel is compiled for (register budget 512 / WPE).  Every
// instantiation fits 4 with room: without a bound the compiler allocates 70 to 72
// VGPRs for 4:2:2, 81 to 82 for 4:4:4 and 93 to 95 for 4:2:0, no scratch
// (-Rpass-analysis=kernel-resource-usage), and 24 KiB (4:2:2) or 35 KiB of LDS:
// at least four resident workgroups per CU, as k_front's u8 4:4:4 and 4:2:2.
constexpr int front_ycc_wpe() { return 4; }

template <int FMT>
static void front_ycc_sub(const YccArgs& ya, size_t frame_stride, int n_frames, const Geom& g, const Work& w,
                          hipStream_t st, int per_cu_cap) {
    front_with_sampling(g, [&](auto hr, auto vr) {
        constexpr int HR = decltype(hr)::value, VR = decltype(vr)::value, WPE = front_ycc_wpe();
        front_launch<k_front_ycc<HR, VR, FMT, WPE>, k_front_ycc_n<HR, VR, FMT, WPE>>(
            g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ya, frame_stride, g, w.qtab, w.coef);
    });
}

static int ycc_chroma_width(int width, int hr) { return (width + hr - 1) / hr; }

size_t ycc_plane_span(int format, int plane, int width, int height, int hr, int vr, size_t luma_pitch,
                      size_t chroma_pitch) {
    return ycc_plane_span_levels(format, plane, width, height, hr, vr, luma_pitch, chroma_pitch, 1);  // uint8
}

hipError_t launch_front_ycc(const YccFrames& yf, size_t frame_stride_bytes, int n_frames, const Geom& g, const Work& w,
                            hipStream_t st, int per_cu_cap) {
    if (yf.format < YCC_PLANAR || yf.format > YCC_NV_VU) return hipErrorInvalidValue;
    YccArgs ya{};
    ya.p0 = (const uint8_t*)yf.plane[0];
    ya.p1 = (const uint8_t*)yf.plane[1];
    ya.p2 = (const uint8_t*)yf.plane[yf.format == YCC_PLANAR ? 2 : 1];
    ya.d.luma_pitch = (long long)yf.luma_pitch;
    ya.d.chroma_pitch = (long long)yf.chroma_pitch;
    ya.d.luma_span = (long long)ycc_plane_span(yf.format, 0, g.width, g.height, g.hr, g.vr, yf.luma_pitch, yf.chroma_pitch);
    ya.d.chroma_span = (long long)ycc_plane_span(yf.format, 1, g.width, g.height, g.hr, g.vr, yf.luma_pitch, yf.chroma_pitch);
    ya.d.width = g.width, ya.d.height = g.height;
    ya.d.cw = ycc_chroma_width(g.width, g.hr), ya.d.ch = (g.height + g.vr - 1) / g.vr;
    if (yf.format == YCC_PLANAR)
        front_ycc_sub<YCC_PLANAR>(ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    else if (yf.format == YCC_NV)
        front_ycc_sub<YCC_NV>(ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    else
        front_ycc_sub<YCC_NV_VU>(ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    return hipGetLastError();
}

}  // namespace dmmt
