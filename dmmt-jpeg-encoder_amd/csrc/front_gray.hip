// front_gray.hip -- k_front_gray: the front kernel for one-channel frames
// (dmmt_encode_device_gray): a pitched plane of uint8, uint16 or float samples ->
// the luma blocks of a single-component file.
//
// The reference has no gray input (Image<f32> is always RGB); the contract is
// stated in its stages.  DMMT_GRAY_AS_RGB: the sample v is the pixel (v, v, v) --
// normalised by color.rs:45-53 (float samples are Image<f32> dots as they are),
// luma by color.rs:75-100, (((n * 0.299 + n * 0.587) + n * 0.114) - 128/255) * 255
// in that order, every operation rounded to f32 (the three weights do not sum to
// 1 in f32, so this is not n * 255 - 128).  DMMT_GRAY_Y_FULL_RANGE (uint8): the
// sample s enters the DCT as (float)s - 128, dmmt_encode_device_ycc's luma.  Both
// pad with sample 0 (padder.rs:12-42's black) up to multiples of 8.  Integer
// samples go through a table of the luma per sample value, filled on the host
// (gray_fill_lut), so the two transfers differ only in the table.  From there on
// k_front's path: arai.rs:29-104 rows then columns, quantizer.rs:53-62 with the
// luma table, and k_front's coefficient layout in HBM at the block's raster index
// (an MCU is one block), so k_hist and every kernel after it run unchanged.
//
// Compiled with -ffp-contract=off like kernels.hip (the Makefile's HIPFLAGS), the
// host side too: gray_fill_lut rounds as the device would.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dct_quant.hpp"
#include "device_common.hpp"
#include "front_common.hpp"
#include "front_launch.hpp"
#include "gray_load.hpp"
#include "jpeg_common.hpp"
#include "kernels.hpp"

namespace dmmt {

// color.rs:75-100's Y of the pixel (n, n, n), level-shifted and scaled as rgb_to_ycbcr
// (kernels.hip) has it
__host__ __device__ __forceinline__ float gray_luma(float n) {
    const float k128 = 128.0f / 255.0f;
    return (((n * 0.299f + n * 0.587f) + n * 0.114f) - k128) * 255.0f;
}

// (maxval > 0 for AS_RGB: dmmt_encode_device_gray refuses 0)
void gray_fill_lut(float* lut, size_t n, int maxval, int transfer) {
    for (size_t v = 0; v < n; ++v)
        lut[v] = transfer == GRAY_Y_FULL_RANGE ? (float)v - 128.0f : gray_luma((float)v / (float)maxval);
}

// the plane of frame 0 and its description
struct GrayArgs {
    const uint8_t* p;
    GrayDesc d;
};

// One workgroup (256 threads) per tile = 32 horizontally adjacent blocks of one
// block row (256 columns, 8 rows), a grid-stride loop over the frame's tiles
// (blockIdx.y = frame) with the next tile's bytes prefetched into registers while
// this one computes -- k_front's shape, from the same pieces (front_common.hpp):
// the one-component FrontGeom with k_front's LDS layout of the row-transformed
// blocks (sT, front_store_row), front_stage and front_column_pass.
//  staging  GrayTile / gray_tile_chunk (gray_load.hpp): 8 tile rows, each at its own
//     misalignment; past the rectangle everything stages as 0
//  A  one thread per (row r, block c): its 8 samples from LDS -- the table's luma
//     per integer sample (u8: the table in LDS), gray_luma of a float dot -- and the
//     row pass.  Integer samples: the largest one against maxval where a sample can
//     exceed it (color.rs:63-65, status bit 1)
//  C, D  front_column_pass (integer samples quantize_col8_scaled, whose bound holds
//     as for k_front: the luma of a sample in range lies in [-128, 128], and no NaN
//     can arise -- the host refuses maxval 0 for integer samples -- so nan_possible =
//     false; float dots are unbounded and may be NaN: arai8 and quantize_col8, wide
//     blocks only), the blocks at el = their raster index.
// NARROW: the 80-byte block form (coef_format.hpp), as front_body's.
template <typename Sample, bool NARROW>
__device__ __forceinline__ void front_gray_body(const GrayArgs& ga, size_t frame_stride, const Geom& g,
                                                const float* __restrict__ lut,   // luma per sample value (integer samples)
                                                const float* __restrict__ qtab,  // [2][64] natural, as f32
                                                int16_t* __restrict__ coef, int* __restrict__ status,
                                                int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    constexpr int SB = (int)sizeof(Sample);
    static_assert(!NARROW || SB != 4, "Image<f32> dots are unbounded: wide blocks");
    using T = GrayTile<SB>;
    using G = FrontGeom<1, 1, 1>;  // 32 blocks per tile, an MCU is one block (front_common.hpp)

    __shared__ __attribute__((aligned(16))) float sT[G::ST_FLOATS];
    __shared__ __attribute__((aligned(16))) uint8_t sRaw[T::BYTES + 16];  // (+ 16: lds_words reads 3 bytes past a row)
    __shared__ float sLut[SB == 1 ? 256 : 1];
    __shared__ float sQ[64];
    __shared__ float sRQ[64];

    const int tid = threadIdx.x;
    const int frame = blockIdx.y;
    const PlaneMem m{ga.p + (size_t)frame * frame_stride};
    const GrayDesc& d = ga.d;
    front_fill_qtabs<G, SB != 4>(qtab, sQ, sRQ, tid);
    if constexpr (SB == 1) sLut[tid] = lut[tid];
    int bad = 0;
    const bool check_range = SB != 4 && g.maxval < (SB == 1 ? 255 : 65535);

    uint4 raw[T::NQ];
    auto load_tile = [&](int tx0, int ty0) {
        const bool interior = gray_tile_interior<T>(d, tx0, ty0);  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < T::NQ; ++i) {
            const int q = tid + 256 * i;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (q < T::NCHUNK) gray_tile_chunk<T>(m, d, tx0, ty0, interior, q, w);
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
        // ---- A: sample -> luma (color.rs:45-53, 75-100), row pass (arai.rs:97-99)
        {
            const int c = tid & 31, r = tid >> 5;  // block, row
            const int mis = surf_misalign32(m.base_lo(), (uint32_t)d.pitch, SB, x0, y0 + r);
            const int off = T::row(r) + mis + 8 * SB * c;
            float v[8];
            if constexpr (SB == 4) {  // Image<f32> dots as given (0.0 past the edges); mis is a multiple of 4
                const float* src = reinterpret_cast<const float*>(sRaw + off);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = gray_luma(src[k]);
            } else {
                uint32_t w[2 * SB];
                lds_words<2 * SB>(sRaw, off, w);
                uint32_t smax = 0;  // largest sample of the row (a sample above maxval panics in color.rs:63-65)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t s = SB == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 0xFFu : (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                    smax = max(smax, s);
                    v[k] = SB == 1 ? sLut[s] : lut[s];
                }
                if (check_range) bad |= (int)(smax > (uint32_t)g.maxval);  // status bit 1
            }
            arai8(v);
            front_store_row<G>(sT, c, r, v);
        }
        __syncthreads();
        front_column_pass<G, NARROW, SB == 4>(sT, sQ, sRQ, tid, false, g, frame, mx0, my, coef, coef_lo, coef_hi);
    }
    if (bad) raise_status(status, bad);  // 1: sample above maxval
}

template <typename Sample, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_gray(GrayArgs ga, size_t frame_stride, Geom g,
                                                        const float* __restrict__ lut, const float* __restrict__ qtab,
                                                        int16_t* __restrict__ coef, int* __restrict__ status) {
    front_gray_body<Sample, false>(ga, frame_stride, g, lut, qtab, coef, status, nullptr, nullptr);
}
template <typename Sample, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_gray_n(GrayArgs ga, size_t frame_stride, Geom g,
                                                          const float* __restrict__ lut, const float* __restrict__ qtab,
                                                          int16_t* __restrict__ coef, int* __restrict__ status,
                                                          int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    front_gray_body<Sample, true>(ga, frame_stride, g, lut, qtab, coef, status, coef_lo, coef_hi);
}

// ============================================================== launcher

// Waves per SIMD the kernel is compiled for (register budget 512 / WPE): uint8
// samples fit 64 registers, eight resident workgroups per CU; uint16 (four raw
// words per row, the table in HBM) and float samples (quantize_col8) spill there
// and get 128.  DESIGN.md section 12 lists what each instantiation takes.
template <typename S>
constexpr int front_gray_wpe() {
    return sizeof(S) == 1 ? 8 : 4;
}

template <typename S>
static void front_gray_impl(const GrayArgs& ga, size_t frame_stride, int n_frames, const Geom& g, const Work& w,
                            const float* lut, hipStream_t st, int per_cu_cap) {
    constexpr int WPE = front_gray_wpe<S>();
    if constexpr (sizeof(S) == 4)  // (float samples have no narrow twin)
        front_launch<k_front_gray<S, WPE>, nullptr>(g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ga, frame_stride,
                                                    g, lut, w.qtab, w.coef, w.status);
    else
        front_launch<k_front_gray<S, WPE>, k_front_gray_n<S, WPE>>(g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ga,
                                                                   frame_stride, g, lut, w.qtab, w.coef, w.status);
}

size_t gray_plane_span(int width, int height, int sample_bytes, size_t row_pitch) {
    if (width <= 0 || height <= 0 || (sample_bytes != 1 && sample_bytes != 2 && sample_bytes != 4)) return 0;
    return (size_t)(height - 1) * row_pitch + (size_t)width * sample_bytes;
}

hipError_t launch_front_gray(const GrayPlane& gp, size_t frame_stride_bytes, int sample_bytes, int n_frames,
                             const Geom& g, const Work& w, hipStream_t st, int per_cu_cap) {
    if (g.ncomp != 1 || (sample_bytes != 4 && !gp.lut) || (sample_bytes == 4 && w.coef_lo)) return hipErrorInvalidValue;
    GrayArgs ga{};
    ga.p = (const uint8_t*)gp.plane;
    ga.d.pitch = (long long)gp.row_pitch;
    ga.d.span = (long long)gray_plane_span(g.width, g.height, sample_bytes, gp.row_pitch);
    ga.d.width = g.width, ga.d.height = g.height;
    if (sample_bytes == 1)
        front_gray_impl<uint8_t>(ga, frame_stride_bytes, n_frames, g, w, gp.lut, st, per_cu_cap);
    else if (sample_bytes == 2)
        front_gray_impl<uint16_t>(ga, frame_stride_bytes, n_frames, g, w, gp.lut, st, per_cu_cap);
    else if (sample_bytes == 4)
        front_gray_impl<float>(ga, frame_stride_bytes, n_frames, g, w, gp.lut, st, per_cu_cap);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace dmmt
