// kernels.hip -- gfx950 kernels of the baseline-JPEG encode path.
//
// Pipeline per launch batch (all frames share one geometry; frame = blockIdx.y
// or blockIdx.x as noted).  Reference stages in brackets (paths relative to the
// reference repository):
//
//  k_front      pixels -> quantised blocks in MCU emission order.  [color.rs:45-100,
//               padder.rs:12-42, subsampling.rs:102-310, arai.rs:29-104,
//               quantizer.rs:53-62, block_entangler.rs:5-77,
//               block_fold_iterator.rs:53-148]  (front_ycc.hip: k_front_ycc, the
//               same stage for frames that already are YCbCr)
//  k_hist       per block: DC prediction in emission order, AC run/size symbols;
//               DC and AC histograms [categorize.rs:132-169, symbol_counting.rs:55-74]
//  k_tables     one workgroup per (table, frame): package-merge code lengths, canonical
//               codes, JFIF header bytes [symbol_counting.rs:85-94,
//               length_limited.rs:37-134, huffman/encoder.rs:45-157,
//               encoder.rs:125-262]
//  k_emit, k_offsets, k_stuffwrite (entropy.hip): Huffman bit emission per
//               chunk, chunk offsets, byte stuffing, EOI [encoder.rs:264-404,
//               binary_stream.rs:38-96, segment_marker_injector.rs:13-30]
//
// Floating point: this file is compiled with -ffp-contract=off and without
// fast-math, f32 '/' is the correctly rounded IEEE division (hipcc default),
// roundf rounds half away from zero -- the reference's Rust f32 semantics.  The
// one place that fuses on purpose is rgb_to_ycbcr<true> (integer samples): two
// fma per pixel whose product, a normalised sample times 0.5, is exact.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "dct_quant.hpp"
#include "device_common.hpp"
#include "front_common.hpp"
#include "front_launch.hpp"
#include "jpeg_common.hpp"
#include "kernels.hpp"
#include "surface_load.hpp"
#include "wave_merge.hpp"

namespace dmmt {

#ifdef DMMT_PHASE_TRACE
static __device__ unsigned long long g_trace[64];
#endif

__constant__ uint8_t c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                     12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                     58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// zigzag position of natural index n
__constant__ uint8_t c_inv_zigzag[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                         3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                         10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                         21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// color.rs:75-100.  HALF_FMA (integer samples): the two products by 0.5 are exact
// -- a normalised sample is 0 or at least 1/65535, far from the subnormals -- so
// fma(b, 0.5, t) rounds once, exactly as t + b * 0.5 does, and each saves a
// v_mul: the only two v_fma per pixel this file means to have.  An Image<f32>
// dot may be small enough for its half to be subnormal and inexact: that path
// keeps the separate multiply.
template <bool HALF_FMA>
__device__ __forceinline__ void rgb_to_ycbcr(float r, float g, float b, float& y, float& cb, float& cr) {
    const float k128 = 128.0f / 255.0f;
    y = (((r * 0.299f + g * 0.587f) + b * 0.114f) - k128) * 255.0f;
    if constexpr (HALF_FMA) {
        cb = __builtin_fmaf(b, 0.5f, r * -0.1687f + g * -0.3312f) * 255.0f;
        cr = (__builtin_fmaf(r, 0.5f, g * -0.4186f) + b * -0.0813f) * 255.0f;
    } else {
        cb = ((r * -0.1687f + g * -0.3312f) + b * 0.5f) * 255.0f;
        cr = ((r * 0.5f + g * -0.4186f) + b * -0.0813f) * 255.0f;
    }
}

// ============================================================== k_front

// Raw pixel staging: a tile row is 256 pixels = RB bytes, fetched as the RC
// aligned 16-byte chunks that cover it at any alignment (byte loads only for a
// chunk that crosses the frame's first or last byte).  Chunk q of a tile is
// chunk q % RC of tile row q / RC; thread t owns chunks t, t+256, ...  In LDS a
// tile row starts at row * RS, its first pixel `misalign` bytes further.  Every
// byte of a tile row past the image's right edge, and every row past its bottom,
// stages as 0: sample 0 normalises to 0.0, the reference's black padding
// (padder.rs:12-42), so phase A needs no bounds checks.
template <typename Sample, int ROWS>
struct RawTile {
    static constexpr int RB = 256 * 3 * (int)sizeof(Sample);
    static constexpr int RC = RB / 16 + 1;
    static constexpr int RS = RC * 16;
    static constexpr int NCHUNK = ROWS * RC;
    static constexpr int NQ = (NCHUNK + 255) / 256;
    static constexpr int BYTES = NCHUNK * 16;

    __device__ static __forceinline__ long long row_start(const Geom& g, int x0, int py) {
        return ((long long)py * g.width + x0) * 3 * (long long)sizeof(Sample);
    }
    __device__ static __forceinline__ int misalign(const uint8_t* fbase, long long start) {
        return (int)(((uintptr_t)fbase + (uintptr_t)start) & 15u);
    }

    // misalign() from 32-bit arithmetic: only the address's low 4 bits matter
    __device__ static __forceinline__ int misalign32(const uint8_t* fbase, const Geom& g, int x0, int py) {
        return (int)(((uint32_t)(uintptr_t)fbase + (uint32_t)(py * g.width + x0) * (uint32_t)(3 * sizeof(Sample))) & 15u);
    }

    __device__ static __forceinline__ void load(const uint8_t* __restrict__ fbase, long long fbytes, const Geom& g,
                                                int x0, int y0, int tid, uint4 (&v)[NQ]) {
        // Interior tile (wave-uniform): every row inside the image, no pixel past its
        // right edge, every chunk inside the frame's bytes -- plain aligned loads, no
        // masking.  The bytes a chunk holds beyond the tile row are never read.
        const long long last = row_start(g, x0, y0 + ROWS - 1);
        if (x0 + 256 <= g.width && y0 + ROWS <= g.height && row_start(g, x0, y0) >= 16 && last + RB + 16 <= fbytes) {
            const uint8_t* tb = fbase + row_start(g, x0, y0);
            const uint32_t rowpitch = (uint32_t)g.width * (uint32_t)(3 * sizeof(Sample));
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const int q = tid + 256 * i;
                const int row = q / RC, j = q - (q / RC) * RC;
                const uint8_t* r = tb + (size_t)((uint32_t)row * rowpitch);  // pointer arithmetic: stays global
                const uint8_t* a = r - ((uint32_t)(uintptr_t)r & 15u) + 16u * (uint32_t)j;
                v[i] = q < NCHUNK ? ld16_nt(a) : make_uint4(0u, 0u, 0u, 0u);
            }
            return;
        }
        const long long rowbytes = (long long)min(256, g.width - x0) * 3 * (long long)sizeof(Sample);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            const int q = tid + 256 * i;
            const int row = q / RC, j = q - (q / RC) * RC;
            const int py = y0 + row;
            if (q >= NCHUNK || py >= g.height) continue;
            const long long start = row_start(g, x0, py);
            const long long c = start - misalign(fbase, start) + 16LL * j;  // frame-relative
            if (c >= start + rowbytes) continue;
            if (c >= 0 && c + 16 <= fbytes) {
                v[i] = ld16_nt(fbase + c);
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                for (int k = 0; k < 16; ++k)
                    if (c + k >= 0 && c + k < fbytes) w[k >> 2] |= (uint32_t)fbase[c + k] << (8 * (k & 3));
                v[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            const long long keep = start + rowbytes - c;  // bytes of the chunk inside the tile row
            if (keep < 16) {  // zero the rest: past the image's right edge the tile reads black
                uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long n = keep - 4 * k;
                    w[k] &= n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u);
                }
                v[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    }
};

// Raw pixel staging of a surface (dmmt_device_surfaces): rows row_pitch bytes
// apart, 3 or 4 interleaved samples per pixel or three planes of one sample each.
// As RawTile, with the chunk arithmetic of surface_load.hpp: a pixel row stages as
// NPL tile rows (one per plane, tile row ly * NPL + p), each with the misalignment
// of its own first byte; nothing outside [plane, plane + span) is read, and every
// byte past the rectangle's right edge or bottom stages as 0.
enum { LAY_TIGHT = 0, LAY_RGB = 1, LAY_RGBX = 2, LAY_PLANAR = 3 };
template <int LAY>
struct SurfLayout {
    static constexpr int NPL = LAY == LAY_PLANAR ? 3 : 1;                        // planes
    static constexpr int SPP = LAY == LAY_RGBX ? 4 : (LAY == LAY_PLANAR ? 1 : 3);  // samples per pixel of a plane
};
template <typename Sample, int ROWS, int LAY>
struct SurfTile {
    static constexpr int NPL = SurfLayout<LAY>::NPL;
    static constexpr int BPP = SurfLayout<LAY>::SPP * (int)sizeof(Sample);  // bytes per pixel of a plane
    static constexpr int RB = 256 * BPP;
    static constexpr int RC = RB / 16 + 1;
    static constexpr int RS = RC * 16;
    static constexpr int NCHUNK = ROWS * NPL * RC;
    static constexpr int NQ = (NCHUNK + 255) / 256;
    static constexpr int BYTES = NCHUNK * 16;

    // plane p's first byte of the frame (the three pointers as values: an indexed
    // read of the kernel argument would put it into scratch)
    struct Planes {
        const uint8_t *p0, *p1, *p2;
    };
    __device__ static __forceinline__ Planes planes(const SurfArgs& sa, size_t foff) {
        return Planes{sa.plane[0] + foff, sa.plane[NPL == 1 ? 0 : 1] + foff, sa.plane[NPL == 1 ? 0 : 2] + foff};
    }
    __device__ static __forceinline__ const uint8_t* plane(const Planes& pl, int p) {
        return NPL == 1 || p == 0 ? pl.p0 : (p == 1 ? pl.p1 : pl.p2);
    }
    __device__ static __forceinline__ int misalign32(const uint8_t* pbase, const SurfArgs& sa, int x0, int py) {
        return surf_misalign32((uint32_t)(uintptr_t)pbase, (uint32_t)sa.pitch, BPP, x0, py);
    }

    __device__ static __forceinline__ void load(const SurfArgs& sa, size_t foff, const Geom& g, int x0, int y0, int tid,
                                                uint4 (&v)[NQ]) {
        // interior tile (wave-uniform), as RawTile::load: the same offsets in every plane
        const Planes pl = planes(sa, foff);
        const long long first = surf_row_start(sa.pitch, BPP, x0, y0);
        if (x0 + 256 <= g.width && y0 + ROWS <= g.height &&
            surf_interior(first, surf_row_start(sa.pitch, BPP, x0, y0 + ROWS - 1), RB, sa.span)) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const int q = tid + 256 * i;
                const int tr = q / RC, j = q - (q / RC) * RC;
                const int row = tr / NPL, p = tr - (tr / NPL) * NPL;
                const uint8_t* pb = plane(pl, p);
                const long long c = surf_interior_chunk((uint32_t)(uintptr_t)pb, first + (long long)row * sa.pitch, j);
                v[i] = q < NCHUNK ? ld16_nt(pb + c) : make_uint4(0u, 0u, 0u, 0u);
            }
            return;
        }
        const long long rowbytes = surf_row_bytes(g.width, BPP, x0);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            const int q = tid + 256 * i;
            const int tr = q / RC, j = q - (q / RC) * RC;
            const int row = tr / NPL, p = tr - (tr / NPL) * NPL;
            const int py = y0 + row;
            if (q >= NCHUNK || py >= g.height) continue;
            const PlaneMem m{plane(pl, p)};
            uint32_t w[4];
            surf_load_chunk(m, surf_row_start(sa.pitch, BPP, x0, py), misalign32(m.base, sa, x0, py), rowbytes, sa.span,
                            j, w);
            v[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
};

// One workgroup (256 threads) per tile = TM horizontally adjacent MCUs of one
// MCU row (256 padded pixel columns, 8*VR rows), looping over the frame's tiles
// (grid = resident workgroups; blockIdx.y = frame) with the next tile's pixels
// prefetched into registers while the current one computes.  The tile's block
// geometry, the staging copy and phases C and D are front_common.hpp's (FrontGeom,
// front_stage, front_column_pass), shared with k_front_ycc and k_front_gray.
//  A  colour + subsampling + row DCT, fused: one thread per (chroma row, luma
//     block column) converts its 8 x VR pixels (raw bytes from LDS), box-averages
//     the chroma in the reference's sum order and runs the row pass of its VR
//     luma rows and of the chroma rows in registers -> LDS (front_store_row);
//     with 4:2:x the two threads of a chroma block swap four chroma samples
//     over DPP and take one chroma row pass each
//  C  column DCT + quantise (quantize_col8_scaled): one lane per (block, column),
//     the column's 8 coefficients kept in registers for
//  D  their store: 16 B per lane, 8 lanes per block (blocks are column-major in
//     HBM, coef_pos).  The symbols are counted by k_hist, one thread per block:
//     a walk over the block costs a third of the instructions the same counts
//     cost here, spread over the block's 8 lanes.
// Two barriers per tile: the next tile's staging barrier also keeps its phase A
// from overwriting sT before every wave has read its columns.
// LAY: the input layout.  LAY_TIGHT (k_front) reads rgb + frame * frame_stride
// samples through RawTile; the others (k_front_surf) read the surface sa, its
// frames frame_stride bytes apart, through SurfTile, and phase A picks its three
// samples at SPP-sample pixels of NPL planes (sa.bgr, wave-uniform: samples 0 and
// 2 of an interleaved pixel change roles).
// NARROW: the blocks go out in the 80-byte form (coef_format.hpp: coef_lo, coef_hi,
// coef the escape store); integer samples only.
template <int HR, int VR, typename Sample, int LAY, bool NARROW = false>
__device__ __forceinline__ void front_body(const Sample* __restrict__ rgb, size_t frame_stride, const SurfArgs& sa,
                                           Geom g, const float* __restrict__ norm_lut,
                                           const float* __restrict__ qtab,  // [2][64] natural, as f32
                                           int16_t* __restrict__ coef, int* __restrict__ status,
                                           int16_t* __restrict__ coef_lo = nullptr,
                                           int8_t* __restrict__ coef_hi = nullptr) {
    // the tile's blocks (front_layout.hpp); u8 4:4:4 takes sT without padding
    using G = FrontGeom<HR, VR, 3, sizeof(Sample) == 1 && HR * VR == 1>;
    constexpr int ROWS = G::ROWS, NYB = G::NYB, CB = G::CB;
    constexpr int SP = HR;           // threads per (chroma row, chroma block): one per luma block column
    constexpr int NJ = 8 * CB * SP;  // fused jobs (chroma row, chroma block, luma block column): 256
    constexpr int NCS = 8 / SP;      // chroma samples of a job
    constexpr int SB = (int)sizeof(Sample);
    constexpr int NPL = SurfLayout<LAY>::NPL;
    constexpr int SPP = SurfLayout<LAY>::SPP;
    constexpr int PXB = 8 * SPP * SB;  // raw bytes of one job row (8 pixels) in a plane
    constexpr int PXW = PXB / 4;
    using Raw = std::conditional_t<LAY == LAY_TIGHT, RawTile<Sample, ROWS>, SurfTile<Sample, ROWS, LAY>>;

    // row-transformed blocks (A -> C)
    __shared__ __attribute__((aligned(16))) float sT[G::ST_FLOATS];
    __shared__ __attribute__((aligned(16))) uint8_t sRaw[Raw::BYTES];
    __shared__ float sLut[256];
    // u8 4:4:4 keeps no copy of the quantiser tables: its LDS then is at most 32,768
    // bytes, five workgroups per CU, without which the register budget does not bind
    // (front_wpe below); only the quantiser's rare exact path reads them, from qtab
    constexpr bool Q_GLOBAL = SB == 1 && HR * VR == 1;
    __shared__ float sQ[Q_GLOBAL ? 1 : 128];
    __shared__ float sRQ[128];

    DMMT_TRACE_START;
    const int tid = threadIdx.x;
    const int frame = blockIdx.y;
    // tight frames: frame_stride in samples from rgb; surfaces: in bytes, the same offset in every plane
    const uint8_t* fbase = nullptr;
    long long fbytes = 0;
    size_t foff = 0;
    if constexpr (LAY == LAY_TIGHT) {
        fbase = reinterpret_cast<const uint8_t*>(rgb + (size_t)frame * frame_stride);
        fbytes = (long long)g.width * g.height * 3 * SB;
    } else {
        foff = (size_t)frame * frame_stride;
    }
    front_fill_qtabs<G, SB != 4, !Q_GLOBAL>(qtab, sQ, sRQ, tid);
    if (SB == 1) sLut[tid] = norm_lut[tid];
    int bad = 0;
    const bool check_range = SB != 4 && g.maxval < (SB == 1 ? 255 : 65535);

    uint4 raw[Raw::NQ];
    auto load_tile = [&](int tx0, int ty0) {
        if constexpr (LAY == LAY_TIGHT)
            Raw::load(fbase, fbytes, g, tx0, ty0, tid, raw);
        else
            Raw::load(sa, foff, g, tx0, ty0, tid, raw);
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
        const int x0 = mx0 * 8 * HR;
        const int y0 = my * ROWS;

        front_stage<Raw::NCHUNK>(sRaw, tid, raw);
        __syncthreads();
        {  // prefetch the next tile's pixels; they land while this tile computes
            const int nt = tile + gridDim.x;
            if (nt < ntiles) {
                const int ny = nt / tiles_per_row;
                load_tile((nt - ny * tiles_per_row) * 256, ny * G::ROWS);
            }
        }

        // ---- A: colour + subsampling + row pass (color.rs:75-100, padder.rs: outside
        //      = black, subsampling.rs Subsampler::rect x outer / y inner, arai.rs:97-99)
        // the range check (color.rs:63-65) only where a sample can exceed maxval:
        // not for u8 samples with maxval 255 or u16 with 65535 (the PPM norm)
        auto phase_a = [&](auto range_check) {
            constexpr bool CHECK = decltype(range_check)::value;
            const int h = tid % SP, job = tid / SP;
            const int c = job % CB, r = job / CB;  // chroma block, chroma row
            const int lx0 = c * 8 * HR + 8 * h;    // first pixel column of the job
            uint32_t pw[VR * NPL][SB == 4 ? 1 : PXW];  // raw bytes of the job's VR pixel rows (integer samples)
            const float* fsrc[VR * NPL];               // the rows themselves (float samples)
#pragma unroll
            for (int dy = 0; dy < VR; ++dy) {
#pragma unroll
                for (int p = 0; p < NPL; ++p) {
                    const int ly = r * VR + dy;
                    int mis;
                    if constexpr (LAY == LAY_TIGHT)
                        mis = Raw::misalign32(fbase, g, x0, y0 + ly);
                    else
                        mis = Raw::misalign32(sa.plane[p] + foff, sa, x0, y0 + ly);
                    const uint8_t* src = sRaw + (ly * NPL + p) * Raw::RS + mis + lx0 * SPP * SB;
                    fsrc[dy * NPL + p] = reinterpret_cast<const float*>(src);
                    if constexpr (SB == 4) {
                        pw[dy * NPL + p][0] = 0u;
                    } else if ((mis & 7) == 0) {
#pragma unroll
                        for (int k = 0; k < PXW / 2; ++k) {
                            const uint2 u = reinterpret_cast<const uint2*>(src)[k];
                            pw[dy * NPL + p][2 * k] = u.x;
                            pw[dy * NPL + p][2 * k + 1] = u.y;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < PXW; ++k)
                            pw[dy * NPL + p][k] = (uint32_t)src[4 * k] | ((uint32_t)src[4 * k + 1] << 8) |
                                                  ((uint32_t)src[4 * k + 2] << 16) | ((uint32_t)src[4 * k + 3] << 24);
                    }
                }
            }
            float yv[VR][8];
            float cbv[8], crv[8];  // (4:2:x: the job's NCS = 4 samples first)
            uint32_t smax = 0;  // largest sample of the job (a sample above maxval panics in color.rs:63-65)
#pragma unroll
            for (int k = 0; k < NCS; ++k) {  // chroma sample k of the job
                float cbs = 0.0f, crs = 0.0f;
#pragma unroll
                for (int dx = 0; dx < HR; ++dx) {
#pragma unroll
                    for (int dy = 0; dy < VR; ++dy) {
                        const int jx = k * HR + dx;  // pixel within the job row
                        float rr, gg, bb;
                        if constexpr (SB == 4) {  // Image<f32> dots as given (0.0 past the edges)
                            if constexpr (LAY == LAY_PLANAR) {
                                rr = fsrc[dy * NPL][jx];
                                gg = fsrc[dy * NPL + 1][jx];
                                bb = fsrc[dy * NPL + 2][jx];
                            } else {
                                rr = fsrc[dy][jx * SPP];
                                gg = fsrc[dy][jx * SPP + 1];
                                bb = fsrc[dy][jx * SPP + 2];
                                if constexpr (LAY != LAY_TIGHT) {
                                    const float s0 = rr;
                                    rr = sa.bgr ? bb : rr;
                                    bb = sa.bgr ? s0 : bb;
                                }
                            }
                        } else {
                            uint32_t sv[3];
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) {
                                const int si = LAY == LAY_PLANAR ? jx : jx * SPP + ch;  // sample index in the row
                                const uint32_t* rw = pw[LAY == LAY_PLANAR ? dy * NPL + ch : dy];
                                sv[ch] = SB == 1 ? (rw[si >> 2] >> (8 * (si & 3))) & 0xFFu
                                                 : (rw[si >> 1] >> (16 * (si & 1))) & 0xFFFFu;
                            }
                            if constexpr (LAY == LAY_RGB || LAY == LAY_RGBX) {  // B,G,R[,x]: two selects per pixel
                                const uint32_t s0 = sv[0];
                                sv[0] = sa.bgr ? sv[2] : sv[0];
                                sv[2] = sa.bgr ? s0 : sv[2];
                            }
                            if constexpr (CHECK) smax = max(smax, max(sv[0], max(sv[1], sv[2])));
                            if (SB == 1) {
                                rr = sLut[sv[0]];
                                gg = sLut[sv[1]];
                                bb = sLut[sv[2]];
                            } else {
                                rr = norm_lut[sv[0]];
                                gg = norm_lut[sv[1]];
                                bb = norm_lut[sv[2]];
                            }
                        }
                        float y, cb, cr;
                        rgb_to_ycbcr<SB != 4>(rr, gg, bb, y, cb, cr);
                        yv[dy][jx] = y;
                        if (dx == 0 && dy == 0) {
                            cbs = cb;
                            crs = cr;
                        } else {
                            cbs = cbs + cb;
                            crs = crs + cr;
                        }
                    }
                }
                if (HR * VR > 1) {  // average() divides by the sample count
                    cbs = cbs / (float)(HR * VR);
                    crs = crs / (float)(HR * VR);
                }
                cbv[k] = cbs;
                crv[k] = crs;
            }
            if constexpr (CHECK) bad |= (int)(smax > (uint32_t)g.maxval);  // status bit 1
#pragma unroll
            for (int dy = 0; dy < VR; ++dy) {
                const int ly = r * VR + dy;
                arai8(yv[dy]);
                front_store_row<G>(sT, (ly >> 3) * 32 + c * HR + h, ly & 7, yv[dy]);
            }
            if constexpr (SP == 1) {
                arai8(cbv);
                arai8(crv);
                front_store_row<G>(sT, NYB + c, r, cbv);
                front_store_row<G>(sT, NYB + CB + c, r, crv);
            } else {
                // the pair (h = 0, 1) holds chroma samples 0..3 and 4..7 of the row:
                // h = 0 takes the row pass of Cb, h = 1 that of Cr, each swapping
                // the four samples the other needs (DPP quad_perm [1,0,3,2]: lane ^ 1)
                float fr[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float send = h ? cbv[k] : crv[k];
                    const float recv = __int_as_float(
                        __builtin_amdgcn_update_dpp(0, __float_as_int(send), 0xB1, 0xF, 0xF, false));
                    fr[k] = h ? recv : cbv[k];
                    fr[4 + k] = h ? crv[k] : recv;
                }
                arai8(fr);
                front_store_row<G>(sT, NYB + (h ? CB : 0) + c, r, fr);
            }
        };
        if (tid < NJ) {
            if (check_range)
                phase_a(std::integral_constant<bool, true>{});
            else
                phase_a(std::integral_constant<bool, false>{});
        }
        __syncthreads();
        DMMT_TRACE(0);
        front_column_pass<G, NARROW, SB == 4>(sT, Q_GLOBAL ? qtab : sQ, sRQ, tid, g.maxval == 0, g, frame, mx0, my, coef, coef_lo, coef_hi);
        DMMT_TRACE(2);
    }

    if (bad) raise_status(status, bad);  // 1: sample above maxval
    DMMT_TRACE(5);
    DMMT_TRACE_FLUSH(0, 0);
}

template <int HR, int VR, typename Sample, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front(const Sample* __restrict__ rgb, size_t frame_stride, Geom g,
                                               const float* __restrict__ norm_lut,
                                               const float* __restrict__ qtab,  // [2][64] natural, as f32
                                               int16_t* __restrict__ coef, int* __restrict__ status) {
    front_body<HR, VR, Sample, LAY_TIGHT>(rgb, frame_stride, SurfArgs{}, g, norm_lut, qtab, coef, status);
}

// the same tile loop over a surface (frame_stride in bytes)
template <int HR, int VR, typename Sample, int LAY, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_surf(SurfArgs sa, size_t frame_stride, Geom g,
                                                    const float* __restrict__ norm_lut,
                                                    const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                    int* __restrict__ status) {
    front_body<HR, VR, Sample, LAY>(nullptr, frame_stride, sa, g, norm_lut, qtab, coef, status);
}

// the narrow twins (integer samples)
template <int HR, int VR, typename Sample, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_n(const Sample* __restrict__ rgb, size_t frame_stride, Geom g,
                                                 const float* __restrict__ norm_lut, const float* __restrict__ qtab,
                                                 int16_t* __restrict__ coef, int* __restrict__ status,
                                                 int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    front_body<HR, VR, Sample, LAY_TIGHT, true>(rgb, frame_stride, SurfArgs{}, g, norm_lut, qtab, coef, status, coef_lo,
                                                coef_hi);
}
template <int HR, int VR, typename Sample, int LAY, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_surf_n(SurfArgs sa, size_t frame_stride, Geom g,
                                                      const float* __restrict__ norm_lut,
                                                      const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                      int* __restrict__ status, int16_t* __restrict__ coef_lo,
                                                      int8_t* __restrict__ coef_hi) {
    front_body<HR, VR, Sample, LAY, true>(nullptr, frame_stride, sa, g, norm_lut, qtab, coef, status, coef_lo, coef_hi);
}

// ============================================================== k_hist
// One thread per block, emission order (grid-stride over the frame's blocks):
//  * the DC difference to the previous block of the component (categorize.rs:
//    153-169; the predictor reset at restart-interval starts, an extension) and
//    the DC histograms;
//  * the block's AC symbols (categorize.rs:132-151): a register walk over its 63
//    AC coefficients in zigzag order -- a ZRL per 16 zeros before a non-zero,
//    (run & 15) << 4 | category, EOB after trailing zeros -- counted into the AC
//    histograms (symbol_counting.rs:55-74), and its last non-zero position
//    (k_emit's walk order).
// The DC is read from the block itself (index 0 of the column-major block).
// CHECK: an AC -32768 can occur (Image<f32> dots or host blocks); it has no
// category (categorize.rs:25-30).  Integer samples bound |v| by 2049 and skip the
// test (four instructions per position of the walk).
struct HistCoef {
    uint32_t w[32];  // zigzag position 2i in the low half of w[i], 2i+1 in the high half
};

// (the fused tables, defined below)
constexpr int kTailSmallWords = 4 + 4 * 16;
__device__ __forceinline__ void tables_tail(uint8_t* lds, const uint32_t* ac_hist, const uint32_t* dc_hist, int frame,
                                            const Geom& g, uint32_t* __restrict__ code_tab, uint8_t* __restrict__ out,
                                            size_t out_stride, uint32_t* __restrict__ hdr_len,
                                            const uint8_t* __restrict__ qtab_u8, int bits_per_channel,
                                            int* __restrict__ status, int* sCnt, int* sBits);
constexpr int kHistCopies = 4, kHistCopyWords = 545;
constexpr int kTailLdsBytes = 7072;  // tables_tail's per-table regions (static_assert below)

// FUSE (tables_fusable): the frame's last workgroup to finish also builds the four
// Huffman tables and the header (tables_tail), so no k_tables launch follows.
// Eight waves per SIMD (at most 64 VGPRs): the tail alone would take more, and the
// histogram loop wants the occupancy.
#ifndef DMMT_HIST_NEWEST_FIRST
#define DMMT_HIST_NEWEST_FIRST 0  // study builds: 1 = every thread takes its passes in descending block order
#endif
// NARROW (k_hist_n): the blocks come in the 80-byte form (coef_format.hpp): one lo
// and four hi loads, 20 registers; position kk >= 8 is a byte, and an escape byte
// (a wave vote inside the non-zero branch) takes its int16 from coef.  The
// -32768 test then lives at the lo positions and in that branch.
template <bool CHECK, bool FUSE, bool NARROW>
__device__ __forceinline__ void hist_body(const int16_t* __restrict__ coef, const int16_t* __restrict__ coef_lo,
                                          const int8_t* __restrict__ coef_hi, int16_t* __restrict__ dcdiff,
                                          uint8_t* __restrict__ lastnz, const Geom& g,
                                          uint32_t* __restrict__ ac_hist /*[frames][reps][2][256]*/,
                                          uint32_t* __restrict__ dc_hist /*[frames][reps][2][16]*/,
                                          int* __restrict__ status, uint32_t* __restrict__ arrive,
                                          uint32_t* __restrict__ code_tab, uint8_t* __restrict__ out,
                                          size_t out_stride, uint32_t* __restrict__ hdr_len,
                                          const uint8_t* __restrict__ qtab_u8, int bits_per_channel) {
    // four copies of the histograms (lane & 3): the lanes of a wave often count
    // the same symbol at the same position; 545 words apart (different banks).
    // FUSE: the same LDS then holds the tables' work (tables_tail).
    constexpr int NC = kHistCopies, HS = kHistCopyWords;
    constexpr int kWords = FUSE && kTailLdsBytes / 4 > NC * HS ? kTailLdsBytes / 4 : NC * HS;
    __shared__ __attribute__((aligned(16))) uint32_t sH[kWords];  // per copy: [AC luma 256][AC chroma 256][DC luma 16][DC chroma 16]
    __shared__ int sSmall[FUSE ? kTailSmallWords : 1];
    __shared__ uint32_t sLastWg;
    const int tid = threadIdx.x;
    const int frame = blockIdx.y;
    for (int i = tid; i < NC * HS; i += 256) sH[i] = 0;
    __syncthreads();
    uint32_t* const H = sH + HS * (tid & 3);
    const long long base = (long long)frame * g.bpf;
    const int lane = lane_id();
    int bad = 0;
    // block el = MCU m, block k of it (bpf < 2^31: every index fits 32 bits); the
    // loop steps (m, k) and m mod the restart interval instead of dividing again
    const uint32_t bpf = (uint32_t)g.bpf, bpm = (uint32_t)g.bpm, ri = (uint32_t)max(g.restart_interval, 1);
    const uint32_t stride = gridDim.x * 256u, sm = stride / bpm, sk = stride - sm * bpm;
    uint32_t el = blockIdx.x * 256u + (uint32_t)tid;
#if DMMT_HIST_NEWEST_FIRST
    // study build: the passes in descending block order (k_front's most recently
    // written lines first).  Every thread of the grid counts the same passes down --
    // a wave's lanes stay on neighbouring blocks for the DC shuffle -- and sits out
    // the first when it lies past the frame; (m, k, mr) step back from the first
    // block the thread takes.
    const uint32_t passes = (bpf + stride - 1u) / stride;
    el += (passes - 1u) * stride;
    const uint32_t el1 = el < bpf ? el : el - stride;
    uint32_t m = el1 / bpm, k = el1 - m * bpm, mr = m % ri;
#else
    uint32_t m = el / bpm, k = el - m * bpm, mr = m % ri;
#endif
    const uint32_t smr = sm % ri;
#if DMMT_HIST_NEWEST_FIRST
    for (uint32_t left = passes; left > 0; --left, el -= stride) {
        if (el >= bpf) continue;
#else
    for (; el < bpf; el += stride) {
#endif
        const long long e = base + el;
        uint32_t cw[NARROW ? 1 : 32];  // column-major (coef_pos)
        NarrowCoef nc;
        if constexpr (NARROW) {
            load_narrow(coef_lo, coef_hi, e, nc);
            cw[0] = nc.lo[0];
        } else {
            const uint4* q = reinterpret_cast<const uint4*>(coef + e * 64);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint4 v = q[i];
                cw[4 * i] = v.x, cw[4 * i + 1] = v.y, cw[4 * i + 2] = v.z, cw[4 * i + 3] = v.w;
            }
        }
        const int t = k < (uint32_t)g.n_luma ? 0 : 1;
        // DC: the predictor is the previous block of the component, usually a few
        // lanes back in this wave (its DC over a lane shuffle), else a load -- issued
        // here, used after the AC walk, so that the walk hides its latency
        const bool restart = g.restart_interval > 0 && mr == 0;
        int back = 0;  // blocks back to the predictor; 0: none (predictor 0)
        if (k > 0 && k < (uint32_t)g.n_luma)
            back = 1;
        else if (m > 0 && !restart)
            back = (k == 0) ? (int)bpm - g.n_luma + 1 : (int)bpm;
        const int cur = (int)(int16_t)(cw[0] & 0xFFFFu);
        const int nb = __shfl_up(cur, (unsigned)back, 64);  // (lanes below `back` get their own)
        int pv = 0;
        if (back) pv = lane >= back ? nb : NARROW ? (int)coef_lo[(e - back) * 8] : (int)coef[(e - back) * 64];
        // AC: zigzag order in registers (a constant permutation of the 64 halves)
        HistCoef b;
        if constexpr (!NARROW) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int i0 = coef_pos(2 * j), i1 = coef_pos(2 * j + 1);
                const uint32_t lo = (cw[i0 >> 1] >> (16 * (i0 & 1))) & 0xFFFFu;
                const uint32_t hi = (cw[i1 >> 1] >> (16 * (i1 & 1))) & 0xFFFFu;
                b.w[j] = lo | (hi << 16);
            }
        }
        uint32_t* h = H + 256 * t;
        // l16 = 16 * (position of the last non-zero + 1): the zero run before position
        // kk is r16 / 16 with r16 = 16 * kk - l16, (run & 15) << 4 = r16 & 0xF0
        int l16 = 16;
        uint32_t zrl = 0;
        // (narrow blocks: the escape test only in a wave that holds a flagged block)
        auto walk = [&](auto with_escapes) {
            constexpr bool ESC = decltype(with_escapes)::value;
#pragma unroll
            for (int kk = 1; kk < 64; ++kk) {
                int v;
                if constexpr (NARROW)
                    v = narrow_at(nc, kk);
                else
                    v = (kk & 1) ? ((int)b.w[kk >> 1] >> 16) : (int)(int16_t)(b.w[kk >> 1] & 0xFFFFu);
                if (v != 0) {
                    if (NARROW && ESC && !coef_in_lo(kk)) {
                        if (__builtin_amdgcn_ballot_w64(v == kCoefEscape) != 0) {  // rare: the int16 from the wide store
                            if (v == kCoefEscape) v = (int)coef[e * 64 + coef_pos(kk)];
                            if (CHECK && v == -32768) bad |= 4;
                        }
                    } else if (CHECK) {
                        bad |= v == -32768 ? 4 : 0;
                    }
                    const int r16 = 16 * kk - l16;
                    zrl += (uint32_t)(r16 >> 8);
                    atomicAdd(&h[(r16 & 0xF0) | category_fast(v)], 1u);
                    l16 = 16 * kk + 16;
                }
            }
        };
        if constexpr (NARROW) {
            if (__builtin_amdgcn_ballot_w64(narrow_flag(nc)) != 0)  // (uniform) rare: a block of the wave escapes
                walk(std::integral_constant<bool, true>{});
            else
                walk(std::integral_constant<bool, false>{});
        } else {
            walk(std::integral_constant<bool, false>{});
        }
        if (zrl) atomicAdd(&h[0xF0], zrl);
        if (l16 < 16 * 64) atomicAdd(&h[0], 1u);  // EOB
        lastnz[e] = (uint8_t)((l16 >> 4) - 1);      // 0: no non-zero AC coefficient
        {
            const int16_t d = (int16_t)(cur - pv);  // i16 subtraction
            bad |= d == -32768 ? 4 : 0;               // no category (categorize.rs:25-30)
            dcdiff[e] = d;
            atomicAdd(&H[512 + 16 * t + category_of(d)], 1u);
        }
#if DMMT_HIST_NEWEST_FIRST
        // (unsigned: a borrow wraps past bpm / ri; m is not read once it would pass 0)
        m -= sm, k -= sk, mr -= smr;
        if (k >= bpm) k += bpm, --m, --mr;
        if (mr >= ri) mr += ri;
#else
        m += sm, k += sk, mr += smr;
        if (k >= bpm) k -= bpm, ++m, ++mr;
        if (mr >= ri) mr -= ri;
#endif
    }
    if (bad) raise_status(status, bad);
    __syncthreads();
    const size_t rep = (size_t)frame * kHistReps + blockIdx.x % kHistReps;
    for (int i = tid; i < 544; i += 256) {
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) v += sH[HS * c + i];
        if (!v) continue;
        if (i < 512)
            atomicAdd(&ac_hist[rep * 512 + i], v);
        else
            atomicAdd(&dc_hist[rep * 32 + (i - 512)], v);
    }
    if (FUSE) {  // count this workgroup in (arrive_last); the frame's last one builds the tables
#if !DMMT_ARRIVE_FORMAL
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's flush atomics have completed
#endif
        __syncthreads();  // (also: every wave's sH reads are done before the tail reuses the LDS)
        if (tid == 0) sLastWg = arrive_last(arrive + (size_t)frame * kArriveWords, blockIdx.x, gridDim.x);
        __syncthreads();
        if (sLastWg) {
            arrive_acquire();
            tables_tail(reinterpret_cast<uint8_t*>(sH), ac_hist, dc_hist, frame, g, code_tab, out, out_stride, hdr_len,
                        qtab_u8, bits_per_channel, status, sSmall, sSmall + 4);
        }
    }
}

template <bool CHECK, bool FUSE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_hist(const int16_t* __restrict__ coef, int16_t* __restrict__ dcdiff,
                                              uint8_t* __restrict__ lastnz, Geom g,
                                              uint32_t* __restrict__ ac_hist, uint32_t* __restrict__ dc_hist,
                                              int* __restrict__ status, uint32_t* __restrict__ arrive,
                                              uint32_t* __restrict__ code_tab, uint8_t* __restrict__ out,
                                              size_t out_stride, uint32_t* __restrict__ hdr_len,
                                              const uint8_t* __restrict__ qtab_u8, int bits_per_channel) {
    hist_body<CHECK, FUSE, false>(coef, nullptr, nullptr, dcdiff, lastnz, g, ac_hist, dc_hist, status, arrive, code_tab,
                                  out, out_stride, hdr_len, qtab_u8, bits_per_channel);
}
template <bool CHECK, bool FUSE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_hist_n(const int16_t* __restrict__ coef, const int16_t* __restrict__ coef_lo,
                                                const int8_t* __restrict__ coef_hi, int16_t* __restrict__ dcdiff,
                                                uint8_t* __restrict__ lastnz, Geom g,
                                                uint32_t* __restrict__ ac_hist, uint32_t* __restrict__ dc_hist,
                                                int* __restrict__ status, uint32_t* __restrict__ arrive,
                                                uint32_t* __restrict__ code_tab, uint8_t* __restrict__ out,
                                                size_t out_stride, uint32_t* __restrict__ hdr_len,
                                                const uint8_t* __restrict__ qtab_u8, int bits_per_channel) {
    hist_body<CHECK, FUSE, true>(coef, coef_lo, coef_hi, dcdiff, lastnz, g, ac_hist, dc_hist, status, arrive, code_tab,
                                 out, out_stride, hdr_len, qtab_u8, bits_per_channel);
}

// ============================================================== k_tables
// One 512-thread workgroup per (table, frame): blockIdx.x = table (0 luma DC,
// 1 luma AC, 2 chroma DC, 3 chroma AC); thread s < 256 = symbol / leaf s,
// thread 256 + j = package j.
//  1 histograms summed over the replicas (k_emit zeroes them after this launch);
//    every workgroup counts the present symbols of all four tables, which place
//    the DHT segments
//  2 compact the present symbols and rank them by (frequency, symbol): the stable
//    ascending sort of symbol_counting.rs:92-94 over the f>0 filter of 25-32
//  3 package-merge, limit 15 (length_limited.rs:37-134): level k = merge of the
//    pairwise packages of level k-1 with the leaves, ties leaf-first.  A leaf's
//    count of lighter packages never falls from one level to the next and a
//    package's count of leaves not heavier never rises (every level's items are
//    no heavier than the previous level's at the same index), so each search
//    gallops from its previous answer: usually one or two LDS reads per level
//  4 solution from the deepest level (n-1 packages): a scalar chain over
//    per-level package bitmasks with word prefix counts; lengths, +1 on the least
//    frequent symbol (symbol_counting.rs:85-90)
//  5 canonical codes over the reversed list (huffman/encoder.rs:45-67,116-119)
//  6 this table's DHT segment; table 0's workgroup also writes SOI, APP0, DQT,
//    SOF0, [DRI], SOS (encoder.rs:125-262)

#define PM_LEVELS 15

__device__ __forceinline__ void put_be16(uint8_t* p, int v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}

// write_table_header for a single-component (grayscale) file, g.ncomp == 1: the
// colour header with every chroma part taken out and the order kept -- SOI, APP0,
// one DQT (Tq 0), SOF0 of length 11 (Nf 1, component 01 11 00), DHT luma AC, DHT
// luma DC, [DRI], the 10-byte SOS.  Only tables 0 and 1 are built (nt[2] = nt[3] = 0).
__device__ void write_table_header_gray(uint8_t* o, int tab, int t0, int step, int n, const int nt[4],
                                        const uint8_t* symrank, const int* bits16, const Geom& g,
                                        const uint8_t* __restrict__ qtab_u8, int bits_per_channel,
                                        uint32_t* hdr_len, int dq) {
    if (tab > 1) return;
    const int off_lac = 2 + 18 + 69 + 13;
    const int off_ldc = off_lac + 21 + nt[1];
    const int dht = tab == 0 ? off_ldc : off_lac;
    for (int s = t0; s < n; s += step) o[dht + 21 + s] = symrank[n - 1 - s];
    for (int s = t0; s < 16; s += step) o[dht + 5 + s] = (uint8_t)bits16[s];
    if (t0 == 0) {
        uint8_t* d = o + dht;
        d[0] = 0xFF;
        d[1] = 0xC4;
        put_be16(d + 2, 2 + 17 + n);
        d[4] = tab == 0 ? 0x00 : 0x11;
    }
    if (tab != 0) return;
    const int pos_after_dht = off_ldc + 21 + nt[0];
    const int pos_sos = pos_after_dht + (g.restart_interval > 0 ? 6 : 0);
    if (t0 == 0) {
        o[0] = 0xFF;
        o[1] = 0xD8;  // SOI
        const uint8_t app0[18] = {0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 0x01, 0x02, 0x00, 0x00, 0x48, 0x00, 0x48, 0, 0};
        for (int i = 0; i < 18; ++i) o[2 + i] = app0[i];
        uint8_t* d = o + 20;  // DQT, the luma table in zigzag order
        d[0] = 0xFF;
        d[1] = 0xDB;
        put_be16(d + 2, 67);
        d[4] = 0;
        uint8_t* sof = o + 89;
        sof[0] = 0xFF;
        sof[1] = 0xC0;
        put_be16(sof + 2, 11);
        sof[4] = (uint8_t)bits_per_channel;
        put_be16(sof + 5, g.sof_height);
        put_be16(sof + 7, g.width);
        sof[9] = 1;
        sof[10] = 1;
        sof[11] = 0x11;
        sof[12] = 0;
        if (g.restart_interval > 0) {  // extension: DRI
            uint8_t* r = o + pos_after_dht;
            r[0] = 0xFF;
            r[1] = 0xDD;
            put_be16(r + 2, 4);
            put_be16(r + 4, g.restart_interval);
        }
        const uint8_t sos[10] = {0xFF, 0xDA, 0x00, 0x08, 0x01, 0x01, 0x01, 0x00, 0x3F, 0x00};
        for (int i = 0; i < 10; ++i) o[pos_sos + i] = sos[i];
        *hdr_len = (uint32_t)(pos_sos + 10);
    }
    if (dq >= 0) {
        o[25 + t0] = (uint8_t)dq;
        return;
    }
    for (int s = t0; s < 64; s += step) o[25 + s] = qtab_u8[c_zigzag[s]];
}

// The table's DHT segment (encoder.rs:169-181: BITS, then the symbols most frequent
// first, i.e. symrank -- symbols by ascending frequency -- reversed) and, for table
// 0, SOI, APP0, DQT x2, SOF0, [DRI], SOS (encoder.rs:125-262) and the header length;
// a later stripe of an image (dmmt_stripe_*) writes no header.  Written by threads
// t0, t0 + step, ... of the table (k_tables: 256 per table; k_hist's fused tail: 64,
// whose table-0 wave passes the DQT bytes of zigzag position t0 already loaded:
// dq = luma | chroma << 8, else -1).
__device__ void write_table_header(uint8_t* o, int tab, int t0, int step, int n, const int nt[4],
                                   const uint8_t* symrank, const int* bits16, const Geom& g,
                                   const uint8_t* __restrict__ qtab_u8, int bits_per_channel, uint32_t* hdr_len,
                                   int dq = -1) {
    if (!g.stripe_first) {  // a later stripe of an image: tables only, no header
        if (tab == 0 && t0 == 0) *hdr_len = 0;
        return;
    }
    if (g.ncomp == 1) {  // (uniform) a single-component file
        write_table_header_gray(o, tab, t0, step, n, nt, symrank, bits16, g, qtab_u8, bits_per_channel, hdr_len, dq);
        return;
    }
    const int pos_dht0 = 2 + 18 + 69 + 69 + 19;
    const int off_lac = pos_dht0;
    const int off_ldc = off_lac + 21 + nt[1];
    const int off_cac = off_ldc + 21 + nt[0];
    const int off_cdc = off_cac + 21 + nt[3];
    const int dht = tab == 0 ? off_ldc : tab == 1 ? off_lac : tab == 2 ? off_cdc : off_cac;
    for (int s = t0; s < n; s += step) o[dht + 21 + s] = symrank[n - 1 - s];  // DHT symbols in reversed order (encoder.rs:180)
    for (int s = t0; s < 16; s += step) o[dht + 5 + s] = (uint8_t)bits16[s];
    if (t0 == 0) {
        uint8_t* d = o + dht;
        d[0] = 0xFF;
        d[1] = 0xC4;
        put_be16(d + 2, 2 + 17 + n);
        const uint8_t kind[4] = {0x00, 0x11, 0x02, 0x13};  // encoder.rs:92-98 TableKind
        d[4] = kind[tab];
    }
    if (tab != 0) return;
    const int pos_after_dht = pos_dht0 + 4 * 21 + nt[0] + nt[1] + nt[2] + nt[3];
    const int pos_sos = pos_after_dht + (g.restart_interval > 0 ? 6 : 0);
    if (t0 == 0) {
        o[0] = 0xFF;
        o[1] = 0xD8;  // SOI
        const uint8_t app0[18] = {0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 0x01, 0x02, 0x00, 0x00, 0x48, 0x00, 0x48, 0, 0};
        for (int i = 0; i < 18; ++i) o[2 + i] = app0[i];
        for (int q = 0; q < 2; ++q) {  // DQT, table in zigzag order (encoder.rs:193-212)
            uint8_t* d = o + 20 + 69 * q;
            d[0] = 0xFF;
            d[1] = 0xDB;
            put_be16(d + 2, 67);
            d[4] = (uint8_t)q;
        }
        uint8_t* sof = o + 158;  // encoder.rs:227-245
        sof[0] = 0xFF;
        sof[1] = 0xC0;
        put_be16(sof + 2, 17);
        sof[4] = (uint8_t)bits_per_channel;
        put_be16(sof + 5, g.sof_height);
        put_be16(sof + 7, g.width);
        sof[9] = 3;
        sof[10] = 1;
        sof[11] = (uint8_t)((g.hr << 4) | g.vr);
        sof[12] = 0;
        sof[13] = 2;
        sof[14] = 0x11;
        sof[15] = 1;
        sof[16] = 3;
        sof[17] = 0x11;
        sof[18] = 1;
        if (g.restart_interval > 0) {  // extension: DRI
            uint8_t* d = o + pos_after_dht;
            d[0] = 0xFF;
            d[1] = 0xDD;
            put_be16(d + 2, 4);
            put_be16(d + 4, g.restart_interval);
        }
        const uint8_t sos[14] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x01, 0x02, 0x23, 0x03, 0x23, 0x00, 0x3F, 0x00};
        for (int i = 0; i < 14; ++i) o[pos_sos + i] = sos[i];
        *hdr_len = (uint32_t)(pos_sos + 14);
    }
    if (dq >= 0) {
        o[25 + t0] = (uint8_t)dq;
        o[94 + t0] = (uint8_t)(dq >> 8);
        return;
    }
    for (int s = t0; s < 128; s += step) {
        const int q = s >> 6, i = s & 63;
        o[20 + 69 * q + 5 + i] = qtab_u8[q * 64 + c_zigzag[i]];
    }
}

// #{j < m : pair sum prev[2j] + prev[2j+1] < x}, known to be >= lb (sums ascending)
__device__ __forceinline__ int packages_below(const unsigned long long* prev, int m, unsigned long long x, int lb) {
    const ulonglong2* pr = reinterpret_cast<const ulonglong2*>(prev);
    int lo = lb, hi = m, step = 1;  // every j < lo is below x; the answer is in [lo, hi]
    while (lo < hi) {               // gallop up
        const int probe = min(lo + step - 1, hi - 1);
        const ulonglong2 p = pr[probe];
        if (p.x + p.y < x) {
            lo = probe + 1;
            step <<= 1;
        } else {
            hi = probe;
            break;
        }
    }
    while (lo < hi) {  // bisect [lo, hi]
        const int mid = (lo + hi) >> 1;
        const ulonglong2 p = pr[mid];
        if (p.x + p.y < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// #{i < m : f[i] <= x}, known to be <= ub (f ascending)
__device__ __forceinline__ int leaves_not_above(const unsigned long long* f, int m, unsigned long long x, int ub) {
    int lo = 0, hi = min(ub, m), step = 1;  // every i < lo is <= x, every i >= hi is > x
    while (lo < hi) {                       // gallop down
        const int probe = max(hi - step, lo);
        if (f[probe] <= x) {
            lo = probe + 1;
            break;
        }
        hi = probe;
        step <<= 1;
    }
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (f[mid] <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(512) void k_tables(const uint32_t* __restrict__ ac_hist,
                                                const uint32_t* __restrict__ dc_hist,
                                                uint32_t* __restrict__ code_tab,  // [frames][4][256]
                                                uint8_t* __restrict__ out, size_t out_stride,
                                                uint32_t* __restrict__ hdr_len, Geom g,
                                                const uint8_t* __restrict__ qtab_u8,  // [2][64] natural
                                                int bits_per_channel, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) unsigned long long sKey[256];  // present symbols, symbol order
    __shared__ __attribute__((aligned(16))) unsigned long long sF[256];    // frequencies, ascending
    __shared__ __attribute__((aligned(16))) unsigned long long sLev[2][512];
    __shared__ unsigned long long sPk[PM_LEVELS][8];  // package positions per level (bitmask)
    __shared__ int sPkCum[PM_LEVELS][8];              // packages in the words before
    __shared__ uint8_t sSym[256];  // symbols by rank
    __shared__ int sLen[256];      // code length by rank
    __shared__ int sCnt[4][4];     // [wave][table] present symbols
    __shared__ int sLeaf[PM_LEVELS];
    __shared__ uint32_t sWave[4];
    __shared__ int sBits[16];

    DMMT_TRACE_START;
    const int tab = blockIdx.x, frame = blockIdx.y;
    const int t = threadIdx.x, lane = lane_id();
    const int s = t & 255, wave = s >> 6;
    const bool sym_thread = t < 256;

    // ---- 1
    unsigned long long fr[4] = {0, 0, 0, 0};
    if (sym_thread) {
        uint32_t va[2][kHistReps], vd[2][kHistReps];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < kHistReps; ++r) {
                va[c][r] = ac_hist[(((size_t)frame * kHistReps + r) * 2 + c) * 256 + s];
                vd[c][r] = s < 16 ? dc_hist[((size_t)frame * kHistReps + r) * 32 + c * 16 + s] : 0u;
            }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            unsigned long long a = 0, d = 0;
#pragma unroll
            for (int r = 0; r < kHistReps; ++r) {
                a += va[c][r];
                d += vd[c][r];
            }
            fr[2 * c] = d;
            fr[2 * c + 1] = a;
        }
    }
    const unsigned long long f = fr[tab];
    const unsigned long long own = __ballot(f > 0);
    if (sym_thread) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long b = __ballot(fr[q] > 0);
            if (lane == 0) sCnt[wave][q] = __popcll(b);
        }
        if (s < 16) sBits[s] = 0;
    } else if (s < PM_LEVELS * 8) {
        sPk[s >> 3][s & 7] = 0ull;
    }
    __syncthreads();
    int nt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) nt[q] = sCnt[0][q] + sCnt[1][q] + sCnt[2][q] + sCnt[3][q];
    const int n = nt[tab];
    if (sym_thread && f > 0) {
        int idx = __popcll(own & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) idx += sCnt[w][tab];
        sKey[idx] = (f << 8) | (unsigned)s;
    }
    if (sym_thread && ((s == 0 && n == 0) || ((tab & 1) && s == 0xFF && f > 0))) raise_status(status, 2);
    __syncthreads();
    DMMT_TRACE(10);

    // ---- 2: rank = present keys below mine
    if (sym_thread && f > 0) {
        const unsigned long long mykey = (f << 8) | (unsigned)s;
        const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(sKey);
        int r = 0;
        for (int j = 0; j < (n >> 1); ++j) {
            const ulonglong2 kk = k2[j];
            r += (kk.x < mykey ? 1 : 0) + (kk.y < mykey ? 1 : 0);
        }
        if (n & 1) r += sKey[n - 1] < mykey ? 1 : 0;
        sF[r] = f;
        sSym[r] = (uint8_t)s;
        sLev[0][r] = f;
    }
    __syncthreads();
    DMMT_TRACE(11);

    // ---- 3
    {
        int size_prev = n, np_prev = 0;
        int cnt = sym_thread ? 0 : n;  // previous answer: lower bound (leaf) / upper bound (package)
        const unsigned long long fl = sym_thread && s < n ? sF[s] : 0ull;
        for (int k = 1; k < PM_LEVELS; ++k) {
            const unsigned long long* prev = sLev[(k - 1) & 1];
            unsigned long long* cur = sLev[k & 1];
            const int np = size_prev >> 1;
            if (sym_thread) {
                if (s < n) {  // leaf s: after every package strictly lighter
                    cnt = packages_below(prev, np, fl, cnt);
                    cur[s + cnt] = fl;
                }
            } else if (s < np) {  // package s: after every leaf not heavier
                const ulonglong2 pp = reinterpret_cast<const ulonglong2*>(prev)[s];
                const unsigned long long P = pp.x + pp.y;
                cnt = leaves_not_above(sF, n, P, s < np_prev ? cnt : n);
                const int pos = s + cnt;
                cur[pos] = P;
                atomicOr(&sPk[k][pos >> 6], 1ull << (pos & 63));
            }
            np_prev = np;
            size_prev = n + np;
            __syncthreads();
        }
    }
    DMMT_TRACE(12);

    // ---- 4: leaves in the solution prefix of every level, deepest first: the
    // prefix of level k holds 2 * (packages taken at level k+1) items; the packages
    // among them are the ones taken at level k-1
    if (!sym_thread && s < PM_LEVELS * 8) {
        const int k = s >> 3, w = s & 7;
        int c = 0;
        for (int q = 0; q < w; ++q) c += __popcll(sPk[k][q]);
        sPkCum[k][w] = c;
    }
    __syncthreads();
    if (t == 0) {
        int packages = n - 1;
        for (int k = PM_LEVELS - 1; k >= 0; --k) {
            const int c = max(2 * packages, 0);  // <= 2n - 2 < 512
            const int w = c >> 6, b = c & 63;
            const int pk = sPkCum[k][w] + __popcll(sPk[k][w] & ((1ull << b) - 1ull));
            sLeaf[k] = c - pk;
            packages = pk;
        }
    }
    __syncthreads();
    if (sym_thread && s < n) {
        int len = s == 0 ? 1 : 0;
#pragma unroll
        for (int k = 0; k < PM_LEVELS; ++k) len += s < sLeaf[k] ? 1 : 0;
        sLen[s] = len;
        atomicAdd(&sBits[len - 1], 1);
    }
    __syncthreads();
    DMMT_TRACE(13);

    // ---- 5: code(p) = sum over reversed positions before p of 2^(16 - len)
    uint32_t* ct = code_tab + ((size_t)frame * 4 + tab) * 256;
    {
        const int rk = n - 1 - s;  // rank at reversed position s
        const uint32_t wgt = sym_thread && s < n ? 1u << (16 - sLen[rk]) : 0u;
        const uint32_t incl = wave_incl_scan_full_u32(wgt);
        if (sym_thread && lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t excl = incl - wgt;
        for (int q = 0; q < wave; ++q) excl += sWave[q];
        if (sym_thread && f == 0) ct[s] = 0;
        __syncthreads();  // the zeroes before the codes (a present symbol's entry is written by another thread)
        if (sym_thread && s < n) {
            const int L = sLen[rk];
            const uint32_t pat = excl & 0xFFFFu;  // left aligned u16 (wrapping as in the reference)
            ct[sSym[rk]] = ((uint32_t)L << 16) | (pat >> (16 - L));
        }
    }
    DMMT_TRACE(14);

    // ---- 6: header
    if (!sym_thread) return;
    write_table_header(out + (size_t)frame * out_stride, tab, s, 256, n, nt, sSym, sBits, g, qtab_u8, bits_per_channel,
                       hdr_len + frame);
    DMMT_TRACE(15);
    DMMT_TRACE_FLUSH(0, 1);
}

// ============================================================== fused tables
// k_tables' work done by k_hist's last workgroup of a frame (tables_fusable): wave
// t builds table t (0 luma DC, 1 luma AC, 2 chroma DC, 3 chroma AC).  Frequencies in
// 32 bits: the host fuses only frames whose symbol counts, and thus every package
// weight (at most 15 times their sum), stay below 2^30.  The phases of k_tables:
//  1 the 8 replicas summed (agent-scope loads after the arrival); symbol s = lane
//    + 64 q; the present symbols counted
//  2 symbol_counting.rs:92-94's stable ascending sort over the f > 0 filter of
//    25-32: keys (frequency << 8 | s) sorted in registers (sort_bitonic,
//    wave_merge.hpp; absent symbols are kMergeInf and sort last) when every
//    frequency is below 2^24; else the 64-bit keys compacted and ranked
//    (tail_rank)
//  3 package-merge, limit 15 (length_limited.rs:37-134), in registers: level k is
//    the merge of the leaves (ascending) with the pair sums of level k-1
//    (ascending), ties leaf first -- keys (weight << 1 | is_package), one
//    bitonic merger of the wave (wave_merge.hpp) per level, the package
//    positions of every level kept as 64-bit masks (a ballot per register slot,
//    parked in a lane of a VGPR)
//  4 the solution from the deepest level (n-1 packages), every lane alike, lengths,
//    +1 on the least frequent (symbol_counting.rs:85-90)
//  5 canonical codes over the reversed list (huffman/encoder.rs:45-67,116-119)
//  6 the DHT segment, and for table 0 the rest of the header (write_table_header)
// One barrier: before 6 (every table's symbol count).  LDS per table (bytes):
// F u32[cap] | the keys u64[cap] | Sym u8[cap]; cap = 256 for the AC tables, 16 DC.
#ifndef DMMT_TAIL_SORT2
#define DMMT_TAIL_SORT2 1  // an AC table of at most 128 symbols sorted in two register slots (0: study builds)
#endif
constexpr int kTailLevels = 15;
constexpr int kTailBase[4] = {0, 208, 3536, 3744};
static_assert(kTailBase[3] + 3328 == kTailLdsBytes, "tables_tail's LDS regions");

// Levels 1-14 of the package-merge over n leaves F (ascending) in 64 * EPL element
// merges (n <= 32 * EPL): slot-major, the leaves ascending in the lower half
// (static), the packages DESCENDING in the upper (element S/2 + m holds package
// S/2 - 1 - m), so each level is one bitonic merge.  Level k's package positions
// (a ballot per slot) and the packages before each slot are kept in lane k EPL + s
// of two VGPR pairs, and the solution chain reads them back
// (readlane): leaf[k] = the leaves in the solution prefix of level k.
template <int EPL>
__device__ __forceinline__ void tail_levels(const uint32_t* F, int n, int (&leaf)[kTailLevels]) {
    const int lane = lane_id();
    constexpr int H = EPL == 1 ? 1 : EPL / 2;  // register slots per half (EPL 1: lanes 0-31 / 32-63)
    // leaf index of lower-half slot t / package index of upper-half slot t in this lane
    auto leaf_index = [&](int t) { return EPL == 1 ? lane : 64 * t + lane; };
    auto pkg_index = [&](int t) { return EPL == 1 ? 63 - lane : 32 * EPL - 1 - 64 * t - lane; };
    uint32_t lk[H], pk[H];
    int np = n >> 1;
#pragma unroll
    for (int t = 0; t < H; ++t) {
        const int i = leaf_index(t), j = pkg_index(t);
        lk[t] = i < n ? F[min(i, 255)] << 1 : kMergeInf;
        pk[t] = j >= 0 && j < np ? ((F[2 * j] + F[2 * j + 1]) << 1) | 1u : kMergeInf;  // level 1: pairs of the leaves
    }
    // entry e = k EPL + s (level 0: no packages) in lane e & 63 of register e >> 6
    uint32_t mlo[2] = {0u, 0u}, mhi[2] = {0u, 0u}, mcum[2] = {0u, 0u};
    // the gather's source (see below): lane 2 (31 - (lane & 31)), upper-half slot t's
    // packages from slot EPL - 1 - 2t - (lane >> 5)
    const int src = 8 * (31 - (lane & 31));
    for (int k = 1; k < kTailLevels; ++k) {
        uint32_t x[EPL];
        if constexpr (EPL == 1) {
            x[0] = lane < 32 ? lk[0] : pk[0];
        } else {
#pragma unroll
            for (int t = 0; t < H; ++t) {
                x[t] = lk[t];
                x[H + t] = pk[t];
            }
        }
        merge_bitonic<EPL>(x);
        int before = 0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            const unsigned long long m = __ballot((x[s] & 1u) != 0u);
            const int e = k * EPL + s;
            const bool here = lane == (e & 63);
            if (EPL < 8 || e < 64) {  // (uniform)
                mlo[0] = here ? (uint32_t)m : mlo[0];
                mhi[0] = here ? (uint32_t)(m >> 32) : mhi[0];
                mcum[0] = here ? (uint32_t)before : mcum[0];
            } else {
                mlo[1] = here ? (uint32_t)m : mlo[1];
                mhi[1] = here ? (uint32_t)(m >> 32) : mhi[1];
                mcum[1] = here ? (uint32_t)before : mcum[1];
            }
            before += __popcll(m);
        }
        // the next level's packages: pairs (2j, 2j + 1) -- neighbouring lanes of a
        // slot -- summed in the even lane, then gathered to their descending places
        const int npn = (n + np) >> 1;
        uint32_t q[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) q[s] = (x[s] >> 1) + (lane_xor<1>(x[s]) >> 1);
#pragma unroll
        for (int t = 0; t < H; ++t) {
            uint32_t v;
            if constexpr (EPL == 1) {
                v = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)q[0]);
            } else {
                const uint32_t vh = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)q[EPL - 1 - 2 * t]);
                const uint32_t vl = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)q[EPL - 2 - 2 * t]);
                v = (lane & 32) ? vl : vh;
            }
            const int j = pkg_index(t);
            pk[t] = j >= 0 && j < npn ? (v << 1) | 1u : kMergeInf;
        }
        np = npn;
    }
    // the solution, deepest level first: the prefix of level k holds 2 * (packages
    // taken at level k+1) items, the packages among them are the ones taken at level
    // k-1 (every lane computes it: uniform values)
    int packages = n - 1;
#pragma unroll
    for (int k = kTailLevels - 1; k >= 0; --k) {
        const int cc = max(2 * packages, 0);  // <= 2n - 2 < 64 EPL
        const int e = k * EPL + (cc >> 6), b = cc & 63;
        uint32_t lo, hi, cm;
        if (EPL < 8 || e < 64) {
            lo = (uint32_t)__builtin_amdgcn_readlane((int)mlo[0], e);
            hi = (uint32_t)__builtin_amdgcn_readlane((int)mhi[0], e);
            cm = (uint32_t)__builtin_amdgcn_readlane((int)mcum[0], e);
        } else {
            lo = (uint32_t)__builtin_amdgcn_readlane((int)mlo[1], e - 64);
            hi = (uint32_t)__builtin_amdgcn_readlane((int)mhi[1], e - 64);
            cm = (uint32_t)__builtin_amdgcn_readlane((int)mcum[1], e - 64);
        }
        const unsigned long long m = (((unsigned long long)hi << 32) | lo) & ((1ull << b) - 1ull);
        const int pkc = (int)cm + __popcll(m);
        leaf[k] = cc - pkc;
        packages = pkc;
    }
}

// rank of every present key among the n keys (the stable ascending sort by
// frequency, symbol_counting.rs:92-94: ties by symbol, which the key's low byte
// carries); leaf rank -> F (frequency), Sym.  NS key slots per lane (key i at lane
// i % 64, slot i / 64); the keys read eight at a time, loads together; K: u32 keys
// (frequency << 8 | s) when every frequency is below 2^24, else u64.
template <int NS, typename K>
__device__ __forceinline__ void tail_rank(const K* Key, int n, uint32_t* F, uint8_t* Sym) {
    const int lane = lane_id();
    K mk[NS];
    uint32_t rk[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        mk[r] = lane + 64 * r < n ? Key[lane + 64 * r] : (K)~(K)0;
        rk[r] = 0u;
    }
    constexpr int V = 16 / sizeof(K);  // keys per 16-byte read
    int j = 0;
    for (; j + 4 * V <= n; j += 4 * V) {
        K kk[4 * V];
#pragma unroll
        for (int u = 0; u < 4 * V; ++u) kk[u] = Key[j + u];
#pragma unroll
        for (int u = 0; u < 4 * V; ++u)
#pragma unroll
            for (int r = 0; r < NS; ++r) rk[r] += kk[u] < mk[r] ? 1u : 0u;
    }
    for (; j < n; ++j) {
        const K kk = Key[j];
#pragma unroll
        for (int r = 0; r < NS; ++r) rk[r] += kk < mk[r] ? 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < NS; ++r)
        if (lane + 64 * r < n) {
            F[rk[r]] = (uint32_t)(mk[r] >> 8);
            Sym[rk[r]] = (uint8_t)mk[r];
        }
}

template <typename K>
__device__ __forceinline__ void tail_rank_any(const K* Key, int n, uint32_t* F, uint8_t* Sym) {
    const int ns = (n + 63) >> 6;  // (uniform in the wave)
    if (ns <= 1)
        tail_rank<1>(Key, n, F, Sym);
    else if (ns == 2)
        tail_rank<2>(Key, n, F, Sym);
    else
        tail_rank<4>(Key, n, F, Sym);
}

__device__ __forceinline__ void tables_tail(uint8_t* lds, const uint32_t* ac_hist, const uint32_t* dc_hist, int frame,
                                            const Geom& g, uint32_t* __restrict__ code_tab, uint8_t* __restrict__ out,
                                            size_t out_stride, uint32_t* __restrict__ hdr_len,
                                            const uint8_t* __restrict__ qtab_u8, int bits_per_channel,
                                            int* __restrict__ status, int* sCnt, int* sBits) {
    const int lane = lane_id(), tab = threadIdx.x >> 6;
    const bool ac = tab & 1;
    const int c = tab >> 1;
    const int cap = ac ? 256 : 16;
    uint8_t* const base = lds + kTailBase[tab];
    uint32_t* const F = reinterpret_cast<uint32_t*>(base);
    unsigned long long* const Key = reinterpret_cast<unsigned long long*>(F + cap);
    uint8_t* const Sym = reinterpret_cast<uint8_t*>(F + 3 * cap);
    int* const bits16 = sBits + 16 * tab;
    // a single-component frame has no chroma tables: waves 2 and 3 build nothing,
    // report nothing and leave their code-table rows alone
    const bool idle = g.ncomp == 1 && tab >= 2;  // (wave-uniform)
    int n = 0, dq = -1;
    if (idle) {
        if (lane == 0) sCnt[tab] = 0;
    } else {
        // ---- 1 (AC: symbols lane + 64 q; DC: symbol lane < 16 -- coalesced loads)
        uint32_t f[4] = {0u, 0u, 0u, 0u};
        if (ac) {
            const uint32_t* h = ac_hist + ((size_t)frame * kHistReps * 2 + c) * 256 + lane;
#pragma unroll
            for (int r = 0; r < kHistReps; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) f[q] += ld_agent(h + (size_t)r * 512 + 64 * q);
        } else if (lane < 16) {
            const uint32_t* h = dc_hist + (size_t)frame * kHistReps * 32 + c * 16 + lane;
#pragma unroll
            for (int r = 0; r < kHistReps; ++r) f[0] += ld_agent(h + (size_t)r * 32);
        }
        // table 0's wave: its lane's DQT bytes (zigzag position lane of both tables, kept
        // in zigzag order by the host), loaded with the histograms rather than after
        // the tables
        if (tab == 0 && g.stripe_first) dq = (int)qtab_u8[128 + lane] | ((int)qtab_u8[192 + lane] << 8);
        // keys (frequency << 8 | symbol): u32 while every frequency is below 2^24
        const bool k32 = __ballot(((f[0] | f[1] | f[2] | f[3]) >> 24) != 0u) == 0ull;
        uint32_t* const ct = code_tab + ((size_t)frame * 4 + tab) * 256;
        unsigned long long pres[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            pres[q] = __ballot(f[q] > 0u);
            if (f[q] == 0u) ct[lane + 64 * q] = 0;  // (a present symbol's entry: phase 5)
            n += __popcll(pres[q]);
        }
        // k_tables' checks: a table without symbols; symbol 0xFF in an AC table (the
        // reference's lookup table has 255 entries)
        raise_status(status, ((lane == 0 && n == 0) || (ac && lane == 63 && f[3] > 0u)) ? 2 : 0);  // (s 255: lane 63, q 3)
        if (lane == 0) sCnt[tab] = n;  // (read by every wave in phase 6, after the barrier)
        if (lane < 16) bits16[lane] = 0;

        // ---- 2: the present keys in ascending order (absent symbols: kMergeInf, last)
        // -> F (frequency), Sym by leaf rank
        if (k32) {
            if (ac && (!DMMT_TAIL_SORT2 || n > 128)) {
                uint32_t x[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = f[q] ? (f[q] << 8) | (uint32_t)(lane + 64 * q) : kMergeInf;
                sort_bitonic<4>(x);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (lane + 64 * q < n) {
                        F[lane + 64 * q] = x[q] >> 8;
                        Sym[lane + 64 * q] = (uint8_t)x[q];
                    }
            } else if (ac) {  // (uniform) at most 128 present symbols: compacted into two slots, half the network
                uint32_t* const K32 = reinterpret_cast<uint32_t*>(Key);
                int at = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (f[q]) K32[at + __popcll(pres[q] & ((1ull << lane) - 1ull))] = (f[q] << 8) | (uint32_t)(lane + 64 * q);
                    at += __popcll(pres[q]);
                }
                wave_lds_sync();
                uint32_t x[2] = {lane < n ? K32[lane] : kMergeInf, lane + 64 < n ? K32[lane + 64] : kMergeInf};
                sort_bitonic<2>(x);
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    if (lane + 64 * q < n) {
                        F[lane + 64 * q] = x[q] >> 8;
                        Sym[lane + 64 * q] = (uint8_t)x[q];
                    }
            } else {
                uint32_t x[1] = {f[0] ? (f[0] << 8) | (uint32_t)lane : kMergeInf};
                sort_bitonic<1>(x);
                if (lane < n) {
                    F[lane] = x[0] >> 8;
                    Sym[lane] = (uint8_t)x[0];
                }
            }
        } else {  // rank among 64-bit keys, compacted slot by slot (order immaterial: the keys carry their symbols)
            int at = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (f[q]) Key[at + __popcll(pres[q] & ((1ull << lane) - 1ull))] = ((unsigned long long)f[q] << 8) | (unsigned)(lane + 64 * q);
                at += __popcll(pres[q]);
            }
            wave_lds_sync();
            tail_rank_any(Key, n, F, Sym);
        }
        wave_lds_sync();

        // ---- 3, 4 (wave-uniform choice of the merge width)
        int leaf[kTailLevels];
        if (n <= 32)
            tail_levels<1>(F, n, leaf);
        else if (n <= 64)
            tail_levels<2>(F, n, leaf);
        else if (n <= 128)
            tail_levels<4>(F, n, leaf);
        else
            tail_levels<8>(F, n, leaf);

        uint32_t len[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = lane + 64 * r;
            len[r] = 0;
            if (i < n) {
                uint32_t L = i == 0 ? 1u : 0u;
#pragma unroll
                for (int k = 0; k < kTailLevels; ++k) L += i < leaf[k] ? 1u : 0u;
                len[r] = L;
                atomicAdd(&bits16[L - 1], 1);
            }
        }

        // ---- 5: code(rank i) = sum over the ranks above i of 2^(16 - len), mod 2^16
        {
            uint32_t carry = 0;
            uint32_t inc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t wgt = len[r] ? 1u << (16 - len[r]) : 0u;
                inc[r] = carry + wave_incl_scan_full_u32(wgt);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)inc[r], 63);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = lane + 64 * r;
                if (i < n) {
                    const uint32_t pat = (carry - inc[r]) & 0xFFFFu;  // left aligned u16 (wrapping as in the reference)
                    ct[Sym[i]] = (len[r] << 16) | (pat >> (16 - len[r]));
                }
            }
        }
    }
    __syncthreads();  // every table's count (sCnt); this wave's BITS
    if (idle) return;

    // ---- 6
    const int nt[4] = {sCnt[0], sCnt[1], sCnt[2], sCnt[3]};
    write_table_header(out + (size_t)frame * out_stride, tab, lane, 64, n, nt, Sym, bits16, g, qtab_u8,
                       bits_per_channel, hdr_len + frame, dq);
}

// ============================================================== operator: DCT only
// Discrete8x8CosineTransformer::transform over a block-contiguous f32 array
// (cosine_transform.rs:55-73, arai.rs:95-104); one lane per row, then column.
__global__ __launch_bounds__(256) void k_dct_blocks(float* __restrict__ data, long long nblocks) {
    __shared__ float s[32 * 65];
    const int tid = threadIdx.x;
    for (long long b0 = (long long)blockIdx.x * 32; b0 < nblocks; b0 += (long long)gridDim.x * 32) {
        const int nbk = (int)min(32LL, nblocks - b0);
        for (int i = tid; i < nbk * 64; i += 256) s[(i >> 6) * 65 + (i & 63)] = data[b0 * 64 + i];
        __syncthreads();
        {
            const int blk = tid >> 3, row = tid & 7;
            if (blk < nbk) {
                float v[8];
                for (int i = 0; i < 8; ++i) v[i] = s[blk * 65 + row * 8 + i];
                arai8(v);
                for (int i = 0; i < 8; ++i) s[blk * 65 + row * 8 + i] = v[i];
            }
        }
        __syncthreads();
        {
            const int blk = tid >> 3, col = tid & 7;
            if (blk < nbk) {
                float v[8];
                for (int i = 0; i < 8; ++i) v[i] = s[blk * 65 + i * 8 + col];
                arai8(v);
                for (int i = 0; i < 8; ++i) s[blk * 65 + i * 8 + col] = v[i];
            }
        }
        __syncthreads();
        for (int i = tid; i < nbk * 64; i += 256) data[b0 * 64 + i] = s[(i >> 6) * 65 + (i & 63)];
        __syncthreads();
    }
}

// ============================================================== synthetic input
// SURVEY.md 8(d) generator: base = (x + 8y) % 256 (dct_timing.rs:150-160),
// R = base, G = (base + 85 f + (y >> 3)) % 256, B = (255 - base + (x >> 4)) % 256,
// plus 4-bit xorshift32 noise per channel, clamped to 255.
__device__ __forceinline__ uint32_t xorshift32(uint32_t x) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
}

__global__ __launch_bounds__(256) void k_synthetic(uint8_t* __restrict__ rgb, int w, int h, int n_frames,
                                                   int first_frame, uint32_t seed, int row0, int rows) {
    const long long npx = (long long)w * h;       // the whole frame (the noise index)
    const long long nout = (long long)w * rows;   // rows [row0, row0 + rows) are generated
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nout * n_frames;
         i += (long long)gridDim.x * 256) {
        const int fl = (int)(i / nout);
        const long long pi = i - (long long)fl * nout + (long long)row0 * w;
        const int y = (int)(pi / w), x = (int)(pi - (long long)y * w);
        const uint32_t f = (uint32_t)(first_frame + fl);
        const uint32_t base = (uint32_t)(x + 8 * y) & 255u;
        const uint32_t n = xorshift32(seed ^ (uint32_t)(f * (uint32_t)npx + (uint32_t)pi));
        const uint32_t r = base + (n & 15u);
        const uint32_t g = ((base + 85u * f + ((uint32_t)y >> 3)) & 255u) + ((n >> 4) & 15u);
        const uint32_t b = ((255u - base + ((uint32_t)x >> 4)) & 255u) + ((n >> 8) & 15u);
        uint8_t* p = rgb + i * 3;
        p[0] = (uint8_t)min(r, 255u);
        p[1] = (uint8_t)min(g, 255u);
        p[2] = (uint8_t)min(b, 255u);
    }
}

// explicit instantiations of the front kernel

}  // namespace dmmt

// ============================================================== launchers
namespace dmmt {

#ifndef FRONT_WPE_420
#define FRONT_WPE_420 3
#endif

#ifndef FRONT_WPE_444
#define FRONT_WPE_444 5
#endif
#ifndef FRONT_WPE_422
#define FRONT_WPE_422 4
#endif

// Waves per SIMD k_front is compiled for (register budget 512 / WPE, in steps of 8).
// u8 4:4:4 fits 96 registers, so that two resident workgroups leave 320 of a SIMD's
// 512 to the other lanes' kernels, five waves of k_emit<8> ("what fits
// beside k_front").  The budget only binds where the kernel's LDS allows as many
// workgroups (five: at most 32,768 bytes): past that the compiler drops it and pads
// the allocation up to the occupancy the LDS leaves (RGBX 4:4:4, whose staged rows
// are a third longer).  u8 4:2:2 keeps its 4: it takes 73 to 81 registers and 27 KB,
// under either target as it is.  The rest keep the allocation the compiler picks.
template <int HR, int VR, typename S>
constexpr int front_wpe() {
    return sizeof(S) == 1 ? (HR * VR == 4 ? FRONT_WPE_420 : HR * VR == 2 ? FRONT_WPE_422 : FRONT_WPE_444) : 1;
}

// Resident workgroups per CU of a lone lane's launch (front_launch's MAX_PER_CU; 0: as
// many as fit).  The u8 4:4:4 kernels, the only ones whose occupancy rose with the
// compact sT, now fit five, but a lone lane keeps the four it had: a 4K frame's 4,050
// tiles split worse over 1,280 workgroups than over 1,024, and alone k_front_n took
// 28.3 us at five against 25.2 us at four (profiles/front_coresident_ab.txt, session
// 1).  The fifth slot is for the other lanes' kernels.
template <int HR, int VR, typename S>
constexpr int front_max_per_cu() {
    return sizeof(S) == 1 && HR * VR == 1 ? 4 : 0;
}

// (the launch and its resident grid: front_launch, front_with_sampling of
// front_launch.hpp; float samples have no narrow twin)

template <typename S>
static void front_sub(const void* rgb, size_t stride_elems, int n_frames, const Geom& g, const Work& w, hipStream_t st,
                      int per_cu_cap) {
    front_with_sampling(g, [&](auto hr, auto vr) {
        constexpr int HR = decltype(hr)::value, VR = decltype(vr)::value, WPE = front_wpe<HR, VR, S>();
        if constexpr (sizeof(S) == 4)
            front_launch<k_front<HR, VR, S, WPE>, nullptr>(g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi,
                                                           (const S*)rgb, stride_elems, g, w.norm_lut, w.qtab, w.coef,
                                                           w.status);
        else
            front_launch<k_front<HR, VR, S, WPE>, k_front_n<HR, VR, S, WPE>, front_max_per_cu<HR, VR, S>()>(
                g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, (const S*)rgb, stride_elems, g, w.norm_lut, w.qtab, w.coef,
                w.status);
    });
}

template <typename S, int LAY>
static void front_surf_sub(const SurfArgs& sa, size_t frame_stride, int n_frames, const Geom& g, const Work& w,
                           hipStream_t st, int per_cu_cap) {
    front_with_sampling(g, [&](auto hr, auto vr) {
        constexpr int HR = decltype(hr)::value, VR = decltype(vr)::value, WPE = front_wpe<HR, VR, S>();
        if constexpr (sizeof(S) == 4)
            front_launch<k_front_surf<HR, VR, S, LAY, WPE>, nullptr>(g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi,
                                                                     sa, frame_stride, g, w.norm_lut, w.qtab, w.coef,
                                                                     w.status);
        else
            front_launch<k_front_surf<HR, VR, S, LAY, WPE>, k_front_surf_n<HR, VR, S, LAY, WPE>, front_max_per_cu<HR, VR, S>()>(
                g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, sa, frame_stride, g, w.norm_lut, w.qtab, w.coef,
                w.status);
    });
}

// samples per pixel of a plane, 0: a (format, sample_bytes) pair outside the supported matrix
int surface_samples_per_pixel(int format, int sample_bytes) {
    const bool sb_ok = sample_bytes == 1 || sample_bytes == 2 || sample_bytes == 4;
    if (format == SURF_RGB || format == SURF_BGR) return sb_ok ? 3 : 0;
    if (format == SURF_RGBX || format == SURF_BGRX) return sample_bytes == 1 ? 4 : 0;
    if (format == SURF_PLANAR) return sample_bytes == 1 || sample_bytes == 4 ? 1 : 0;
    return 0;
}

hipError_t launch_front_surface(const Surface& sf, size_t frame_stride_bytes, int sample_bytes, int n_frames,
                                const Geom& g, const Work& w, hipStream_t st, int per_cu_cap) {
    const int spp = surface_samples_per_pixel(sf.format, sample_bytes);
    if (!spp) return hipErrorInvalidValue;
    SurfArgs sa{};
    for (int p = 0; p < 3; ++p) sa.plane[p] = (const uint8_t*)sf.plane[p];
    sa.pitch = (long long)sf.row_pitch;
    sa.span = (long long)(g.height - 1) * sa.pitch + (long long)g.width * spp * sample_bytes;
    sa.bgr = sf.format == SURF_BGR || sf.format == SURF_BGRX;
    if (sf.format == SURF_PLANAR) {
        if (sample_bytes == 1)
            front_surf_sub<uint8_t, LAY_PLANAR>(sa, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
        else
            front_surf_sub<float, LAY_PLANAR>(sa, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else if (spp == 4) {
        front_surf_sub<uint8_t, LAY_RGBX>(sa, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else if (sample_bytes == 1) {
        front_surf_sub<uint8_t, LAY_RGB>(sa, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else if (sample_bytes == 2) {
        front_surf_sub<uint16_t, LAY_RGB>(sa, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else {
        front_surf_sub<float, LAY_RGB>(sa, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    }
    return hipGetLastError();
}

hipError_t launch_front(const void* rgb, size_t frame_stride_bytes, int sample_bytes, int n_frames, const Geom& g,
                        const Work& w, hipStream_t st, int per_cu_cap) {
    const size_t se = frame_stride_bytes / (size_t)sample_bytes;
    if (sample_bytes == 4)
        front_sub<float>(rgb, se, n_frames, g, w, st, per_cu_cap);
    else if (sample_bytes == 1)
        front_sub<uint8_t>(rgb, se, n_frames, g, w, st, per_cu_cap);
    else
        front_sub<uint16_t>(rgb, se, n_frames, g, w, st, per_cu_cap);
    return hipGetLastError();
}

// The fused tail counts in 32 bits: a frame's symbols (at most 64 per block) times
// the 15 levels a package can sum over stay below 2^30 (a key weight << 1 | tag
// stays below its merge's padding); stripes keep k_tables
// (their histograms are summed on the host first)
#ifndef DMMT_HIST_WG_CAP
#define DMMT_HIST_WG_CAP 1024  // k_hist workgroups per launch (study builds: other caps)
#endif
bool tables_fusable(const Geom& g) { return g.stripe_first && !g.more_after && g.bpf * 64 * 16 < (1ll << 30); }

hipError_t launch_hist(int n_frames, const Geom& g, const Work& w, int check_cat, hipStream_t st, bool fuse_tables,
                       int bits_per_channel, uint8_t* out, size_t out_stride, int wg_cap) {
    // at most 1024 workgroups (4K: 1.5 blocks per thread): fewer histogram
    // flushes; 4K q90 bench 157.5 -> 159.6 Gpx/s, 8K 4:2:0 296.6 -> 299.0 against
    // one block per thread.  512 is faster pipelined still but k_hist alone +4 us,
    // so a context of several lanes passes wg_cap = DMMT_HIST_WG_CAP_LANES (512:
    // settled 4-lane bench +2.4 %, profiles/r06_hist_cap_lanes_ab.txt) and one lane
    // keeps the default
    dim3 grid(hist_grid_x(g.bpf, n_frames, wg_cap > 0 ? wg_cap : DMMT_HIST_WG_CAP), n_frames);
    const bool fuse = fuse_tables && tables_fusable(g);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, (const int16_t*)w.coef, w.dcdiff, w.lastnz, g, w.ac_hist,
                           w.dc_hist, w.status, w.arrive, w.code_tab, out, out_stride, w.hdr_len, w.qtab_u8,
                           bits_per_channel);
    };
    auto gon = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, (const int16_t*)w.coef, (const int16_t*)w.coef_lo,
                           (const int8_t*)w.coef_hi, w.dcdiff, w.lastnz, g, w.ac_hist, w.dc_hist, w.status, w.arrive,
                           w.code_tab, out, out_stride, w.hdr_len, w.qtab_u8, bits_per_channel);
    };
    if (w.coef_lo)  // the narrow form: integer samples only, so no -32768 test
        fuse ? gon(k_hist_n<false, true>) : gon(k_hist_n<false, false>);
    else if (check_cat)
        fuse ? go(k_hist<true, true>) : go(k_hist<true, false>);
    else
        fuse ? go(k_hist<false, true>) : go(k_hist<false, false>);
    return hipGetLastError();
}

hipError_t launch_tables(int n_frames, const Geom& g, const Work& w, int bits_per_channel, uint8_t* out,
                         size_t out_stride, hipStream_t st) {
    // (a single-component frame: the luma tables only; the chroma histograms are
    // empty, so every workgroup counts nt[2] = nt[3] = 0)
    hipLaunchKernelGGL(k_tables, dim3(g.ncomp == 1 ? 2 : 4, n_frames), dim3(512), 0, st, (const uint32_t*)w.ac_hist,
                       (const uint32_t*)w.dc_hist, w.code_tab, out, out_stride,
                       w.hdr_len, g, w.qtab_u8, bits_per_channel, w.status);
    return hipGetLastError();
}

hipError_t launch_dct_blocks(float* data, long long nblocks, hipStream_t st) {
    hipLaunchKernelGGL(k_dct_blocks, dim3(clampi((nblocks + 31) / 32, 1, 2048)), dim3(256), 0, st, data, nblocks);
    return hipGetLastError();
}

hipError_t launch_synthetic(uint8_t* rgb, int w, int h, int n_frames, int first_frame, uint32_t seed, int row0,
                            int rows, hipStream_t st) {
    const long long n = (long long)w * rows * n_frames;
    hipLaunchKernelGGL(k_synthetic, dim3(clampi((n + 255) / 256, 1, 8192)), dim3(256), 0, st, rgb, w, h, n_frames,
                       first_frame, seed, row0, rows);
    return hipGetLastError();
}

}  // namespace dmmt

#ifdef DMMT_PHASE_TRACE
// development builds only: copy out and clear this file's phase counters
extern "C" int dmmt_debug_trace_kernels(unsigned long long* out64) {
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(dmmt::g_trace), 64 * 8) != hipSuccess) return -1;
    unsigned long long z[64] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(dmmt::g_trace), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
