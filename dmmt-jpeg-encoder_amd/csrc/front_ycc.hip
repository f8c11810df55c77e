// front_ycc.hip -- k_front_ycc, k_front_ycc_lv: the front kernels for frames that
// already are YCbCr (dmmt_encode_device_ycc, _levels, _matrix): planar I444 / I422 /
// I420 and semi-planar NV24 / NV16 / NV12 (and their Cr,Cb twins).  One body,
// front_ycc_body, serves three kinds of input, told apart by the argument struct
// (Args::IN):
//   plain   (YccArgs, k_front_ycc)       uint8 samples, JFIF full range;
//   levels  (YccLvArgs, k_front_ycc_lv)  limited ("video") range, and 8 to 16
//           significant bits in a uint16 -- P010 / P012 / P016 (the bits at the top,
//           `shift` unused low bits) and I010 / yuv420p10le (the bits at the bottom);
//   matrix  (YccMxArgs, k_front_ycc_lv)  any levels, planes that carry the BT.709 or
//           the BT.2020 (non-constant luminance) matrix.
//
// The reference has no such input (Image<f32> is always RGB); the contract is
// stated in its stages.  What enters the DCT lies in [-128, 127], the value range
// color.rs:75-100 produces for the level-shifted Y and for Cb and Cr, in f32, every
// operation rounded once (-ffp-contract=off, the Makefile's HIPFLAGS, the host side
// too) and never rounded to 8 bits:
//   plain   (float)s - 128 of the sample s;
//   levels  of the code v = s >> shift, with the four constants of
//           ycc_levels_transfer:
//             luma    y  = min(max(((float)v - offY) * kY, 0), 255) - 128
//             chroma  cb = min(max(((float)v - offC) * kC, -128), 127), cr alike
//   matrix  of those y, cb, cr, with the six constants of ycc_matrix_coefficients,
//           in this order: the step to the BT.601 matrix a JFIF file is decoded with
//             Y'  = min(max((y + a*cb) + b*cr, -128), 127)
//             Cb' = min(max(c*cb + d*cr, -128), 127)
//             Cr' = min(max(e*cb + f*cr, -128), 127)
//           A luma sample takes the chroma position that shares its MCU cell,
//           (x / HR, y / VR); chroma is neither interpolated nor re-sited.
// JFIF planes never take the matrix step: it is not exactly the identity for 601 in
// f32, so those frames stay plain or levels.  And uint8 full range stays plain:
// its instantiations unpack no shift and carry no transfer constants.
//
// The chroma planes are taken as they lie, ceil(W / HR) x ceil(H / VR), never
// resampled or averaged (planes finer than the file: front_ycc_sub.hip).  The padding is padder.rs:12-42's black in YCbCr up to the
// MCU multiple, luma -128 and chroma 0: the loader (ycc_load.hpp) stages the
// samples that become just that past the rectangle -- plain 0 and 0x80, levels and
// matrix the codes offY << shift and offC << shift, which transfer to y = -128 and
// cb = cr = 0, and the 2x2 keeps 0 -- and the matrix kind sets luma to -128 outside
// the rectangle itself, whatever chroma shares the cell.  From there on k_front's
// path: arai.rs:29-104 rows then columns, quantizer.rs:53-62 with the luma table for
// Y and the chroma table for Cb and Cr, block_entangler.rs:69-77's emission order,
// and the same coefficient layout in HBM, so k_hist and every kernel after it run
// unchanged.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dct_quant.hpp"
#include "device_common.hpp"
#include "front_common.hpp"
#include "front_launch.hpp"
#include "front_ycc_common.hpp"
#include "jpeg_common.hpp"
#include "kernels.hpp"
#include "ycc_load.hpp"

namespace dmmt {

// (The argument structs, YccArgs / YccLvArgs / YccMxArgs, and the transfer functions:
// front_ycc_common.hpp, shared with front_ycc_sub.hip.)

// One workgroup (256 threads) per tile = TM horizontally adjacent MCUs of one MCU
// row (256 luma columns, 8 * VR luma rows), a grid-stride loop over the frame's
// tiles (blockIdx.y = frame) with the next tile's bytes prefetched into registers
// while this one computes -- k_front's shape, from the same pieces
// (front_common.hpp): FrontGeom's LDS layout of the row-transformed blocks (sT,
// front_store_row), front_stage, and front_column_pass with its emission-order index, so
// the coefficients land where k_front puts them.
//  staging  YccTile<.., SB> / ycc_tile_chunk (ycc_load.hpp): 8 * VR luma tile rows
//     and 8 chroma tile rows per chroma plane, each at its own pitch and
//     misalignment, SB bytes per sample.  A uint16 luma tile row is 512 bytes, 33
//     chunks; the largest tile (4:2:0 NV and 4:4:4, uint16) is 792 chunks, four per
//     thread.  The plain kind takes the loader's default pad samples.
//  A  one thread per (chroma row r, chroma block c, luma block column h).  A row's
//     words come from LDS, funnel-shifted; uint8: a byte each (v_cvt_f32_ubyteN);
//     uint16: twice the words -- the misalignment is even -- a half each, shifted
//     right by `shift` (the low bits never count).  NV: a row of pairs,
//     de-interleaved while unpacking (uint16: a pair is one word); VU (Cr first) is a
//     template parameter.
//     plain, levels: the thread's VR luma rows of 8 samples -- transfer, row pass --
//     and a chroma row pass of 8 samples: both components with 4:4:4; with 4:2:x
//     thread h = 0 takes the block's Cb row and h = 1 its Cr row.  (k_front's pair
//     exchanges four averaged samples over DPP because each thread had computed half
//     of both rows; here the samples are in LDS and each thread reads the row it
//     transforms.)
//     matrix: the thread reads BOTH components of chroma row r's 8 positions of
//     chroma block c -- planar: the row's words of each plane, NV: the pair is in
//     the word it read already -- and transfers them to cb[8], cr[8].  Its chroma row
//     pass: Cb' and Cr' with 4:4:4; with 4:2:x thread h = 0 mixes Cb' and h = 1 Cr'
//     (the same two products and one sum, the pair of constants chosen by h).  Then
//     its VR luma rows: transferred, Y' with chroma position (8h + k) / HR of the
//     block, and -128 at or past width - x0 / height - y0.
//  range vote  where a code can exceed 2^B - 1 (uint16 with shift < 16 - B:
//     wave-uniform), the largest code the thread unpacked is compared with it:
//     status bit 1, raised once per wave after the tile loop.  Only samples of the
//     rectangle and pad codes are unpacked (matrix: both components of the thread's
//     positions).  uint8 instantiations compile no status code: no sample can
//     exceed a maxval.
//  C, D  front_column_pass, k_front's integer-sample path.  Its bound
//     (dct_quant.hpp's integer-sample argument, quantize_col8_scaled) needs the
//     DCT's inputs in [-128, 127] only -- k_front feeds it the f32 YCbCr of RGB
//     pixels.  plain: integers in that range; levels: the transfer's clamps end in
//     it; matrix: ycc_clamp, and -128 outside.  So |DC| = |sum| / 8 <= 1024,
//     |AC| <= (1/4) * 64 * 128 = 2048, to within a few ulps, and with q >= 1
//     `as i16` cannot saturate; no NaN can arise (nan_possible = false).
// WPE: see front_ycc_wpe below.
// NARROW: the 80-byte block form (coef_format.hpp), as front_body's.
template <int HR, int VR, int FMT, int SB, bool NARROW, class Args>
__device__ __forceinline__ void front_ycc_body(const Args& ya, size_t frame_stride, const Geom& g,
                                               const float* __restrict__ qtab,  // [2][64] natural, as f32
                                               int16_t* __restrict__ coef, int* __restrict__ status,
                                               int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    constexpr int IN = Args::IN;
    static_assert(IN != YCC_IN_PLAIN || SB == 1, "plain frames are uint8");
    constexpr bool NV = FMT != YCC_PLANAR;
    constexpr int VU = FMT == YCC_NV_VU ? 1 : 0;
    using T = YccTile<HR, VR, NV, SB>;
    // the tile's blocks (front_layout.hpp); u8 4:4:4 takes sT without padding, as k_front
    using G = FrontGeom<HR, VR, 3, SB == 1 && HR * VR == 1>;
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
    // the kind's constants, copied here whatever phase A reads them: where they are
    // copied (and that each row pass below is written out, not a shared lambda)
    // decides the order of the generated code, not its amount
    YccTransfer t{};                          // (plain: not read)
    YccMatrix m{};                            // (matrix kind only)
    uint32_t shift = 0u, max_code = 0xFFFFu;  // (uint8: neither is read)
    if constexpr (IN != YCC_IN_PLAIN) t = ya.t;
    if constexpr (IN == YCC_IN_MATRIX) m = ya.m;
    if constexpr (SB == 2) shift = ya.c.shift, max_code = ya.c.max_code;
    const bool check_range = SB == 2 && (0xFFFFu >> shift) > max_code;  // (uniform)
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
            if (q < T::NCHUNK) {
                if constexpr (IN == YCC_IN_PLAIN)
                    ycc_tile_chunk<T>(ms, d, tx0, ty0, interior, q, w);
                else
                    ycc_tile_chunk<T>(ms, d, tx0, ty0, interior, q, w, ya.c.luma_fill, ya.c.chroma_fill);
            }
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
        // ---- A: code -> full-range value[, the matrix], level shift, row pass (arai.rs:97-99)
        if constexpr (IN != YCC_IN_MATRIX) {
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
                    v[k] = ycc_luma_in<IN>(s, t);
                }
                arai8(v);
                front_store_row<G>(sT, (ly >> 3) * 32 + c * HR + h, (ly & 7), v);
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
                        v[k] = ycc_chroma_in<IN>(s, t);
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
                        v[k] = ycc_chroma_in<IN>(s, t);
                    }
                }
                arai8(v);
                front_store_row<G>(sT, NYB + comp * CB + c, r, v);
            }
        }
        if constexpr (IN == YCC_IN_MATRIX) {
            const int h = tid % SP, job = tid / SP;
            const int c = job % CB, r = job / CB;  // chroma block, chroma row
            const int lx0 = c * 8 * HR + 8 * h;    // first luma column of the job
            const int cx0 = x0 / HR, cy = y0 / VR + r;
            // position k of the block's chroma row, transferred: (cb, cr)
            uint32_t wb[(NV ? 4 : 2) * SB], wr[NV ? 1 : 2 * SB];  // (NV: the pairs in wb, wr unused)
            if constexpr (NV) {
                const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p1, (uint32_t)d.chroma_pitch, 2 * SB, cx0, cy);
                lds_words<4 * SB>(sRaw, T::chroma_row(0, r) + mis + 16 * SB * c, wb);
            } else {
                const int mb = surf_misalign32((uint32_t)(uintptr_t)ms.p1, (uint32_t)d.chroma_pitch, SB, cx0, cy);
                const int mr = surf_misalign32((uint32_t)(uintptr_t)ms.p2, (uint32_t)d.chroma_pitch, SB, cx0, cy);
                lds_words<2 * SB>(sRaw, T::chroma_row(0, r) + mb + 8 * SB * c, wb);
                lds_words<2 * SB>(sRaw, T::chroma_row(1, r) + mr + 8 * SB * c, wr);
            }
            auto pair_at = [&](int k, float& b, float& rr) {
                uint32_t s0, s1;  // Cb's and Cr's code
                if constexpr (!NV) {
                    s0 = code(wb, k), s1 = code(wr, k);
                } else if constexpr (SB == 1) {
                    const uint32_t p = wb[k >> 1] >> (16 * (k & 1));
                    s0 = (p >> (8 * VU)) & 0xFFu, s1 = (p >> (8 * (1 - VU))) & 0xFFu;
                } else {  // a pair is one word
                    s0 = ((wb[k] >> (16 * VU)) & 0xFFFFu) >> shift, s1 = ((wb[k] >> (16 * (1 - VU))) & 0xFFFFu) >> shift;
                }
                if constexpr (SB == 2) vmax = max(vmax, max(s0, s1));
                b = ycc_chroma_in<IN>(s0, t), rr = ycc_chroma_in<IN>(s1, t);
            };
            // cb, cr: the row's 8 positions; lb, lr: the 8 / HR positions under this thread's
            // luma columns, (8h + k) / HR.  (With HR = 2 they are chosen from values, position j
            // or 4 + j as h says: choosing between two elements of cb would index the array.)
            float cb[8], cr[8], lb[8 / HR], lr[8 / HR];
            if constexpr (HR == 1) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    pair_at(k, cb[k], cr[k]);
                    lb[k] = cb[k], lr[k] = cr[k];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float b0, r0, b1, r1;
                    pair_at(j, b0, r0);
                    pair_at(4 + j, b1, r1);
                    cb[j] = b0, cr[j] = r0, cb[4 + j] = b1, cr[4 + j] = r1;
                    lb[j] = h ? b1 : b0, lr[j] = h ? r1 : r0;
                }
            }
            // (the chroma row pass first: cb and cr are dead when the luma rows start)
#pragma unroll
            for (int pass = 0; pass < (SP == 1 ? 2 : 1); ++pass) {
                const int comp = SP == 1 ? pass : h;  // 0: Cb', 1: Cr'
                const float m0 = comp ? m.e : m.c, m1 = comp ? m.f : m.d;
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = ycc_clamp(m0 * cb[k] + m1 * cr[k]);
                arai8(v);
                front_store_row<G>(sT, NYB + comp * CB + c, r, v);
            }
            const int nx = d.width - x0 - lx0;  // the job's luma columns inside the rectangle (<= 0: none)
#pragma unroll
            for (int dy = 0; dy < VR; ++dy) {
                const int ly = r * VR + dy;
                const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p0, (uint32_t)d.luma_pitch, SB, x0, y0 + ly);
                uint32_t w[2 * SB];
                lds_words<2 * SB>(sRaw, T::luma_row(ly) + mis + SB * lx0, w);
                const int nk = y0 + ly < d.height ? nx : 0;  // samples k < nk lie inside
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t s = code(w, k);
                    if constexpr (SB == 2) vmax = max(vmax, s);
                    const float yy = ycc_clamp((ycc_luma_in<IN>(s, t) + m.a * lb[k / HR]) + m.b * lr[k / HR]);
                    v[k] = k < nk ? yy : -128.0f;
                }
                arai8(v);
                front_store_row<G>(sT, (ly >> 3) * 32 + c * HR + h, (ly & 7), v);
            }
        }
        __syncthreads();
        front_column_pass<G, NARROW, false>(sT, sQ, sRQ, tid, false, g, frame, mx0, my, coef, coef_lo, coef_hi);
    }
    if constexpr (SB == 2) {
        // a code above 2^B - 1 (color.rs:63-65's panic): one vote per wave, its leader stores
        const bool bad = check_range && vmax > max_code;
        if (__ballot(bad)) raise_status(status, bad ? 1 : 0);
    }
}

template <int HR, int VR, int FMT, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc(YccArgs ya, size_t frame_stride, Geom g,
                                                       const float* __restrict__ qtab, int16_t* __restrict__ coef) {
    front_ycc_body<HR, VR, FMT, 1, false>(ya, frame_stride, g, qtab, coef, nullptr, nullptr, nullptr);
}
template <int HR, int VR, int FMT, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_n(YccArgs ya, size_t frame_stride, Geom g,
                                                         const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                         int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    front_ycc_body<HR, VR, FMT, 1, true>(ya, frame_stride, g, qtab, coef, nullptr, coef_lo, coef_hi);
}
// The kinds with levels, YccLvArgs and YccMxArgs: they can raise a status.  (The
// plain pair above keeps its own argument list: one more argument, used or not,
// moves the hidden arguments behind it and so every plain kernel's code.)
template <class Args, int HR, int VR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_lv(Args ya, size_t frame_stride, Geom g,
                                                          const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                          int* __restrict__ status) {
    front_ycc_body<HR, VR, FMT, SB, false>(ya, frame_stride, g, qtab, coef, status, nullptr, nullptr);
}
template <class Args, int HR, int VR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_lv_n(Args ya, size_t frame_stride, Geom g,
                                                            const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                            int* __restrict__ status, int16_t* __restrict__ coef_lo,
                                                            int8_t* __restrict__ coef_hi) {
    front_ycc_body<HR, VR, FMT, SB, true>(ya, frame_stride, g, qtab, coef, status, coef_lo, coef_hi);
}

// ============================================================== host helpers

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

// Source Kr, Kb (Kg = 1 - Kr - Kb) to the target Kr' = 0.299, Kb' = 0.114: with
// R = Y + 2(1-Kr) Cr, B = Y + 2(1-Kb) Cb and G from Y = Kr R + Kg G + Kb B, the
// target luma is Y + a Cb + b Cr and the target chroma (B - Y') / (2(1-Kb')),
// (R - Y') / (2(1-Kr')).  In double precision, each constant rounded once to f32.
bool ycc_matrix_coefficients(int matrix, YccMatrix* out) {
    double kr, kb;
    if (matrix == YCC_MATRIX_BT709)
        kr = 0.2126, kb = 0.0722;
    else if (matrix == YCC_MATRIX_BT2020)
        kr = 0.2627, kb = 0.0593;
    else
        return false;
    const double kg = 1.0 - kr - kb;
    const double tr = 0.299, tb = 0.114, tg = 0.587;
    const double ub = 2.0 * (1.0 - kb), ur = 2.0 * (1.0 - kr);  // B - Y per Cb, R - Y per Cr
    const double a = tb * ub - tg * (kb * ub / kg);
    const double b = tr * ur - tg * (kr * ur / kg);
    const double nb = 2.0 * (1.0 - tb), nr = 2.0 * (1.0 - tr);
    out->a = (float)a;
    out->b = (float)b;
    out->c = (float)((ub - a) / nb);
    out->d = (float)(-b / nb);
    out->e = (float)(-a / nr);
    out->f = (float)((ur - b) / nr);
    return true;
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
size_t ycc_plane_span(int format, int plane, int width, int height, int hr, int vr, size_t luma_pitch,
                      size_t chroma_pitch) {
    return ycc_plane_span_levels(format, plane, width, height, hr, vr, luma_pitch, chroma_pitch, 1);  // uint8
}

// ============================================================== launcher

// Waves per SIMD the kernel is compiled for (register budget 512 / WPE).  uint8
// tiles fit 4 with room: without a bound the compiler allocates 70 to 72 VGPRs for
// 4:2:2, 81 to 82 for 4:4:4 and 93 to 95 for 4:2:0 of the plain kind, no scratch
// (-Rpass-analysis=kernel-resource-usage), and 24 KiB (4:2:2) or 35 KiB of LDS: at
// least four resident workgroups per CU, as k_front's u8 4:4:4 and 4:2:2.  uint16
// tiles stage twice the bytes: 27 KiB of LDS with 4:2:2 -- 4 again: 104 to 113
// registers, so four workgroups per CU although the LDS would hold five -- and 41 KiB
// with 4:4:4 and 4:2:0, where three workgroups fit a CU's 160 KiB whatever the
// registers: 3, a budget of 168.  DESIGN.md sections 13 and 14 list what each
// instantiation takes; none spills.  uint8 4:4:4, as k_front's: sT without padding,
// 32 KiB of LDS, and a budget of 5 (96 registers) that leaves two resident workgroups'
// neighbours a fifth k_emit workgroup; a lone lane's launch stays at
// four workgroups per CU (front_ycc_max_per_cu).
template <int HR, int VR, int SB>
constexpr int front_ycc_wpe() {
    return SB == 1 && HR * VR == 1 ? 5 : SB == 2 && !(HR == 2 && VR == 1) ? 3 : 4;
}
template <int HR, int VR, int SB>
constexpr int front_ycc_max_per_cu() {
    return SB == 1 && HR * VR == 1 ? 4 : 0;
}

// the instantiation for (format, sb, g's sampling): the plain kind has uint8 ones only
template <class Args>
static void front_ycc_dispatch(const Args& ya, int format, int sb, size_t frame_stride, int n_frames, const Geom& g,
                               const Work& w, hipStream_t st, int per_cu_cap) {
    auto launch = [&](auto fmt, auto sbc) {
        front_with_sampling(g, [&](auto hr, auto vr) {
            constexpr int FMT = decltype(fmt)::value, SB = decltype(sbc)::value;
            constexpr int HR = decltype(hr)::value, VR = decltype(vr)::value, WPE = front_ycc_wpe<HR, VR, SB>();
            if constexpr (Args::IN == YCC_IN_PLAIN)
                front_launch<k_front_ycc<HR, VR, FMT, WPE>, k_front_ycc_n<HR, VR, FMT, WPE>, front_ycc_max_per_cu<HR, VR, SB>()>(
                    g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ya, frame_stride, g, w.qtab, w.coef);
            else
                front_launch<k_front_ycc_lv<Args, HR, VR, FMT, SB, WPE>, k_front_ycc_lv_n<Args, HR, VR, FMT, SB, WPE>,
                             front_ycc_max_per_cu<HR, VR, SB>()>(
                    g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ya, frame_stride, g, w.qtab, w.coef, w.status);
        });
    };
    auto with_sb = [&](auto fmt) {
        if constexpr (Args::IN != YCC_IN_PLAIN) {
            if (sb == 2) return launch(fmt, std::integral_constant<int, 2>{});
        }
        launch(fmt, std::integral_constant<int, 1>{});
    };
    if (format == YCC_PLANAR)
        with_sb(std::integral_constant<int, YCC_PLANAR>{});
    else if (format == YCC_NV)
        with_sb(std::integral_constant<int, YCC_NV>{});
    else
        with_sb(std::integral_constant<int, YCC_NV_VU>{});
}

hipError_t launch_front_ycc(const YccFrames& yf, const YccLevels* lv, const YccMatrix* mx, size_t frame_stride_bytes,
                            int n_frames, const Geom& g, const Work& w, hipStream_t st, int per_cu_cap) {
    if (yf.format < YCC_PLANAR || yf.format > YCC_NV_VU || (lv && !ycc_levels_valid(*lv)) || (mx && !lv))
        return hipErrorInvalidValue;
    if (yf.src_hr)  // planes at a finer sampling than the file's: front_ycc_sub.hip
        return launch_front_ycc_sub(yf, lv, mx, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    const int sb = lv ? lv->sample_bytes : 1;
    if (mx) {
        YccMxArgs ya = ycc_args<YccMxArgs>(yf, lv, g, g.hr, g.vr);
        ya.m = *mx;
        front_ycc_dispatch(ya, yf.format, sb, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else if (lv) {
        front_ycc_dispatch(ycc_args<YccLvArgs>(yf, lv, g, g.hr, g.vr), yf.format, sb, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else {
        front_ycc_dispatch(ycc_args<YccArgs>(yf, nullptr, g, g.hr, g.vr), yf.format, sb, frame_stride_bytes, n_frames, g, w, st,
                           per_cu_cap);
    }
    return hipGetLastError();
}

}  // namespace dmmt
