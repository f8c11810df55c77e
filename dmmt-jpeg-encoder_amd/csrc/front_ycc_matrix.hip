// front_ycc_matrix.hip -- k_front_ycc_mx: the front kernel for YCbCr frames whose
// planes carry the BT.709 or the BT.2020 (non-constant luminance) matrix
// (dmmt_encode_device_ycc_matrix): k_front_ycc_lv (front_ycc_levels.hip) with one
// step after the transfer, which takes the three values to the BT.601 matrix a JFIF
// file is decoded with.
//
// With y, cb, cr the values k_front_ycc_lv feeds the DCT (level-shifted, clamped,
// [-128, 127]) and the six constants of ycc_matrix_coefficients, in f32, every
// operation rounded once (-ffp-contract=off, the Makefile's HIPFLAGS), in this order:
//   Y'  = min(max((y + a*cb) + b*cr, -128), 127)
//   Cb' = min(max(c*cb + d*cr, -128), 127)
//   Cr' = min(max(e*cb + f*cr, -128), 127)
// A luma sample takes the chroma position that shares its MCU cell, (x / HR, y / VR);
// chroma is neither interpolated nor re-sited.  The padding is black after the
// matrix: luma -128 outside the rectangle whatever chroma shares the cell, chroma 0
// (the loader's pad codes transfer to cb = cr = 0, which the 2x2 keeps).  The loader,
// the LDS layout, the prefetch, the column pass and the range vote are
// k_front_ycc_lv's.  The JFIF matrix never comes here: the step is not exactly the
// identity for 601 in f32, and those frames keep their kernels (front_ycc.hip,
// front_ycc_levels.hip).
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

// the planes of frame 0 (three pointers as values: an indexed read of a kernel
// argument would put it into scratch), their description, the sample levels and
// the matrix
struct YccMxArgs {
    const uint8_t *p0, *p1, *p2;  // Y; Cb or the pairs; Cr (planar only)
    YccDesc d;
    YccTransfer t;
    YccMatrix m;
    uint32_t luma_fill, chroma_fill;  // the pad codes << shift, in every sample of a word
    uint32_t shift;                   // unused low bits of a uint16 sample
    uint32_t max_code;                // 2^B - 1
};
struct YccMxMems {
    const uint8_t *p0, *p1, *p2;
    __device__ __forceinline__ PlaneMem plane(int p) const { return PlaneMem{p == 0 ? p0 : (p == 1 ? p1 : p2)}; }
};

// k_front_ycc_lv's transfer (front_ycc_levels.hip)
__device__ __forceinline__ float ycc_mx_luma_in(uint32_t v, const YccTransfer& t) {
    return fminf(fmaxf(((float)v - t.off_y) * t.k_y, 0.0f), 255.0f) - 128.0f;
}
__device__ __forceinline__ float ycc_mx_chroma_in(uint32_t v, const YccTransfer& t) {
    return fminf(fmaxf(((float)v - t.off_c) * t.k_c, -128.0f), 127.0f);
}
__device__ __forceinline__ float ycc_mx_clamp(float v) { return fminf(fmaxf(v, -128.0f), 127.0f); }

// front_ycc_lv_body (front_ycc_levels.hip) with another phase A:
//  A  thread (h, c, r) reads BOTH components of chroma row r's 8 positions of chroma
//     block c -- planar: the row's words of each plane, NV: the pair is in the word
//     it read already -- and transfers them to cb[8], cr[8].  Its chroma row pass:
//     Cb' and Cr' with 4:4:4; with 4:2:x thread h = 0 mixes Cb' and h = 1 Cr' (the
//     same two products and one sum, the pair of constants chosen by h).  Then its
//     VR luma rows of 8 samples: transferred, Y' with chroma position (8h + k) / HR
//     of the block, and -128 at or past width - x0 / height - y0.
//     The range vote counts every code the thread unpacked, as before: both
//     components of its positions now, which lie inside the rectangle or are pad
//     codes like its own.
template <int HR, int VR, int FMT, int SB, bool NARROW>
__device__ __forceinline__ void front_ycc_mx_body(const YccMxArgs& ya, size_t frame_stride, const Geom& g,
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
    const YccMxMems ms{ya.p0 + foff, ya.p1 + foff, ya.p2 + foff};  // (NV: p2 = p1)
    const YccDesc& d = ya.d;
    const YccTransfer t = ya.t;
    const YccMatrix m = ya.m;
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
        // ---- A: code -> full-range value, the matrix, level shift, row pass (arai.rs:97-99)
        {
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
                b = ycc_mx_chroma_in(s0, t), rr = ycc_mx_chroma_in(s1, t);
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
                for (int k = 0; k < 8; ++k) v[k] = ycc_mx_clamp(m0 * cb[k] + m1 * cr[k]);
                arai8(v);
                float4* o = reinterpret_cast<float4*>(sT + G::blk_base(NYB + comp * CB + c) + r * 8);
                o[0] = make_float4(v[0], v[1], v[2], v[3]);
                o[1] = make_float4(v[4], v[5], v[6], v[7]);
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
                    const float y = ycc_mx_luma_in(s, t);
                    const float yy = ycc_mx_clamp((y + m.a * lb[k / HR]) + m.b * lr[k / HR]);
                    v[k] = k < nk ? yy : -128.0f;
                }
                arai8(v);
                float4* o = reinterpret_cast<float4*>(sT + G::blk_base((ly >> 3) * 32 + c * HR + h) + (ly & 7) * 8);
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
__global__ __launch_bounds__(256, WPE) void k_front_ycc_mx(YccMxArgs ya, size_t frame_stride, Geom g,
                                                          const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                          int* __restrict__ status) {
    front_ycc_mx_body<HR, VR, FMT, SB, false>(ya, frame_stride, g, qtab, coef, status, nullptr, nullptr);
}
template <int HR, int VR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_mx_n(YccMxArgs ya, size_t frame_stride, Geom g,
                                                            const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                            int* __restrict__ status, int16_t* __restrict__ coef_lo,
                                                            int8_t* __restrict__ coef_hi) {
    front_ycc_mx_body<HR, VR, FMT, SB, true>(ya, frame_stride, g, qtab, coef, status, coef_lo, coef_hi);
}

// ============================================================== launcher

// Waves per SIMD the kernel is compiled for (register budget 512 / WPE): the levels
// kernel's bounds (front_ycc_lv_wpe, front_ycc_levels.hip).  DESIGN.md section 14
// lists what each instantiation takes; none spills.
template <int HR, int VR, int SB>
constexpr int front_ycc_mx_wpe() {
    return SB == 2 && !(HR == 2 && VR == 1) ? 3 : 4;
}

template <int FMT, int SB>
static void front_ycc_mx_sub(const YccMxArgs& ya, size_t frame_stride, int n_frames, const Geom& g, const Work& w,
                             hipStream_t st, int per_cu_cap) {
    front_with_sampling(g, [&](auto hr, auto vr) {
        constexpr int HR = decltype(hr)::value, VR = decltype(vr)::value, WPE = front_ycc_mx_wpe<HR, VR, SB>();
        front_launch<k_front_ycc_mx<HR, VR, FMT, SB, WPE>, k_front_ycc_mx_n<HR, VR, FMT, SB, WPE>>(
            g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ya, frame_stride, g, w.qtab, w.coef, w.status);
    });
}
template <int SB>
static void front_ycc_mx_fmt(int format, const YccMxArgs& ya, size_t frame_stride, int n_frames, const Geom& g,
                             const Work& w, hipStream_t st, int per_cu_cap) {
    if (format == YCC_PLANAR)
        front_ycc_mx_sub<YCC_PLANAR, SB>(ya, frame_stride, n_frames, g, w, st, per_cu_cap);
    else if (format == YCC_NV)
        front_ycc_mx_sub<YCC_NV, SB>(ya, frame_stride, n_frames, g, w, st, per_cu_cap);
    else
        front_ycc_mx_sub<YCC_NV_VU, SB>(ya, frame_stride, n_frames, g, w, st, per_cu_cap);
}

hipError_t launch_front_ycc_matrix(const YccFrames& yf, const YccLevels& lv, const YccMatrix& mx,
                                   size_t frame_stride_bytes, int n_frames, const Geom& g, const Work& w,
                                   hipStream_t st, int per_cu_cap) {
    if (yf.format < YCC_PLANAR || yf.format > YCC_NV_VU || !ycc_levels_valid(lv)) return hipErrorInvalidValue;
    const int sb = lv.sample_bytes;
    YccMxArgs ya{};
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
    ya.m = mx;
    // the pad codes: offY and offC are integers below 2^B, so << shift stays inside 16 (8) bits
    const uint32_t py = (uint32_t)ya.t.off_y << lv.shift, pc = (uint32_t)ya.t.off_c << lv.shift;
    ya.luma_fill = sb == 1 ? py * 0x01010101u : py * 0x00010001u;
    ya.chroma_fill = sb == 1 ? pc * 0x01010101u : pc * 0x00010001u;
    ya.shift = (uint32_t)lv.shift;
    ya.max_code = (1u << lv.bit_depth) - 1u;
    if (sb == 1)
        front_ycc_mx_fmt<1>(yf.format, ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    else
        front_ycc_mx_fmt<2>(yf.format, ya, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    return hipGetLastError();
}

}  // namespace dmmt
