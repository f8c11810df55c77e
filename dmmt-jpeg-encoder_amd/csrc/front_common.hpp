// front_common.hpp -- the device code the front kernels share (kernels.hip:
// k_front, k_front_surf; front_ycc.hip: k_front_ycc; front_ycc_sub.hip: k_front_ycc_sub;
// front_gray.hip: k_front_gray,
// and their narrow twins): the tile's block geometry, the plane accessor of the
// chunk loaders, the staging copy, the quantiser tables' LDS fill, the column pass
// with the blocks' store.  What differs between the kernels -- how a tile's bytes
// are fetched and phase A, the samples' way to the row-transformed blocks -- stays
// in their own files, and so does the tile loop that calls both: each kernel body
// writes out the same loop (as a function taking the two as callables it cost three
// of the budgeted instantiations registers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coef_format.hpp"
#include "dct_quant.hpp"
#include "device_common.hpp"
#include "jpeg_common.hpp"

namespace dmmt {

// A tile: 256 padded pixel columns by 8 * VR rows = TM horizontally adjacent MCUs
// of one MCU row.  In LDS its row-transformed blocks (sT) lie block-major: the Y
// blocks first, 32 columns x VR rows, then the Cb and the Cr blocks (NCOMP 3).
// NCOMP 1: a grayscale frame, HR = VR = 1, an MCU is one Y block.
template <int HR_, int VR_, int NCOMP_ = 3>
struct FrontGeom {
    static_assert(NCOMP_ == 3 || (NCOMP_ == 1 && HR_ == 1 && VR_ == 1), "gray: one block per MCU");
    static constexpr int HR = HR_, VR = VR_, NCOMP = NCOMP_;
    static constexpr int TM = 32 / HR;            // MCUs per tile
    static constexpr int ROWS = 8 * VR;           // pixel rows per tile
    static constexpr int NLUMA = HR * VR;
    static constexpr int BPM = NLUMA + NCOMP - 1; // blocks per MCU
    static constexpr int NB = TM * BPM;           // blocks per tile
    static constexpr int NYB = 32 * VR;           // Y blocks: 32 columns x VR rows
    static constexpr int CB = NCOMP == 1 ? 0 : TM;  // chroma blocks per component
    static constexpr int NQT = NCOMP == 1 ? 1 : 2;  // quantiser tables: luma[, chroma]
    static constexpr int BS = 72;                 // LDS floats per block: 64 + pad (conflict-free column reads)
    static constexpr int ST_FLOATS = NB * BS + 4;  // sT
    static constexpr int JPT = NB * 8 / 256;      // column jobs (block, column) per thread
    static_assert(NB * 8 % 256 == 0, "JPT column jobs for every thread");

    // Block b starts at b * BS + 4 * f(b), f(b) = bit 2 of b, flipped for Cr: the
    // 16-byte row stores of phase A (ds_write_b128, lanes in groups of 8 on 8
    // consecutive blocks -- and Cb next to Cr with 4:2:x) start on 8 distinct
    // 4-bank offsets mod 32, and the column reads of phase C (32 lanes = 4
    // consecutive blocks x 8 columns) still hit 32 distinct banks.  With the plain
    // stride the stores were 2-way conflicted.
    static constexpr int blk_base(int b) { return b * BS + 4 * (((b >> 2) ^ (NCOMP == 3 && b >= NYB + CB ? 1 : 0)) & 1); }

    // the tile's index of LDS block blk in MCU emission order (block_entangler.rs:
    // 69-77, block_fold_iterator.rs:53-148): per MCU its Y blocks row by row (4:2:0:
    // TL, TR, BL, BR), then Cb, then Cr.  Gray: el = blk.
    static constexpr int emit_index(int blk) {
        if (blk < NYB) return (blk % 32 / HR) * BPM + (blk / 32) * HR + blk % 32 % HR;
        return blk < NYB + CB ? (blk - NYB) * BPM + NLUMA : (blk - NYB - CB) * BPM + NLUMA + 1;
    }
};

template <class G>
constexpr bool front_emit_is_permutation() {
    bool seen[G::NB] = {};
    for (int b = 0; b < G::NB; ++b) {
        const int el = G::emit_index(b);
        if (el < 0 || el >= G::NB || seen[el]) return false;
        seen[el] = true;
    }
    return true;
}
static_assert(front_emit_is_permutation<FrontGeom<1, 1>>() && front_emit_is_permutation<FrontGeom<2, 1>>() &&
                  front_emit_is_permutation<FrontGeom<2, 2>>() && front_emit_is_permutation<FrontGeom<1, 1, 1>>(),
              "every block of a tile goes out once");
static_assert(FrontGeom<2, 2>::emit_index(0) == 0 && FrontGeom<2, 2>::emit_index(1) == 1 &&
                  FrontGeom<2, 2>::emit_index(32) == 2 && FrontGeom<2, 2>::emit_index(33) == 3 &&
                  FrontGeom<2, 2>::emit_index(64) == 4 && FrontGeom<2, 2>::emit_index(80) == 5 &&
                  FrontGeom<2, 2>::emit_index(2) == 6,
              "4:2:0: TL, TR, BL, BR, Cb, Cr, the next MCU's TL");
static_assert(FrontGeom<2, 1>::emit_index(1) == 1 && FrontGeom<2, 1>::emit_index(32) == 2 &&
                  FrontGeom<1, 1>::emit_index(1) == 3 && FrontGeom<1, 1, 1>::emit_index(31) == 31,
              "4:2:2: L, R, Cb; 4:4:4: Y, Cb, Cr; gray: raster");

// One plane of a frame as the chunk loaders read it (surface_load.hpp's
// surf_load_chunk, ycc_load.hpp, gray_load.hpp): offsets relative to its first byte.
struct PlaneMem {
    const uint8_t* base;
    __device__ __forceinline__ void load16(long long off, uint32_t (&w)[4]) const {
        const uint4 v = ld16_nt(base + off);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    __device__ __forceinline__ uint32_t load1(long long off) const { return base[off]; }
    __device__ __forceinline__ uint32_t base_lo() const { return (uint32_t)(uintptr_t)base; }
};

// N words from byte offset `off` (any alignment) of the 16-byte aligned LDS array
// s: the N + 1 aligned words that hold them, funnel-shifted (v_alignbyte_b32).
// Reads at most 3 bytes past the N words.
template <int N>
__device__ __forceinline__ void lds_words(const uint8_t* s, int off, uint32_t (&o)[N]) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(s + (off & ~3));
    uint32_t t[N + 1];
#pragma unroll
    for (int i = 0; i <= N; ++i) t[i] = a[i];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], (uint32_t)off & 3u);
}

// a tile's prefetched chunks, registers -> LDS: thread t owns chunks t, t + 256, ...
template <int NCHUNK, int NQ>
__device__ __forceinline__ void front_stage(uint8_t* sRaw, int tid, const uint4 (&v)[NQ]) {
    static_assert(NQ == (NCHUNK + 255) / 256, "chunks per thread");
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = tid + 256 * i;
        if (q < NCHUNK) reinterpret_cast<uint4*>(sRaw)[q] = v[i];
    }
}

// sQ[64 * NQT]: the quantiser tables; sRQ: 1/q, correctly rounded -- integer samples
// (SCALED): fl(scale_row * fl(1/q)), the row scaling of arai8 folded in
template <class G, bool SCALED>
__device__ __forceinline__ void front_fill_qtabs(const float* __restrict__ qtab,  // [2][64] natural, as f32
                                                 float* sQ, float* sRQ, int tid) {
    if (tid < 64 * G::NQT) sQ[tid] = qtab[tid];
    if (tid < 64 * G::NQT) sRQ[tid] = SCALED ? c_arai_scale[(tid >> 3) & 7] * (1.0f / qtab[tid]) : 1.0f / qtab[tid];
}

// ---- C: column pass (stride 8, arai.rs:100-102), quantise (quantizer.rs:53-62):
//      one lane per (block, column), the column's 8 coefficients kept in registers for
// ---- D: their store, the tile's blocks in MCU emission order, only those of MCUs
//      inside the image: 16 B per lane, 8 lanes per block (blocks are column-major
//      in HBM, coef_pos), or the 80-byte form (NARROW, coef_format.hpp).
// The tile starts at MCU (mx0, my) of frame `frame`.  F32: Image<f32> dots, unbounded
// coefficients (arai8, quantize_col8); integer samples take quantize_col8_scaled,
// nan_possible as dct_quant.hpp has it.  (coef, coef_lo and coef_hi are the kernels'
// __restrict__ parameters; repeating the qualifier here costs k_front_gray's uint16
// instantiation a register.)
template <class G, bool NARROW, bool F32>
__device__ __forceinline__ void front_column_pass(const float* sT, const float* sQ, const float* sRQ, int tid,
                                                  bool nan_possible, const Geom& g, int frame, int mx0, int my,
                                                  int16_t* coef, int16_t* coef_lo, int8_t* coef_hi) {
    static_assert(!NARROW || !F32, "Image<f32> dots are unbounded: wide blocks");
    const int col = tid & 7;  // the column pass always handles column tid & 7
    const int nvalid = min(G::TM, g.mcux - mx0) * G::BPM;
    const long long e0 = (long long)frame * g.bpf + ((long long)my * g.mcux + mx0) * G::BPM;
    int16_t* const cbase = coef + e0 * 64;  // (uniform: the stores take a 32-bit lane offset)
    constexpr bool FOLD = NARROW && DMMT_NARROW_FOLD;
#pragma unroll
    for (int jj = 0; jj < G::JPT; ++jj) {
        const int blk = (tid + 256 * jj) >> 3;
        int x[8];
        float mag = 0.0f;  // FOLD: the largest magnitude among the column's hi rows
        {
            const int qt = G::NQT == 1 || blk < G::NYB ? 0 : 64;
            const float* q = sQ + qt + col;
            const float* rq = sRQ + qt + col;
            float v[8];
            const float* tb = sT + G::blk_base(blk) + col;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = tb[i * 8];
            if constexpr (F32) {
                arai8(v);
                quantize_col8(v, q, rq, x);
            } else if constexpr (FOLD) {
                arai8_unscaled(v);
                quantize_col8_scaled_fold(v, q, rq, nan_possible, x, [&](float m, int r, float n) { return coef_hi_mag_row(m, r, n, col); }, mag);
            } else {
                arai8_unscaled(v);
                quantize_col8_scaled(v, q, rq, nan_possible, x);
            }
        }
        const int el = G::NCOMP == 1 ? blk : G::emit_index(blk);
        const bool valid = el < nvalid;  // (uniform over the block's 8 lanes)
        if constexpr (NARROW) {
            coef_store_column_narrow<FOLD>(x, mag > kCoefHiMagMax, col, el, valid, cbase, coef_lo + e0 * 8, coef_hi + e0 * 64);
        } else if (valid) {
            uint32_t pk[4];  // the low halves of two coefficients per word (one v_perm_b32)
#pragma unroll
            for (int i = 0; i < 4; ++i) pk[i] = __builtin_amdgcn_perm((uint32_t)x[2 * i + 1], (uint32_t)x[2 * i], 0x05040100u);
            *reinterpret_cast<uint4*>(cbase + (el * 64 + 8 * col)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
    }
}

}  // namespace dmmt
