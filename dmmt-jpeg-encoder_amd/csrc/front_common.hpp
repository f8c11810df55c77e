// front_common.hpp -- the device code the front kernels share (kernels.hip:
// k_front, k_front_surf; front_ycc.hip: k_front_ycc; front_ycc_sub.hip: k_front_ycc_sub;
// front_gray.hip: k_front_gray,
// and their narrow twins): the tile's block geometry and the LDS layout of its
// row-transformed blocks (front_layout.hpp) with the two accessors every kernel
// goes through, the plane accessor of the chunk loaders, the staging copy, the
// quantiser tables' LDS fill, the column pass with the blocks' store.  What differs
// between the kernels -- how a tile's bytes are fetched and phase A, the samples'
// way to the row-transformed blocks -- stays in their own files, and so does the
// tile loop that calls both: each kernel body writes out the same loop (as a
// function taking the two as callables it cost three of the budgeted instantiations
// registers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coef_format.hpp"
#include "dct_quant.hpp"
#include "device_common.hpp"
#include "front_layout.hpp"
#include "jpeg_common.hpp"

namespace dmmt {

// (the tile's block geometry and sT's layout: FrontGeom, front_layout.hpp)

// sT's two accessors.  Phase A of every front kernel stores a row-transformed row
// with front_store_row, the column pass reads a column with front_load_column: the
// layout (front_layout.hpp) is written down there and nowhere else.
// row r of block b: two 16-byte stores
template <class G>
__device__ __forceinline__ void front_store_row(float* sT, int b, int r, const float (&v)[8]) {
    const int q = G::st_quad(b, r, 0);
    *reinterpret_cast<float4*>(sT + q) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(sT + G::st_second_half(q)) = make_float4(v[4], v[5], v[6], v[7]);
}
// column c of block b, rows 0 to 7
template <class G>
__device__ __forceinline__ void front_load_column(const float* sT, int b, int c, float (&v)[8]) {
    const int a0 = G::st_at(b, 0, c);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = sT[G::st_row_of_column(a0, i)];
}

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

// sQ[64 * NQT]: the quantiser tables (KEEP_Q false: the kernel keeps no copy and hands
// the column pass qtab itself); sRQ: 1/q, correctly rounded -- integer samples
// (SCALED): fl(scale_row * fl(1/q)), the row scaling of arai8 folded in
template <class G, bool SCALED, bool KEEP_Q = true>
__device__ __forceinline__ void front_fill_qtabs(const float* __restrict__ qtab,  // [2][64] natural, as f32
                                                 float* sQ, float* sRQ, int tid) {
    if constexpr (KEEP_Q) {
        if (tid < 64 * G::NQT) sQ[tid] = qtab[tid];
    }
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
// instantiation a register.)  q: the quantiser tables, the kernel's copy in LDS or
// the table in global memory -- only the quantisers' rare exact path reads them.
template <class G, bool NARROW, bool F32>
__device__ __forceinline__ void front_column_pass(const float* sT, const float* qt, const float* sRQ, int tid,
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
            const int qo = G::NQT == 1 || blk < G::NYB ? 0 : 64;
            const float* q = qt + qo + col;
            const float* rq = sRQ + qo + col;
            float v[8];
            front_load_column<G>(sT, blk, col, v);
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
