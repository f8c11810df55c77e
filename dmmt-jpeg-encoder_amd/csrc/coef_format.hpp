// coef_format.hpp -- the narrow form of a quantised block between k_front and the
// entropy kernels: 80 bytes instead of the 128 of an int16 block.
//   coef_lo[block]  int16[8]: zigzag positions 0..7 (the DC and the first seven ACs),
//                   consecutive blocks 16 bytes apart
//   coef_hi[block]  int8[64]: zigzag position k >= 8 at byte coef_pos(k) (the
//                   column-major order of the wide block); a value outside
//                   -127..127 is stored as 0x80, the escape; the bytes of positions
//                   1..7 are 0 and the byte of position 0 (byte 0) is the block's
//                   flag: 1 when one of its bytes is an escape, else 0 -- the walks
//                   vote on it once per block and test for escapes position by
//                   position only in a wave that holds such a block (a vote at every
//                   non-zero position cost k_hist 3.5 us of its 25 on the 4K frame,
//                   profiles/STUDIES.md section J)
//   coef[block]     the wide int16 block is the escape store: a column (8 values,
//                   16 bytes at int16 index 8 * column) is written there only when
//                   one of its hi bytes is an escape; the rest of the buffer is not
//                   touched and not read
// The form is chosen per call on the host (coef_narrow_for): the same layout for
// every block of the call, no per-block switch.  Everything here but the device
// section is plain C++ (tests/native/coef_format_check.cpp).
#pragma once
#include <stdint.h>

#include "jpeg_common.hpp"

namespace dmmt {

constexpr int kCoefLoCount = 8;  // zigzag positions held as int16
constexpr int kCoefLoBytes = 2 * kCoefLoCount, kCoefHiBytes = 64;
constexpr int kCoefEscape = -128;  // the hi byte 0x80

constexpr bool coef_in_lo(int k) { return k < kCoefLoCount; }
// the hi byte of value v (v_med3_i32(v, -128, 128), low byte)
constexpr int coef_hi_byte(int v) { return v < -127 || v > 127 ? kCoefEscape : v; }
// 32-bit word of the 16 hi words, and bit offset in it, of zigzag position k
constexpr int coef_hi_word(int k) { return coef_pos(k) >> 2; }
constexpr int coef_hi_shift(int k) { return 8 * (coef_pos(k) & 3); }
// hi bytes of column c that belong to lo positions (rows 0 .. n-1 of the column):
// natural (row, col) of zigzag 0..7 = (0,0) (0,1) (1,0) (2,0) (1,1) (0,2) (0,3) (1,2)
constexpr int coef_lo_rows(int c) { return c == 0 ? 3 : c < 3 ? 2 : c == 3 ? 1 : 0; }

// host model of k_front's store of one block (zz: zigzag order)
inline void coef_pack_block(const int16_t* zz, int16_t* lo, int8_t* hi, int16_t* wide) {
    for (int k = 0; k < kCoefLoCount; ++k) lo[k] = zz[k];
    bool esc[8] = {false};
    bool any = false;
    for (int k = 0; k < 64; ++k) {
        const int p = coef_pos(k);
        const int b = coef_in_lo(k) ? 0 : coef_hi_byte(zz[k]);
        hi[p] = (int8_t)b;
        if (!coef_in_lo(k) && b == kCoefEscape) esc[p >> 3] = any = true;
    }
    hi[coef_pos(0)] = any ? 1 : 0;  // the block's flag
    for (int k = 0; k < 64; ++k)
        if (esc[coef_pos(k) >> 3]) wide[coef_pos(k)] = zz[k];
}
// host model of the walks' read of zigzag position k: the escape test only in a
// flagged block
inline bool coef_block_flag(const int8_t* hi) { return hi[coef_pos(0)] != 0; }
inline int coef_read(int k, const int16_t* lo, const int8_t* hi, const int16_t* wide) {
    if (coef_in_lo(k)) return lo[k];
    const int b = hi[coef_pos(k)];
    return coef_block_flag(hi) && b == kCoefEscape ? wide[coef_pos(k)] : b;
}

// The form of a call.  DMMT_COEF_FORMAT=auto|wide|narrow is read at context
// creation; Image<f32> dots are unbounded and always wide (k_front's f32
// instantiations have no narrow twin).  auto: narrow when no quantiser of a hi
// position is below kCoefNarrowMinQ in either table (natural order, as
// dmmt_options) -- the hi coefficient is about 1016 / q at most, and at q = 1
// (IJG quality 95 and above) escapes are a few per cent of the non-zero ACs,
// each a dependent load for its wave (profiles/STUDIES.md section J).  A wrong
// choice costs time, never bytes.
enum { COEF_FORMAT_AUTO = 0, COEF_FORMAT_WIDE = 1, COEF_FORMAT_NARROW = 2 };
constexpr int kCoefNarrowMinQ = 2;
inline bool coef_narrow_for(int mode, int sample_bytes, const uint8_t* luma_q, const uint8_t* chroma_q) {
    if (sample_bytes == 4 || mode == COEF_FORMAT_WIDE) return false;
    if (mode == COEF_FORMAT_NARROW) return true;
    for (int k = kCoefLoCount; k < 64; ++k)
        if (luma_q[kZigzag[k]] < kCoefNarrowMinQ || chroma_q[kZigzag[k]] < kCoefNarrowMinQ) return false;
    return true;
}

// k_front's escape test (DMMT_NARROW_FOLD): a column job escapes iff one of its hi
// rows -- rows 3..7 always, of rows 0..2 those from coef_lo_rows(col) on -- holds a
// value outside -127..127.  n: the column's values as floats (the quantiser's rintf
// results, exact).  The largest magnitude among the hi rows: rows 0..2 through a
// select on the column (on the device the three conditions are lane masks that do
// not change in the kernel: col = lane & 7), then three v_max3 and a v_max with the
// magnitudes as source modifiers.
#ifdef __HIPCC__
#define DMMT_CF_FN __host__ __device__ __forceinline__
#else
#define DMMT_CF_FN inline
#endif
// one row at a time (r a constant once unrolled): the running maximum m with row r of column c
DMMT_CF_FN float coef_hi_mag_row(float m, int r, float n, int c) {
    static_assert(coef_lo_rows(0) == 3 && coef_lo_rows(1) == 2 && coef_lo_rows(2) == 2 && coef_lo_rows(3) == 1 &&
                      coef_lo_rows(4) == 0 && coef_lo_rows(7) == 0,
                  "row 2 is hi from column 1 on, row 1 from column 3 on, row 0 from column 4 on");
    const float a = __builtin_fabsf(n);
    const bool hi = r >= 3 || c >= (r == 0 ? 4 : r == 1 ? 3 : 1);
    return __builtin_fmaxf(m, hi ? a : 0.0f);
}
DMMT_CF_FN float coef_hi_mag(const float (&n)[8], int c) {
    float m = 0.0f;
    for (int r = 0; r < 8; ++r) m = coef_hi_mag_row(m, r, n[r], c);
    return m;
}
constexpr float kCoefHiMagMax = 127.0f;  // a larger coef_hi_mag: the column escapes
// host model of the test on the int16 column x (rows 0..7) of column c
inline bool coef_column_escapes(const int16_t* x, int c) {
    float n[8];
    for (int r = 0; r < 8; ++r) n[r] = (float)x[r];
    return coef_hi_mag(n, c) > kCoefHiMagMax;
}

#ifndef DMMT_NARROW_FOLD
// k_front's narrow store: one folded range test, clamps only in a wave with an escape.
// Off in the product: alone it measured level with or below the clamps on the 4-lane
// 4K bench (profiles/STUDIES.md section K); `make VARIANT=x EXTRA=-DDMMT_NARROW_FOLD=1`
// builds it.
#define DMMT_NARROW_FOLD 0
#endif

#ifdef __HIPCC__
// true when a byte of w is 0x80
__device__ __forceinline__ bool coef_word_escapes(uint32_t w) {
    const uint32_t t = w ^ 0x80808080u;  // (a zero byte of t)
    return ((t - 0x01010101u) & ~t & 0x80808080u) != 0u;
}

// k_front's store of one column job: lane `col` of a block's 8 lanes holds the
// column's 8 quantised values x (rows 0..7).  Every lane of the wave calls it (the
// lo values travel to the block's col-0 lane over DPP row shifts); `valid` is
// uniform over a block's lanes.  el: the block's index from the three (uniform)
// bases.  FOLD: `esc_fold` is the lane's escape test (coef_hi_mag of the column above
// kCoefHiMagMax), and a wave in which no lane escapes -- nearly every one, by
// coef_narrow_for -- packs the low bytes of x as they are (two's complement: the
// value, for |v| <= 127), without the clamps and the test on the packed words.
template <bool FOLD>
__device__ __forceinline__ void coef_store_column_narrow(const int (&x)[8], bool esc_fold, int col, int el, bool valid,
                                                         int16_t* __restrict__ wide, int16_t* __restrict__ lo,
                                                         int8_t* __restrict__ hi) {
    // byte 0 of four values per word (selector 0x0c: a zero byte)
    auto pack4 = [](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        return __builtin_amdgcn_perm(b, a, 0x0c0c0400u) | __builtin_amdgcn_perm(d, c, 0x04000c0cu);
    };
    const uint32_t himask = 0xFFFFFFFFu << (8 * (col == 0 ? 3 : col < 3 ? 2 : col == 3 ? 1 : 0));  // the lo positions' bytes (coef_lo_rows)
    // rows 0 and 1 of columns 1, 2, 3 to the col-0 lane (row_shl:n: lane i reads lane i + n)
    const uint32_t p = __builtin_amdgcn_perm((uint32_t)x[1], (uint32_t)x[0], 0x05040100u);
    const uint32_t s1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x101, 0xF, 0xF, true);
    const uint32_t s2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x102, 0xF, 0xF, true);
    const uint32_t s3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p, 0x103, 0xF, 0xF, true);
    uint32_t w0, w1;
    bool esc;
    unsigned long long em;
    if (FOLD) {
        esc = esc_fold;
        em = __builtin_amdgcn_ballot_w64(esc);
    }
    if (FOLD && em == 0) {  // (uniform) nearly always
        w0 = pack4((uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)x[3]) & himask;
        w1 = pack4((uint32_t)x[4], (uint32_t)x[5], (uint32_t)x[6], (uint32_t)x[7]);
    } else {
        uint32_t c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = (uint32_t)min(max(x[i], -128), 128);  // v_med3_i32; low byte: the value or 0x80
        w0 = pack4(c[0], c[1], c[2], c[3]) & himask;
        w1 = pack4(c[4], c[5], c[6], c[7]);
        if (!FOLD) {
            esc = coef_word_escapes(w0) || coef_word_escapes(w1);
            em = __builtin_amdgcn_ballot_w64(esc);
        }
        // the block's flag: the OR of its 8 lanes' escape tests into the col-0 lane, whose
        // byte 0 is position 0's -- from the wave's vote, and only when a lane escapes
        if (em != 0) {  // (uniform) rare
            const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const uint32_t group = (uint32_t)(em >> (lane & 56u)) & 0xFFu;  // the votes of the block's 8 lanes
            w0 |= col == 0 && group != 0u ? 1u : 0u;
        }
    }
    if (valid) {
        *reinterpret_cast<uint2*>(hi + (el * 64 + 8 * col)) = make_uint2(w0, w1);
        if (col == 0) {
            const uint32_t l0 = __builtin_amdgcn_perm(s1, p, 0x05040100u);                 // (0,0) (0,1)
            const uint32_t l1 = __builtin_amdgcn_perm((uint32_t)x[2], p, 0x05040302u);     // (1,0) (2,0)
            const uint32_t l2 = __builtin_amdgcn_perm(s2, s1, 0x05040302u);                // (1,1) (0,2)
            const uint32_t l3 = __builtin_amdgcn_perm(s2, s3, 0x07060100u);                // (0,3) (1,2)
            *reinterpret_cast<uint4*>(lo + el * 8) = make_uint4(l0, l1, l2, l3);
        }
        if (esc) {  // rare: the int16 column, where the wide form has it
            uint32_t pk[4];
            pk[0] = p;
#pragma unroll
            for (int i = 1; i < 4; ++i) pk[i] = __builtin_amdgcn_perm((uint32_t)x[2 * i + 1], (uint32_t)x[2 * i], 0x05040100u);
            *reinterpret_cast<uint4*>(wide + (el * 64 + 8 * col)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
    }
}

// the walks' view of a narrow block in registers: 4 lo words, 16 hi words
struct NarrowCoef {
    uint32_t lo[4];
    uint32_t hi[16];
};
__device__ __forceinline__ void load_narrow(const int16_t* __restrict__ lo, const int8_t* __restrict__ hi, long long e,
                                            NarrowCoef& b) {
    const uint4 l = *reinterpret_cast<const uint4*>(lo + e * 8);
    b.lo[0] = l.x, b.lo[1] = l.y, b.lo[2] = l.z, b.lo[3] = l.w;
    const uint4* q = reinterpret_cast<const uint4*>(hi + e * 64);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 v = q[i];
        b.hi[4 * i] = v.x, b.hi[4 * i + 1] = v.y, b.hi[4 * i + 2] = v.z, b.hi[4 * i + 3] = v.w;
    }
}
// the block's flag, and zigzag position k (a constant once the walk is unrolled):
// its value as stored (an escape reads -128), v_bfe_i32
__device__ __forceinline__ bool narrow_flag(const NarrowCoef& b) { return (b.hi[0] & 0xFFu) != 0u; }
__device__ __forceinline__ int narrow_at(const NarrowCoef& b, int k) {
    if (coef_in_lo(k)) return (k & 1) ? ((int)b.lo[k >> 1] >> 16) : (int)(int16_t)(b.lo[k >> 1] & 0xFFFFu);
    return (int)(b.hi[coef_hi_word(k)] << (24 - coef_hi_shift(k))) >> 24;
}
#endif

}  // namespace dmmt
