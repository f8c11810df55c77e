// front_layout.hpp -- the front kernels' tile: its block geometry and where a
// row-transformed block's floats lie in LDS (sT).  Plain C++, no device code:
// front_common.hpp includes it for the kernels, tests/native/front_layout_check.cpp
// compiles it for the host.
#pragma once

namespace dmmt {

// A tile: 256 padded pixel columns by 8 * VR rows = TM horizontally adjacent MCUs
// of one MCU row.  In LDS its row-transformed blocks (sT) lie block-major: the Y
// blocks first, 32 columns x VR rows, then the Cb and the Cr blocks (NCOMP 3).
// NCOMP 1: a grayscale frame, HR = VR = 1, an MCU is one Y block.
// COMPACT: sT without padding (below); the kernels that need the LDS for a fifth
// workgroup per CU take it (uint8 4:4:4), the others keep the padded layout, which
// costs them a register or two less (one store address per row, not two).
template <int HR_, int VR_, int NCOMP_ = 3, bool COMPACT_ = false>
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
    static constexpr bool COMPACT = COMPACT_;
    static constexpr int BS = 72;                 // padded: LDS floats per block, 64 + pad
    static constexpr int ST_FLOATS = COMPACT ? NB * 64 : NB * BS + 4;  // sT
    static constexpr int JPT = NB * 8 / 256;      // column jobs (block, column) per thread
    static_assert(NB * 8 % 256 == 0, "JPT column jobs for every thread");
    static_assert(NB % 4 == 0, "compact: sT holds the blocks four by four");

    // The padded layout.  Block b starts at b * BS + 4 * f(b), f(b) = bit 2 of b,
    // flipped for Cr: the 16-byte row stores of phase A (ds_write_b128, lanes in
    // groups of 8 on 8 consecutive blocks -- and Cb next to Cr with 4:2:x) start on 8
    // distinct 4-bank offsets mod 32, and the column reads of phase C (32 lanes = 4
    // consecutive blocks x 8 columns) hit 32 distinct banks.
    static constexpr int blk_base(int b) { return b * BS + 4 * (((b >> 2) ^ (NCOMP == 3 && b >= NYB + CB ? 1 : 0)) & 1); }

    // The compact layout: 64 floats per block, no padding.  Four consecutive blocks
    // share 256 floats, row by row: row r of the four lies in the 32 floats from
    // 32 r, block b's eight at 8 (b & 3) of them, and the row's two 16-byte halves
    // change places where f(b) is set: bit 2 of b, with 4:2:x flipped by bit 4 of b,
    // which tells Cr from Cb there (CB = 16, NYB a multiple of 32) and is one value
    // over 8 consecutive Y blocks.
    //  * The column reads of phase C take 32 consecutive floats: 32 distinct banks,
    //    and a column's rows lie a constant 32 floats apart, one address and eight
    //    offsets.
    //  * The row stores of phase A start at 8 (b & 3) + 4 (h ^ f(b)) mod 32: b & 3 and
    //    f(b) take their 8 combinations, 8 distinct 4-bank offsets.  (A constant
    //    distance between a row's halves is not to be had without padding: the halves
    //    of 8 consecutive blocks must fill the 8 four-bank slots for either half.)
    // The same count of conflicts as the padded layout: none
    // (tests/native/front_layout_check.cpp counts both).
    static constexpr int st_flip(int b) { return ((b >> 2) ^ (HR == 2 ? b >> 4 : 0)) & 1; }
    static_assert(HR == 1 || (CB == 16 && NYB % 32 == 0), "bit 4 of a chroma block's index: Cr");
    // columns 4h .. 4h + 3 of row r of block b: 16-byte aligned
    static constexpr int st_quad(int b, int r, int h) {
        return COMPACT ? ((b >> 2) << 8) + (r << 5) + ((b & 3) << 3) + ((h ^ st_flip(b)) << 2)
                       : blk_base(b) + r * 8 + h * 4;
    }
    // st_quad(b, r, 1) from q = st_quad(b, r, 0)
    static constexpr int st_second_half(int q) { return COMPACT ? q ^ 4 : q + 4; }
    // column c of row r of block b
    static constexpr int st_at(int b, int r, int c) {
        return COMPACT ? st_quad(b, r, c >> 2) + (c & 3) : blk_base(b) + r * 8 + c;
    }
    // st_at(b, r, c) from a0 = st_at(b, 0, c)
    static constexpr int st_row_of_column(int a0, int r) { return a0 + r * (COMPACT ? 32 : 8); }

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
static_assert(FrontGeom<1, 1, 3, true>::st_row_of_column(FrontGeom<1, 1, 3, true>::st_at(87, 0, 6), 5) ==
                  FrontGeom<1, 1, 3, true>::st_at(87, 5, 6),
              "a column's rows, 32 floats apart");

}  // namespace dmmt
