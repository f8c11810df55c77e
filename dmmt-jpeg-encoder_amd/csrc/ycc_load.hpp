// ycc_load.hpp -- k_front_ycc's staging arithmetic for planar and semi-planar
// YCbCr device frames (front_ycc.hip), on top of surface_load.hpp's chunk loader
// and, like it, compiled for the host by a CPU unit check
// (tests/native/ycc_load_check.cpp: byte arrays as memory, every access recorded).
//
// A tile is 256 luma columns by 8 * VR luma rows of one frame.  Its bytes:
//  * 8 * VR luma tile rows of 256 bytes from the Y plane (luma_pitch);
//  * 8 chroma tile rows per chroma plane (more for planes finer than the file, see
//    YccTile), 256 / HR positions each: one byte per
//    position from the Cb and from the Cr plane (planar), or two bytes per position
//    -- a Cb,Cr or Cr,Cb pair -- from the one chroma plane (NV); chroma_pitch.
// Every tile row is fetched as the aligned 16-byte chunks that cover it at its own
// misalignment (surf_load_chunk: whole loads inside the plane's span, byte loads
// where a chunk crosses the plane's first or last byte, nothing outside the span)
// and staged at a fixed LDS offset; the row's first sample lies `mis` bytes into
// it.  What a tile row holds past the plane's rectangle -- to the right of its
// last sample and in the rows below its last row -- is the pad sample: 0 for luma
// (0 - 128 = -128, black) and 0x80 for chroma (128 - 128 = 0, no colour), the
// reference's black padding (padder.rs:12-42) in YCbCr.  Phase A needs no bounds
// checks.
//
// SB: bytes per sample, 1 (uint8) or 2 (uint16, the levels and matrix kinds; every pitch,
// plane address and so every offset and misalignment even).  Every byte count above
// scales with it: a luma tile row is 256 * SB bytes, a chroma position SB or 2 * SB
// bytes.  The pad samples are then the caller's (luma_fill, chroma_fill: the code
// that transfers to black, in every sample of a 32-bit word).
#pragma once
#include <stdint.h>

#include "surface_load.hpp"

namespace dmmt {

// the planes of one frame as the loader sees them
struct YccDesc {
    long long luma_pitch, chroma_pitch;  // bytes between rows
    long long luma_span, chroma_span;    // readable bytes of a plane, per frame (dmmt_ycc_plane_span)
    int width, height;                   // luma samples
    int cw, ch;                          // chroma positions: ceil(width / HR), ceil(height / VR)
};

// Tile geometry.  NV: the chroma plane holds pairs.  Chunk q of a tile: the luma
// chunks first (tile row q / LRC, chunk q % LRC of it), then the chroma tile rows
// (plane-major: all CROWS rows of Cb, then of Cr), CRC chunks each.
//
// SHR, SVR: the rates the chroma planes lie at, the file's (HR, VR) unless the kernel
// box-averages finer planes to the file's sampling (front_ycc_sub.hip): a chroma tile
// row then holds 256 / SHR positions and a chroma plane CROWS = 8 * VR / SVR tile rows,
// the plane rows under the tile's 8 * VR luma rows.
template <int HR_, int VR_, bool NV_, int SB_ = 1, int SHR_ = HR_, int SVR_ = VR_>
struct YccTile {
    static_assert(SB_ == 1 || SB_ == 2, "uint8 or uint16 samples");
    static_assert(HR_ % SHR_ == 0 && VR_ % SVR_ == 0, "the planes are as fine as the file or finer");
    static constexpr int HR = HR_, VR = VR_, SB = SB_, SHR = SHR_, SVR = SVR_;
    static constexpr bool NV = NV_;
    static constexpr int ROWS = 8 * VR;               // luma tile rows
    static constexpr int LRB = 256 * SB;              // bytes of a luma tile row
    static constexpr int LRC = LRB / 16 + 1;          // its chunks at any misalignment
    static constexpr int LRS = LRC * 16;              // its stride in LDS
    static constexpr int CPX = 256 / SHR;             // chroma positions of a tile row
    static constexpr int CROWS = 8 * VR / SVR;        // chroma tile rows per plane: 8 or 16
    static constexpr int CSH = CROWS == 8 ? 3 : 4;    // log2 of it
    static constexpr int CBPP = (NV ? 2 : 1) * SB;    // bytes per chroma position of a plane
    static constexpr int CRB = CPX * CBPP, CRC = CRB / 16 + 1, CRS = CRC * 16;
    static constexpr int NCPL = NV ? 1 : 2;           // chroma planes
    static constexpr int NLC = ROWS * LRC;            // luma chunks
    static constexpr int NCHUNK = NLC + CROWS * NCPL * CRC;
    static constexpr int NQ = (NCHUNK + 255) / 256;   // chunks per thread
    static constexpr int BYTES = NCHUNK * 16;
    static constexpr int C_OFF = NLC * 16;            // LDS offset of the first chroma tile row
    // LDS offset of luma tile row ly / of chroma tile row r of chroma plane cp
    static constexpr int luma_row(int ly) { return ly * LRS; }
    static constexpr int chroma_row(int cp, int r) { return C_OFF + (cp * CROWS + r) * CRS; }
};

// the samples of the tile row at position px0 that lie inside a plane `width` wide
DMMT_SURF_FN long long ycc_row_bytes(int width, int bytes_per_pos, int px0, int tile_px) {
    const int px = width - px0 < tile_px ? width - px0 : tile_px;
    return (long long)px * bytes_per_pos;
}

// set every byte of a chunk from byte n on to the pad sample (n <= 0: all, n >= 16: none)
DMMT_SURF_FN void ycc_fill_from(uint32_t (&w)[4], long long n, uint32_t fill) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const long long m = n - 4 * k;
        const uint32_t keep = m >= 4 ? 0xFFFFFFFFu : (m <= 0 ? 0u : (1u << (8 * m)) - 1u);
        w[k] = (w[k] & keep) | (fill & ~keep);
    }
}

// Every chunk of the tile at (x0, y0) is a whole load inside its plane's span:
// the tile lies inside the luma rectangle -- and so inside the chroma rectangle,
// x0 and y0 being multiples of 256 and 8 * VR, which SHR and SVR divide -- and away
// from the planes' first and last bytes.
template <class T>
DMMT_SURF_FN bool ycc_tile_interior(const YccDesc& d, int x0, int y0) {
    if (x0 + 256 > d.width || y0 + T::ROWS > d.height) return false;
    const int cx0 = x0 / T::SHR, cy0 = y0 / T::SVR;
    return surf_interior(surf_row_start(d.luma_pitch, T::SB, x0, y0),
                         surf_row_start(d.luma_pitch, T::SB, x0, y0 + T::ROWS - 1), T::LRB, d.luma_span) &&
           surf_interior(surf_row_start(d.chroma_pitch, T::CBPP, cx0, cy0),
                         surf_row_start(d.chroma_pitch, T::CBPP, cx0, cy0 + T::CROWS - 1), T::CRB, d.chroma_span);
}

// Chunk q < NCHUNK of the tile at (x0, y0) as staged.  Mems:
//   plane(p) -> Mem     plane p of the frame (0: Y, 1: Cb or the pairs, 2: Cr), with
//                       load16 / load1 as surf_load_chunk and
//   uint32_t base_lo()  the low bits of the plane's address
// luma_fill, chroma_fill: the pad samples, as 32-bit words
template <class T, class Mems>
DMMT_SURF_FN void ycc_tile_chunk(const Mems& ms, const YccDesc& d, int x0, int y0, bool interior, int q,
                                 uint32_t (&w)[4], uint32_t luma_fill = 0u, uint32_t chroma_fill = 0x80808080u) {
    const bool luma = q < T::NLC;
    const int qc = luma ? q : q - T::NLC;
    const int rc = luma ? T::LRC : T::CRC;
    const int tr = qc / rc, j = qc - tr * rc;
    const int p = luma ? 0 : 1 + (tr >> T::CSH);
    const int bpp = luma ? T::SB : T::CBPP;
    const int px0 = luma ? x0 : x0 / T::SHR;
    const int py = luma ? y0 + tr : y0 / T::SVR + (tr & (T::CROWS - 1));
    const long long pitch = luma ? d.luma_pitch : d.chroma_pitch;
    const auto& m = ms.plane(p);
    const long long start = surf_row_start(pitch, bpp, px0, py);
    if (interior) {
        m.load16(surf_interior_chunk(m.base_lo(), start, j), w);
        return;
    }
    const uint32_t fill = luma ? luma_fill : chroma_fill;
    w[0] = w[1] = w[2] = w[3] = fill;
    if (py >= (luma ? d.height : d.ch)) return;  // a row below the plane's last: the pad sample
    const int mis = surf_misalign32(m.base_lo(), (uint32_t)pitch, bpp, px0, py);
    const long long rowbytes = ycc_row_bytes(luma ? d.width : d.cw, bpp, px0, luma ? 256 : T::CPX);
    surf_load_chunk(m, start, mis, rowbytes, luma ? d.luma_span : d.chroma_span, j, w);
    ycc_fill_from(w, rowbytes + mis - 16ll * j, fill);  // (bytes of the chunk before the row's end)
}

}  // namespace dmmt
