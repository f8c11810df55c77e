// gray_load.hpp -- k_front_gray's staging arithmetic for a one-channel device
// plane (front_gray.hip), on top of surface_load.hpp's chunk loader and, like it,
// compiled for the host by a CPU unit check (tests/native/gray_load_check.cpp: a
// byte array as memory, every access recorded).
//
// A tile is 256 columns by 8 rows of one frame: 8 tile rows of 256 * SB bytes (SB
// = bytes per sample) from the plane, rows `pitch` bytes apart.  Every tile row is
// fetched as the aligned 16-byte chunks that cover it at its own misalignment
// (surf_load_chunk: whole loads inside the plane's span, byte loads where a chunk
// crosses the plane's first or last byte, nothing outside the span) and staged at
// a fixed LDS offset; the row's first sample lies `mis` bytes into it.  What a
// tile row holds past the plane's rectangle -- to the right of its last sample
// and in the rows below its last row -- is 0: sample 0 (or the dot 0.0), the
// reference's black padding (padder.rs:12-42).  Phase A needs no bounds checks.
#pragma once
#include <stdint.h>

#include "surface_load.hpp"

namespace dmmt {

// the plane of one frame as the loader sees it
struct GrayDesc {
    long long pitch;  // bytes between rows
    long long span;   // readable bytes of the plane, per frame (dmmt_gray_span)
    int width, height;
};

// Tile geometry for SB-byte samples.  Chunk q of a tile: tile row q / RC, chunk
// q % RC of it.
template <int SB_>
struct GrayTile {
    static constexpr int SB = SB_;
    static constexpr int ROWS = 8;
    static constexpr int RB = 256 * SB;        // bytes of a tile row
    static constexpr int RC = RB / 16 + 1;     // its chunks at any misalignment
    static constexpr int RS = RC * 16;         // its stride in LDS
    static constexpr int NCHUNK = ROWS * RC;
    static constexpr int NQ = (NCHUNK + 255) / 256;  // chunks per thread
    static constexpr int BYTES = NCHUNK * 16;
    static constexpr int row(int ly) { return ly * RS; }  // LDS offset of tile row ly
};

// Every chunk of the tile at (x0, y0) is a whole load inside the plane's span: the
// tile lies inside the rectangle and away from the plane's first and last bytes.
template <class T>
DMMT_SURF_FN bool gray_tile_interior(const GrayDesc& d, int x0, int y0) {
    if (x0 + 256 > d.width || y0 + T::ROWS > d.height) return false;
    return surf_interior(surf_row_start(d.pitch, T::SB, x0, y0), surf_row_start(d.pitch, T::SB, x0, y0 + T::ROWS - 1),
                         T::RB, d.span);
}

// Chunk q < NCHUNK of the tile at (x0, y0) as staged.  Mem: the plane of the frame,
// with load16 / load1 as surf_load_chunk and base_lo(), the low bits of its address.
template <class T, class Mem>
DMMT_SURF_FN void gray_tile_chunk(const Mem& m, const GrayDesc& d, int x0, int y0, bool interior, int q,
                                  uint32_t (&w)[4]) {
    const int tr = q / T::RC, j = q - tr * T::RC;
    const int py = y0 + tr;
    const long long start = surf_row_start(d.pitch, T::SB, x0, py);
    if (interior) {
        m.load16(surf_interior_chunk(m.base_lo(), start, j), w);
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (py >= d.height) return;  // a row below the plane's last: black
    const int mis = surf_misalign32(m.base_lo(), (uint32_t)d.pitch, T::SB, x0, py);
    surf_load_chunk(m, start, mis, surf_row_bytes(d.width, T::SB, x0), d.span, j, w);
}

}  // namespace dmmt
