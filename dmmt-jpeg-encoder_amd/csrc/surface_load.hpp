// surface_load.hpp -- k_front's chunk address arithmetic for pitched, 4-sample
// and planar device surfaces (kernels.hip, SurfTile), kept in a header of its own
// so that the same code is compiled for the host by the CPU unit check
// tests/native/surface_load_check.cpp (a byte array as memory, every access
// recorded).
//
// A plane of a surface is `span` bytes from its first byte (dmmt_surface_span):
// (height - 1) * row_pitch + width * bytes_per_pixel.  The loader may read only
// plane-relative offsets [0, span).  A tile row is 256 pixels of one pixel row of
// one plane; the part of it inside the rectangle is `rowbytes` bytes from offset
// `start` (py * row_pitch + x0 * bytes_per_pixel).  It is fetched as the aligned
// 16-byte chunks that cover it: chunk j lies at offset start - mis + 16 j, mis =
// the address of `start` mod 16.
//  * a chunk that begins at or past start + rowbytes is not fetched (it stages 0);
//  * a chunk inside [0, span) is one 16-byte load;
//  * a chunk that crosses the plane's first or last byte is read byte by byte,
//    only the bytes inside [0, span);
//  * of a fetched chunk only the bytes before start + rowbytes are kept: whatever
//    follows the rectangle's right edge in memory -- row padding, the next pixels
//    of a parent image, another plane -- stages as 0, the reference's black
//    padding (padder.rs:12-42), and never reaches the range check.
// The bytes of the first chunk in front of `start` are staged as loaded; phase A
// starts reading at `mis` and never sees them.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DMMT_SURF_FN __device__ __forceinline__
#else
#define DMMT_SURF_FN inline
#endif

namespace dmmt {

// largest row pitch the 64-bit offsets are specified for (65535 rows * 2^30 < 2^46)
constexpr long long kMaxRowPitch = 1ll << 30;

// plane-relative offset of pixel (x0, py)
DMMT_SURF_FN long long surf_row_start(long long pitch, int bytes_per_pixel, int x0, int py) {
    return (long long)py * pitch + (long long)x0 * bytes_per_pixel;
}

// (address of that pixel) mod 16 from 32-bit arithmetic: only the low 4 bits matter
DMMT_SURF_FN int surf_misalign32(uint32_t base_lo, uint32_t pitch_lo, int bytes_per_pixel, int x0, int py) {
    return (int)((base_lo + (uint32_t)py * pitch_lo + (uint32_t)x0 * (uint32_t)bytes_per_pixel) & 15u);
}

// bytes of the tile row at x0 that lie inside the rectangle
DMMT_SURF_FN long long surf_row_bytes(int width, int bytes_per_pixel, int x0) {
    const int px = width - x0 < 256 ? width - x0 : 256;
    return (long long)px * bytes_per_pixel;
}

// every chunk of the tile rows [first, last] (offsets of their first bytes) is a
// whole load inside [0, span) whatever the misalignment: RB = 256 * bytes_per_pixel
DMMT_SURF_FN bool surf_interior(long long first, long long last, int RB, long long span) {
    return first >= 16 && last + RB + 16 <= span;
}

// plane-relative offset of chunk j of the interior tile row at offset row_off
// (base_lo: the low bits of the plane's address)
DMMT_SURF_FN long long surf_interior_chunk(uint32_t base_lo, long long row_off, int j) {
    return row_off - (long long)((base_lo + (uint32_t)row_off) & 15u) + 16ll * j;
}

// keep the first n bytes of a chunk (n <= 0: none, n >= 16: all)
DMMT_SURF_FN void surf_keep(uint32_t (&w)[4], long long n) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const long long m = n - 4 * k;
        w[k] &= m >= 4 ? 0xFFFFFFFFu : (m <= 0 ? 0u : (1u << (8 * m)) - 1u);
    }
}

// Chunk j of the tile row at `start` (mis = its address mod 16), through Mem:
//   void load16(long long off, uint32_t (&w)[4])   16 bytes at plane offset off
//   uint32_t load1(long long off)                  one byte
// w: the chunk as staged.
template <typename Mem>
DMMT_SURF_FN void surf_load_chunk(const Mem& m, long long start, int mis, long long rowbytes, long long span, int j,
                                  uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    const long long c = start - mis + 16ll * j;
    const long long end = start + rowbytes;
    if (c >= end) return;
    if (c >= 0 && c + 16 <= span) {
        m.load16(c, w);
    } else {
        for (int k = 0; k < 16; ++k)
            if (c + k >= 0 && c + k < span && c + k < end) w[k >> 2] |= m.load1(c + k) << (8 * (k & 3));
    }
    if (end - c < 16) surf_keep(w, end - c);
}

}  // namespace dmmt
