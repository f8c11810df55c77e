// CPU unit check of k_front's surface loader (csrc/surface_load.hpp, the kernel's
// own header compiled for the host): every tile of small surfaces is loaded the
// way SurfTile::load does it -- the interior fast path where surf_interior allows
// it, surf_load_chunk elsewhere -- from a byte array that records each access.
//  * no byte outside [base, base + span) is touched;
//  * from its first pixel on, a staged tile row holds the row's bytes inside the
//    rectangle followed by zeros, although the bytes around the rectangle are
//    never zero here.
// usage: surface_load_check [--no-span-check]
//   --no-span-check: the loader is given a span 64 bytes too large (the bound
//   widened on purpose); the check must report the out-of-span address, exit 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dmmt-jpeg-encoder_amd/csrc/surface_load.hpp"

using namespace dmmt;

namespace {

struct Memory {
    std::vector<uint8_t> bytes;  // [lead | span | trail], never 0
    long long lead, span;
    mutable long long bad_off = 0;
    mutable int bad = 0;
    void touch(long long off, int n) const {
        if ((off < 0 || off + n > span) && !bad++) bad_off = off < 0 ? off : off + n - 1;
    }
    void load16(long long off, uint32_t (&w)[4]) const {
        touch(off, 16);
        memcpy(w, &bytes[(size_t)(lead + off)], 16);
    }
    uint32_t load1(long long off) const {
        touch(off, 1);
        return bytes[(size_t)(lead + off)];
    }
};

uint32_t rng_state = 12345u;
uint8_t next_nonzero() {
    rng_state = rng_state * 1664525u + 1013904223u;
    const uint8_t b = (uint8_t)(rng_state >> 24);
    return b ? b : 0xFF;
}

long long checked = 0;

// one surface: every tile, as SurfTile<., ROWS, .>::load and ::stage
int run(int mis0, int bpp, int width, int height, long long pitch, int ROWS, long long widen) {
    const long long span = (long long)(height - 1) * pitch + (long long)width * bpp;
    Memory m;
    m.lead = 64, m.span = span;
    m.bytes.resize((size_t)(64 + span + 64 + widen));
    for (auto& b : m.bytes) b = next_nonzero();
    const uint32_t base = 0x1000u + (uint32_t)mis0;  // the plane's address (only its low bits matter)
    const long long lspan = span + widen;           // what the loader is told
    const int RB = 256 * bpp, RC = RB / 16 + 1, RS = RC * 16;
    std::vector<uint8_t> staged((size_t)ROWS * RS);
    for (int y0 = 0; y0 < height; y0 += ROWS)
        for (int x0 = 0; x0 < width; x0 += 256) {
            memset(staged.data(), 0xEE, staged.size());
            const long long first = surf_row_start(pitch, bpp, x0, y0);
            const bool interior = x0 + 256 <= width && y0 + ROWS <= height &&
                                  surf_interior(first, surf_row_start(pitch, bpp, x0, y0 + ROWS - 1), RB, lspan);
            const long long rowbytes = surf_row_bytes(width, bpp, x0);
            for (int q = 0; q < ROWS * RC; ++q) {
                const int row = q / RC, j = q % RC, py = y0 + row;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (interior) {
                    m.load16(surf_interior_chunk(base, first + (long long)row * pitch, j), w);
                } else if (py < height) {
                    surf_load_chunk(m, surf_row_start(pitch, bpp, x0, py),
                                    surf_misalign32(base, (uint32_t)pitch, bpp, x0, py), rowbytes, lspan, j, w);
                }
                memcpy(&staged[(size_t)q * 16], w, 16);
            }
            if (m.bad) {
                printf("FAIL: out-of-span access at plane offset %lld (span %lld): mis %d bpp %d %dx%d pitch %lld "
                       "rows/tile %d tile (%d,%d)\n",
                       m.bad_off, span, mis0, bpp, width, height, pitch, ROWS, x0, y0);
                return 1;
            }
            for (int row = 0; row < ROWS; ++row) {
                const int py = y0 + row;
                const int mis = surf_misalign32(base, (uint32_t)pitch, bpp, x0, py);
                const long long start = surf_row_start(pitch, bpp, x0, py);
                // phase A reads [mis, mis + RB) of the staged row
                for (int k = 0; k < RB; ++k) {
                    const uint8_t got = staged[(size_t)row * RS + mis + k];
                    const uint8_t want = py < height && k < rowbytes ? m.bytes[(size_t)(m.lead + start + k)] : 0;
                    ++checked;
                    if (got != want) {
                        printf("FAIL: staged byte %d of row %d is %u, expected %u: mis %d bpp %d %dx%d pitch %lld "
                               "rows/tile %d tile (%d,%d)\n",
                               k, py, got, want, mis0, bpp, width, height, pitch, ROWS, x0, y0);
                        return 1;
                    }
                }
            }
        }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const long long widen = argc > 1 && !strcmp(argv[1], "--no-span-check") ? 64 : 0;
    const int bpps[] = {1, 2, 3, 4, 6, 12}, widths[] = {1, 5, 255, 256, 257, 768};  // (768: a middle tile on the interior path)
    long long surfaces = 0;
    for (int mis = 0; mis < 16; ++mis)
        for (int bpp : bpps)
            for (int width : widths)
                for (int rows = 1; rows <= 3; ++rows)
                    for (int extra : {0, 1, 16})
                        for (int tile_rows : {rows, 8}) {
                            if (run(mis, bpp, width, rows, (long long)width * bpp + extra, tile_rows, widen)) return 1;
                            ++surfaces;
                        }
    printf("ok: %lld surfaces, %lld staged bytes checked\n", surfaces, checked);
    return 0;
}
