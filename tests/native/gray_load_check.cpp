// CPU unit check of k_front_gray's staging (csrc/gray_load.hpp, the kernel's own
// header compiled for the host): every tile of small one-channel frames is loaded
// the way the kernel does it -- gray_tile_interior, then gray_tile_chunk for every
// chunk -- from a byte array that records each access.
//  * no byte outside [base, base + span) is touched;
//  * from its first sample on, a staged tile row holds the row's bytes inside the
//    rectangle followed by 0, and the tile rows below the plane's last row hold 0
//    only, although the bytes around the rectangle are never 0 here.
// usage: gray_load_check [--no-span-check]
//   --no-span-check: the loader is given a span 64 bytes too large (the bound
//   widened on purpose); the check must report the out-of-span address, exit 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dmmt-jpeg-encoder_amd/csrc/gray_load.hpp"

using namespace dmmt;

namespace {

struct Memory {
    std::vector<uint8_t> bytes;  // [lead | span | trail], never 0
    long long lead = 64, span = 0;
    uint32_t base = 0;           // the plane's address (only its low bits matter)
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
    uint32_t base_lo() const { return base; }
    uint8_t at(long long off) const { return bytes[(size_t)(lead + off)]; }
};

uint32_t rng_state = 12345u;
uint8_t next_sample() {
    rng_state = rng_state * 1664525u + 1013904223u;
    const uint8_t b = (uint8_t)(rng_state >> 24);
    return b == 0 ? 0xFF : b;
}

long long checked = 0;

// one frame of SB-byte samples: every tile, as k_front_gray's load_tile and its staging stores
template <int SB>
int run(int mis0, int width, int height, long long pitch_extra, long long widen) {
    using T = GrayTile<SB>;
    GrayDesc d;
    d.width = width, d.height = height;
    d.pitch = (long long)(width + pitch_extra) * SB;
    const long long span = (long long)(height - 1) * d.pitch + (long long)width * SB;
    d.span = span + widen;  // what the loader is told
    Memory mem;
    mem.span = span, mem.base = 0x1000u + (uint32_t)(mis0 / SB * SB);  // (a multiple of the sample size)
    mem.bytes.resize((size_t)(64 + span + 64 + widen));
    for (auto& b : mem.bytes) b = next_sample();
    std::vector<uint8_t> staged((size_t)T::BYTES);
    for (int y0 = 0; y0 < height; y0 += T::ROWS)
        for (int x0 = 0; x0 < width; x0 += 256) {
            memset(staged.data(), 0xEE, staged.size());
            const bool interior = gray_tile_interior<T>(d, x0, y0);
            for (int q = 0; q < T::NCHUNK; ++q) {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                gray_tile_chunk<T>(mem, d, x0, y0, interior, q, w);
                memcpy(&staged[(size_t)q * 16], w, 16);
            }
            if (mem.bad) {
                printf("FAIL: out-of-span access at plane offset %lld (span %lld): sample bytes %d mis %d %dx%d pitch %lld "
                       "tile (%d,%d)\n",
                       mem.bad_off, mem.span, SB, mis0, width, height, d.pitch, x0, y0);
                return 1;
            }
            // phase A reads [mis, mis + row bytes) of every staged tile row
            for (int ly = 0; ly < T::ROWS; ++ly) {
                const int py = y0 + ly;
                const int mis = surf_misalign32(mem.base, (uint32_t)d.pitch, SB, x0, py);
                const long long start = surf_row_start(d.pitch, SB, x0, py);
                for (int k = 0; k < T::RB; ++k) {
                    const uint8_t got = staged[(size_t)(T::row(ly) + mis + k)];
                    const uint8_t want = py < height && x0 + k / SB < width ? mem.at(start + k) : 0;
                    ++checked;
                    if (got != want) {
                        printf("FAIL: staged byte %d of row %d is %u, expected %u: sample bytes %d mis %d %dx%d pitch %lld "
                               "tile (%d,%d)\n",
                               k, py, got, want, SB, mis0, width, height, d.pitch, x0, y0);
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
    // widths around the 256-column tile; 768 x 24: a middle tile on the interior path
    const int widths[] = {1, 5, 7, 253, 255, 256, 257, 511, 513, 768};
    const int heights[] = {1, 2, 8, 9, 17, 24};
    const long long extras[] = {0, 1, 13};  // samples
    long long frames = 0;
    for (int mis = 0; mis < 16; ++mis)
        for (int width : widths)
            for (int height : heights)
                for (long long e : extras) {
                    if (run<1>(mis, width, height, e, widen) || run<2>(mis, width, height, e, widen) ||
                        run<4>(mis, width, height, e, widen))
                        return 1;
                    frames += 3;
                }
    printf("ok: %lld frames, %lld staged bytes checked\n", frames, checked);
    return 0;
}
