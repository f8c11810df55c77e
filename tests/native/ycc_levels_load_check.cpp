// CPU unit check of k_front_ycc_lv's staging for uint16 samples (csrc/ycc_load.hpp
// with SB = 2, the kernel's own header compiled for the host): every tile of small
// YCbCr frames is loaded the way the kernel does it -- ycc_tile_interior, then
// ycc_tile_chunk for every chunk with the pad codes -- from one byte array per plane
// that records each access.  Plane addresses, pitches and so every offset are even.
//  * no byte outside a plane's [base, base + span) is touched;
//  * from its first sample on, a staged luma tile row holds the row's samples inside
//    the rectangle followed by the luma pad code, a staged chroma tile row the row's
//    samples followed by the chroma pad code, and the tile rows below the plane's last
//    row hold the pad code only, although the samples around the rectangles are never
//    a pad code here.  The pad codes are P010 limited range's: (64 << 6, 512 << 6).
// usage: ycc_levels_load_check [--no-span-check]
//   --no-span-check: the loader is given spans 64 bytes too large (the bound
//   widened on purpose); the check must report the out-of-span address, exit 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dmmt-jpeg-encoder_amd/csrc/ycc_load.hpp"

using namespace dmmt;

namespace {

constexpr int SB = 2;
constexpr uint16_t kLumaPad = 64u << 6, kChromaPad = 512u << 6;
constexpr uint32_t kLumaFill = kLumaPad * 0x00010001u, kChromaFill = kChromaPad * 0x00010001u;

struct Memory {
    std::vector<uint8_t> bytes;  // [lead | span | trail], no sample a pad code
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
    uint16_t at(long long off) const {  // the sample at an (even) plane offset
        uint16_t s;
        memcpy(&s, &bytes[(size_t)(lead + off)], 2);
        return s;
    }
};
struct Mems {
    const Memory* m[3];
    const Memory& plane(int p) const { return *m[p]; }
};

uint32_t rng_state = 54321u;
uint16_t next_sample() {
    rng_state = rng_state * 1664525u + 1013904223u;
    const uint16_t s = (uint16_t)(rng_state >> 16);
    return s == kLumaPad || s == kChromaPad ? 0xFFFF : s;
}
void fill(Memory& m, long long span, long long widen, uint32_t base) {
    m.span = span, m.base = base, m.bad = 0;
    m.bytes.resize((size_t)(64 + span + 64 + widen));
    for (size_t i = 0; i + 1 < m.bytes.size(); i += 2) {
        const uint16_t s = next_sample();
        memcpy(&m.bytes[i], &s, 2);
    }
}

long long checked = 0;

uint16_t staged_at(const std::vector<uint8_t>& staged, int off) {
    uint16_t s;
    memcpy(&s, &staged[(size_t)off], 2);
    return s;
}

// one frame: every tile, as k_front_ycc_lv's load_tile and its staging stores
template <int HR, int VR, bool NV>
int run(const int (&mis0)[3], int width, int height, long long lpitch_extra, long long cpitch_extra, long long widen) {
    using T = YccTile<HR, VR, NV, SB>;
    static_assert(T::LRB == 512 && T::LRC == 33, "a uint16 luma tile row: 512 bytes, 33 chunks");
    YccDesc d;
    d.width = width, d.height = height;
    d.cw = (width + HR - 1) / HR, d.ch = (height + VR - 1) / VR;
    d.luma_pitch = (long long)width * SB + lpitch_extra;
    d.chroma_pitch = (long long)d.cw * T::CBPP + cpitch_extra;
    const long long lspan = (long long)(height - 1) * d.luma_pitch + (long long)width * SB;
    const long long cspan = (long long)(d.ch - 1) * d.chroma_pitch + (long long)d.cw * T::CBPP;
    d.luma_span = lspan + widen, d.chroma_span = cspan + widen;  // what the loader is told
    Memory mem[3];
    fill(mem[0], lspan, widen, 0x1000u + (uint32_t)mis0[0]);
    fill(mem[1], cspan, widen, 0x2000u + (uint32_t)mis0[1]);
    fill(mem[2], cspan, widen, 0x3000u + (uint32_t)mis0[2]);
    const Mems ms{{&mem[0], &mem[1], NV ? &mem[1] : &mem[2]}};
    std::vector<uint8_t> staged((size_t)T::BYTES);
    for (int y0 = 0; y0 < height; y0 += T::ROWS)
        for (int x0 = 0; x0 < width; x0 += 256) {
            memset(staged.data(), 0xEE, staged.size());
            const bool interior = ycc_tile_interior<T>(d, x0, y0);
            for (int q = 0; q < T::NCHUNK; ++q) {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                ycc_tile_chunk<T>(ms, d, x0, y0, interior, q, w, kLumaFill, kChromaFill);
                memcpy(&staged[(size_t)q * 16], w, 16);
            }
            for (int p = 0; p < 3; ++p)
                if (mem[p].bad) {
                    printf("FAIL: out-of-span access at plane offset %lld (plane %d, span %lld): mis %d/%d/%d %dx%d "
                           "hr %d vr %d nv %d pitches %lld/%lld tile (%d,%d)\n",
                           mem[p].bad_off, p, mem[p].span, mis0[0], mis0[1], mis0[2], width, height, HR, VR, (int)NV,
                           d.luma_pitch, d.chroma_pitch, x0, y0);
                    return 1;
                }
            // phase A reads [mis, mis + row bytes) of every staged tile row
            for (int ly = 0; ly < T::ROWS; ++ly) {
                const int py = y0 + ly;
                const int mis = surf_misalign32(mem[0].base, (uint32_t)d.luma_pitch, SB, x0, py);
                const long long start = surf_row_start(d.luma_pitch, SB, x0, py);
                for (int k = 0; k < 256; ++k) {
                    const uint16_t got = staged_at(staged, T::luma_row(ly) + mis + SB * k);
                    const uint16_t want = py < height && x0 + k < width ? mem[0].at(start + SB * k) : kLumaPad;
                    ++checked;
                    if (got != want) {
                        printf("FAIL: staged luma sample %d of row %d is %u, expected %u: mis %d %dx%d hr %d vr %d nv %d "
                               "pitch %lld tile (%d,%d)\n",
                               k, py, got, want, mis0[0], width, height, HR, VR, (int)NV, d.luma_pitch, x0, y0);
                        return 1;
                    }
                }
            }
            const int cx0 = x0 / HR;
            for (int cp = 0; cp < T::NCPL; ++cp)
                for (int r = 0; r < 8; ++r) {
                    const Memory& m = mem[1 + cp];
                    const int cy = y0 / VR + r;
                    const int mis = surf_misalign32(m.base, (uint32_t)d.chroma_pitch, T::CBPP, cx0, cy);
                    const long long start = surf_row_start(d.chroma_pitch, T::CBPP, cx0, cy);
                    for (int k = 0; k < T::CRB / SB; ++k) {  // samples: two per position with NV
                        const uint16_t got = staged_at(staged, T::chroma_row(cp, r) + mis + SB * k);
                        const bool inside = cy < d.ch && cx0 + k * SB / T::CBPP < d.cw;
                        const uint16_t want = inside ? m.at(start + SB * k) : kChromaPad;
                        ++checked;
                        if (got != want) {
                            printf("FAIL: staged chroma sample %d of row %d (plane %d) is %u, expected %u: mis %d %dx%d "
                                   "hr %d vr %d nv %d pitch %lld tile (%d,%d)\n",
                                   k, cy, 1 + cp, got, want, mis0[1 + cp], width, height, HR, VR, (int)NV,
                                   d.chroma_pitch, x0, y0);
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
    // luma widths around the 256-column tile, chroma widths around 128 (253..257 halved) and 256;
    // 768 x 48: middle tiles on the interior path
    const int widths[] = {1, 5, 253, 254, 255, 256, 257, 511, 513, 768};
    const int heights[] = {1, 2, 3, 17, 48};
    const long long extras[] = {0, 2, 16};
    long long frames = 0;
    for (int mis = 0; mis < 16; mis += 2) {
        const int mis0[3] = {mis, (5 * mis + 6) & 14, (11 * mis + 10) & 14};  // another (even) one per plane
        for (int width : widths)
            for (int height : heights)
                for (int e = 0; e < 3; ++e) {
                    const long long le = extras[e], ce = extras[(e + 1 + mis / 2) % 3];  // the pitches differ
                    if (run<1, 1, false>(mis0, width, height, le, ce, widen) || run<1, 1, true>(mis0, width, height, le, ce, widen) ||
                        run<2, 1, false>(mis0, width, height, le, ce, widen) || run<2, 1, true>(mis0, width, height, le, ce, widen) ||
                        run<2, 2, false>(mis0, width, height, le, ce, widen) || run<2, 2, true>(mis0, width, height, le, ce, widen))
                        return 1;
                    frames += 6;
                }
    }
    printf("ok: %lld frames, %lld staged samples checked\n", frames, checked);
    return 0;
}
