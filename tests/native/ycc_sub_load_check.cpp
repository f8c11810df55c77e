// CPU unit check of k_front_ycc_sub's staging (csrc/ycc_load.hpp's YccTile with the
// planes' own rates SHR, SVR, the kernel's own header compiled for the host): chroma
// planes finer than the file -- 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0, 4:2:2 -> 4:2:0 -- with
// uint8 and uint16 samples.  Every tile of small frames is loaded the way the kernel
// does it -- ycc_tile_interior, then ycc_tile_chunk for every chunk with the pad codes
// -- from one byte array per plane that records each access.
//  * no byte outside a plane's [base, base + span) is touched, the spans being those of
//    the planes' sampling: a chroma plane is ceil(W / SHR) x ceil(H / SVR);
//  * a tile the loader calls interior is fetched with whole 16-byte loads only, and
//    768 x 48 frames have such tiles;
//  * from its first sample on, a staged luma tile row holds the row's samples inside
//    the rectangle followed by the luma pad code; each of a chroma plane's 8 * VR / SVR
//    staged tile rows holds the 256 / SHR positions' samples inside the planes'
//    rectangle followed by the chroma pad code, and the tile rows below a plane's last
//    row hold the pad code only, although no sample around the rectangles is a pad
//    code here.
// usage: ycc_sub_load_check [--no-span-check]
//   --no-span-check: the loader is given spans 64 bytes too large (the bound
//   widened on purpose); the check must report the out-of-span address, exit 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dmmt-jpeg-encoder_amd/csrc/ycc_load.hpp"

using namespace dmmt;

namespace {

// the pad codes: uint8 limited range's (16, 128), P010 limited range's (64 << 6, 512 << 6)
template <int SB>
struct Pad;
template <>
struct Pad<1> {
    static constexpr uint32_t luma = 16u, chroma = 128u, rep = 0x01010101u;
};
template <>
struct Pad<2> {
    static constexpr uint32_t luma = 64u << 6, chroma = 512u << 6, rep = 0x00010001u;
};

struct Memory {
    std::vector<uint8_t> bytes;  // [lead | span | trail], no sample a pad code
    long long lead = 64, span = 0;
    uint32_t base = 0;  // the plane's address (only its low bits matter)
    mutable long long bad_off = 0, byte_loads = 0;
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
        ++byte_loads;
        return bytes[(size_t)(lead + off)];
    }
    uint32_t base_lo() const { return base; }
    template <int SB>
    uint32_t at(long long off) const {  // the sample at a plane offset
        uint32_t s = bytes[(size_t)(lead + off)];
        if (SB == 2) s |= (uint32_t)bytes[(size_t)(lead + off + 1)] << 8;
        return s;
    }
};
struct Mems {
    const Memory* m[3];
    const Memory& plane(int p) const { return *m[p]; }
};

uint32_t rng_state = 24680u;
template <int SB>
void fill(Memory& m, long long span, long long widen, uint32_t base) {
    m.span = span, m.base = base, m.bad = 0, m.byte_loads = 0;
    m.bytes.resize((size_t)(64 + span + 64 + widen));
    for (size_t i = 0; i + SB <= m.bytes.size(); i += SB) {
        rng_state = rng_state * 1664525u + 1013904223u;
        uint32_t s = (rng_state >> 16) & (SB == 1 ? 0xFFu : 0xFFFFu);
        if (s == Pad<SB>::luma || s == Pad<SB>::chroma) s = SB == 1 ? 0xFFu : 0xFFFFu;
        m.bytes[i] = (uint8_t)s;
        if (SB == 2) m.bytes[i + 1] = (uint8_t)(s >> 8);
    }
}

long long checked = 0, interior_tiles = 0;

template <int SB>
uint32_t staged_at(const std::vector<uint8_t>& staged, int off) {
    uint32_t s = staged[(size_t)off];
    if (SB == 2) s |= (uint32_t)staged[(size_t)off + 1] << 8;
    return s;
}

// one frame: every tile, as k_front_ycc_sub's load_tile and its staging stores
template <int HR, int VR, int SHR, int SVR, bool NV, int SB>
int run(const int (&mis0)[3], int width, int height, long long lpitch_extra, long long cpitch_extra, long long widen) {
    using T = YccTile<HR, VR, NV, SB, SHR, SVR>;
    static_assert(T::CPX == 256 / SHR && T::CROWS == 8 * VR / SVR, "a plane's tile rows follow the planes' rates");
    static_assert(T::NCHUNK == T::ROWS * T::LRC + T::CROWS * T::NCPL * T::CRC && T::NCHUNK <= 1584, "the tile's chunks");
    static_assert(YccTile<2, 2, false, 2, 1, 1>::NCHUNK == 1584 && YccTile<2, 2, true, 2, 1, 1>::NQ == 7,
                  "the largest tile: 4:4:4 -> 4:2:0 of uint16 samples");
    YccDesc d;
    d.width = width, d.height = height;
    d.cw = (width + SHR - 1) / SHR, d.ch = (height + SVR - 1) / SVR;  // the planes' rectangle
    d.luma_pitch = (long long)width * SB + lpitch_extra;
    d.chroma_pitch = (long long)d.cw * T::CBPP + cpitch_extra;
    const long long lspan = (long long)(height - 1) * d.luma_pitch + (long long)width * SB;
    const long long cspan = (long long)(d.ch - 1) * d.chroma_pitch + (long long)d.cw * T::CBPP;
    d.luma_span = lspan + widen, d.chroma_span = cspan + widen;  // what the loader is told
    Memory mem[3];
    fill<SB>(mem[0], lspan, widen, 0x1000u + (uint32_t)mis0[0]);
    fill<SB>(mem[1], cspan, widen, 0x2000u + (uint32_t)mis0[1]);
    fill<SB>(mem[2], cspan, widen, 0x3000u + (uint32_t)mis0[2]);
    const Mems ms{{&mem[0], &mem[1], NV ? &mem[1] : &mem[2]}};
    const uint32_t lfill = Pad<SB>::luma * Pad<SB>::rep, cfill = Pad<SB>::chroma * Pad<SB>::rep;
    std::vector<uint8_t> staged((size_t)T::BYTES);
    for (int y0 = 0; y0 < height; y0 += T::ROWS)
        for (int x0 = 0; x0 < width; x0 += 256) {
            memset(staged.data(), 0xEE, staged.size());
            const bool interior = ycc_tile_interior<T>(d, x0, y0);
            const long long before = mem[0].byte_loads + mem[1].byte_loads + mem[2].byte_loads;
            for (int q = 0; q < T::NCHUNK; ++q) {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                ycc_tile_chunk<T>(ms, d, x0, y0, interior, q, w, lfill, cfill);
                memcpy(&staged[(size_t)q * 16], w, 16);
            }
            for (int p = 0; p < 3; ++p)
                if (mem[p].bad) {
                    printf("FAIL: out-of-span access at plane offset %lld (plane %d, span %lld): mis %d/%d/%d %dx%d "
                           "hr %d vr %d shr %d svr %d nv %d sb %d pitches %lld/%lld tile (%d,%d)\n",
                           mem[p].bad_off, p, mem[p].span, mis0[0], mis0[1], mis0[2], width, height, HR, VR, SHR, SVR,
                           (int)NV, SB, d.luma_pitch, d.chroma_pitch, x0, y0);
                    return 1;
                }
            if (interior) {
                ++interior_tiles;
                if (mem[0].byte_loads + mem[1].byte_loads + mem[2].byte_loads != before) {
                    printf("FAIL: byte loads on an interior tile: %dx%d hr %d vr %d shr %d nv %d sb %d tile (%d,%d)\n", width,
                           height, HR, VR, SHR, (int)NV, SB, x0, y0);
                    return 1;
                }
            }
            // phase A reads [mis, mis + row bytes) of every staged tile row
            for (int ly = 0; ly < T::ROWS; ++ly) {
                const int py = y0 + ly;
                const int mis = surf_misalign32(mem[0].base, (uint32_t)d.luma_pitch, SB, x0, py);
                const long long start = surf_row_start(d.luma_pitch, SB, x0, py);
                for (int k = 0; k < 256; ++k) {
                    const uint32_t got = staged_at<SB>(staged, T::luma_row(ly) + mis + SB * k);
                    const uint32_t want = py < height && x0 + k < width ? mem[0].at<SB>(start + SB * k) : Pad<SB>::luma;
                    ++checked;
                    if (got != want) {
                        printf("FAIL: staged luma sample %d of row %d is %u, expected %u: mis %d %dx%d hr %d vr %d shr %d nv %d "
                               "sb %d pitch %lld tile (%d,%d)\n",
                               k, py, got, want, mis0[0], width, height, HR, VR, SHR, (int)NV, SB, d.luma_pitch, x0, y0);
                        return 1;
                    }
                }
            }
            const int cx0 = x0 / SHR;
            for (int cp = 0; cp < T::NCPL; ++cp)
                for (int r = 0; r < T::CROWS; ++r) {
                    const Memory& m = mem[1 + cp];
                    const int cy = y0 / SVR + r;
                    const int mis = surf_misalign32(m.base, (uint32_t)d.chroma_pitch, T::CBPP, cx0, cy);
                    const long long start = surf_row_start(d.chroma_pitch, T::CBPP, cx0, cy);
                    for (int k = 0; k < T::CRB / SB; ++k) {  // samples: two per position with NV
                        const uint32_t got = staged_at<SB>(staged, T::chroma_row(cp, r) + mis + SB * k);
                        const bool inside = cy < d.ch && cx0 + k * SB / T::CBPP < d.cw;
                        const uint32_t want = inside ? m.at<SB>(start + SB * k) : Pad<SB>::chroma;
                        ++checked;
                        if (got != want) {
                            printf("FAIL: staged chroma sample %d of row %d (plane %d) is %u, expected %u: mis %d %dx%d "
                                   "hr %d vr %d shr %d nv %d sb %d pitch %lld tile (%d,%d)\n",
                                   k, cy, 1 + cp, got, want, mis0[1 + cp], width, height, HR, VR, SHR, (int)NV, SB,
                                   d.chroma_pitch, x0, y0);
                            return 1;
                        }
                    }
                }
        }
    return 0;
}

// the three converting pairs, planar and pair planes
template <int SB>
int run_pairs(const int (&mis0)[3], int w, int h, long long le, long long ce, long long widen) {
    return run<2, 1, 1, 1, false, SB>(mis0, w, h, le, ce, widen) || run<2, 1, 1, 1, true, SB>(mis0, w, h, le, ce, widen) ||
           run<2, 2, 1, 1, false, SB>(mis0, w, h, le, ce, widen) || run<2, 2, 1, 1, true, SB>(mis0, w, h, le, ce, widen) ||
           run<2, 2, 2, 1, false, SB>(mis0, w, h, le, ce, widen) || run<2, 2, 2, 1, true, SB>(mis0, w, h, le, ce, widen);
}

}  // namespace

int main(int argc, char** argv) {
    const long long widen = argc > 1 && !strcmp(argv[1], "--no-span-check") ? 64 : 0;
    // luma widths around the 256-column tile (4:2:2 planes: chroma widths around 128) and 512;
    // 768 x 48: middle tiles on the interior path
    const int widths[] = {1, 5, 253, 254, 255, 256, 257, 511, 513, 768};
    const int heights[] = {1, 2, 3, 17, 48};
    long long frames = 0;
    for (int mis = 0; mis < 16; ++mis) {
        // another misalignment per plane; uint16 planes lie at even addresses
        const int m8[3] = {mis, (5 * mis + 7) & 15, (11 * mis + 10) & 15};
        const int m16[3] = {mis & 14, (5 * mis + 6) & 14, (11 * mis + 10) & 14};
        for (int width : widths)
            for (int height : heights)
                for (int e = 0; e < 3; ++e) {
                    const long long x8[] = {0, 1, 16}, x16[] = {0, 2, 16};
                    const int e2 = (e + 1 + mis / 2) % 3;  // the pitches differ
                    if (run_pairs<1>(m8, width, height, x8[e], x8[e2], widen)) return 1;
                    frames += 6;
                    if (mis % 2 == 0) {
                        if (run_pairs<2>(m16, width, height, x16[e], x16[e2], widen)) return 1;
                        frames += 6;
                    }
                }
    }
    if (!interior_tiles) {
        printf("FAIL: no tile took the interior path\n");
        return 1;
    }
    printf("ok: %lld frames, %lld interior tiles, %lld staged samples checked\n", frames, interior_tiles, checked);
    return 0;
}
