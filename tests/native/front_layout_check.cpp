// CPU check of the front kernels' LDS layout of the row-transformed blocks (sT):
// csrc/front_layout.hpp, the kernels' own header, compiled for the host.  For every
// FrontGeom in use (4:4:4 compact, the layout of the uint8 4:4:4 kernels, and
// 4:4:4, 4:2:2, 4:2:0, gray padded; the compact form of the other geometries is
// checked too, in case a kernel takes it up):
//  * (block, row, column) -> st_at is injective into [0, ST_FLOATS), st_quad is the
//    16-byte aligned start of a row's half and agrees with st_at, st_second_half and
//    st_row_of_column give what their names say;
//  * the lane sets of every phase A row store (ds_write_b128: lanes in 8 groups of 8
//    contiguous, bank = dword address mod 32, four banks per lane) and of every
//    phase C column read (ds_read_b32: lanes {0-31}, {32-63}, bank = dword address
//    mod 32) cost no more bank-conflict cycles than the layout this one replaced did
//    for the same lanes: 72 floats per block, block b from 72 b + 4 f(b), kept below
//    as old_at.  A group's extra cycles: the largest number of distinct addresses on
//    one bank, less one.
// The lane sets are those of the kernel bodies: thread tid of phase A takes
// h = tid % HR, job = tid / HR, chroma block c = job % CB and chroma row r = job / CB
// (gray: c = tid & 31, r = tid >> 5), stores its VR luma rows r * VR + dy of block
// (ly >> 3) * 32 + c * HR + h and row r of Cb and of Cr block c (4:4:4: one store
// each; 4:2:x: h = 0 Cb, h = 1 Cr); thread tid of phase C reads column tid & 7 of
// block (tid >> 3) + 32 jj, row by row.
// Prints one line per geometry; exit status 1 on any failure.
#include <stdio.h>

#include <algorithm>
#include <set>
#include <vector>

#include "../../dmmt-jpeg-encoder_amd/csrc/front_layout.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (++g_fail < 20) {             \
                fprintf(stderr, __VA_ARGS__); \
                fputc('\n', stderr);         \
            }                                \
        }                                    \
    } while (0)

// the padded layout before this one
template <class G>
int old_at(int b, int r, int c) {
    const int skew = 4 * (((b >> 2) ^ (G::NCOMP == 3 && b >= G::NYB + G::CB ? 1 : 0)) & 1);
    return b * 72 + skew + r * 8 + c;
}

// extra LDS cycles of one lane group: each lane covers `width` dwords from its address
int group_extra(const std::vector<int>& addr, int width) {
    std::set<int> on_bank[32];
    for (int a : addr)
        for (int k = 0; k < width; ++k) on_bank[(a + k) % 32].insert(a + k);
    size_t worst = 1;
    for (const auto& s : on_bank) worst = std::max(worst, s.size());
    return (int)worst - 1;
}

struct Cost {
    int fresh = 0, old = 0, instructions = 0;
};

// one wave-wide instruction: addr[lane] for the 64 lanes, split into groups of `group` contiguous lanes
void account(const int (&fresh)[64], const int (&old)[64], int group, int width, Cost& cost, const char* what) {
    int f = 0, o = 0;
    for (int l0 = 0; l0 < 64; l0 += group) {
        f += group_extra(std::vector<int>(fresh + l0, fresh + l0 + group), width);
        o += group_extra(std::vector<int>(old + l0, old + l0 + group), width);
    }
    CHECK(f <= o, "%s: %d conflict cycles, the padded layout %d", what, f, o);
    cost.fresh += f, cost.old += o, ++cost.instructions;
}

template <class G>
void check(const char* name) {
    // addresses
    std::vector<int> seen(G::ST_FLOATS, 0);
    for (int b = 0; b < G::NB; ++b)
        for (int r = 0; r < 8; ++r) {
            for (int h = 0; h < 2; ++h) {
                const int q = G::st_quad(b, r, h);
                CHECK(q % 4 == 0, "%s: st_quad(%d, %d, %d) = %d is not 16-byte aligned", name, b, r, h, q);
                CHECK(h == 1 || G::st_second_half(q) == G::st_quad(b, r, 1), "%s: st_second_half at (%d, %d, %d)", name, b, r, h);
                for (int k = 0; k < 4; ++k)
                    CHECK(G::st_at(b, r, 4 * h + k) == q + k, "%s: st_at(%d, %d, %d) off its quad", name, b, r, 4 * h + k);
            }
            for (int c = 0; c < 8; ++c) {
                const int a = G::st_at(b, r, c);
                CHECK(a >= 0 && a < G::ST_FLOATS, "%s: st_at(%d, %d, %d) = %d outside sT", name, b, r, c, a);
                if (a >= 0 && a < G::ST_FLOATS) CHECK(!seen[a]++, "%s: st_at(%d, %d, %d) = %d taken twice", name, b, r, c, a);
                CHECK(G::st_row_of_column(G::st_at(b, 0, c), r) == a, "%s: st_row_of_column at (%d, %d, %d)", name, b, r, c);
            }
        }
    CHECK(!G::COMPACT || G::ST_FLOATS == G::NB * 64, "%s: sT has padding", name);
    CHECK(G::COMPACT || G::ST_FLOATS == G::NB * 72 + 4, "%s: the padded sT changed size", name);

    // phase A: the row stores, one instruction per (wave, stored row, half)
    Cost store, load;
    for (int wave = 0; wave < 4; ++wave) {
        // the rows a thread stores: (block, row) per store site
        auto sites = [&](int tid, std::vector<std::pair<int, int>>& out) {
            out.clear();
            if (G::NCOMP == 1) {
                out.push_back({tid & 31, tid >> 5});
                return;
            }
            const int h = tid % G::HR, job = tid / G::HR, c = job % G::CB, r = job / G::CB;
            for (int dy = 0; dy < G::VR; ++dy) {
                const int ly = r * G::VR + dy;
                out.push_back({(ly >> 3) * 32 + c * G::HR + h, ly & 7});
            }
            if (G::HR == 1) {
                out.push_back({G::NYB + c, r});
                out.push_back({G::NYB + G::CB + c, r});
            } else {
                out.push_back({G::NYB + h * G::CB + c, r});
            }
        };
        std::vector<std::pair<int, int>> s[64];
        for (int l = 0; l < 64; ++l) sites(wave * 64 + l, s[l]);
        for (size_t k = 0; k < s[0].size(); ++k)
            for (int h = 0; h < 2; ++h) {
                int fresh[64], old[64];
                for (int l = 0; l < 64; ++l) {
                    CHECK(s[l][k].first < G::NB && s[l][k].second < 8, "%s: store site outside the tile", name);
                    fresh[l] = G::st_quad(s[l][k].first, s[l][k].second, h);
                    old[l] = old_at<G>(s[l][k].first, s[l][k].second, 4 * h);
                }
                account(fresh, old, 8, 4, store, name);
            }
        // phase C: the column reads, one instruction per (wave, column job, row)
        for (int jj = 0; jj < G::JPT; ++jj)
            for (int r = 0; r < 8; ++r) {
                int fresh[64], old[64];
                for (int l = 0; l < 64; ++l) {
                    const int tid = wave * 64 + l, blk = (tid + 256 * jj) >> 3, col = tid & 7;
                    fresh[l] = G::st_at(blk, r, col);
                    old[l] = old_at<G>(blk, r, col);
                }
                account(fresh, old, 32, 1, load, name);
            }
    }
    printf("%s blocks %d floats %d stores %d conflicts %d padded %d reads %d conflicts %d padded %d\n", name, G::NB,
           G::ST_FLOATS, store.instructions, store.fresh, store.old, load.instructions, load.fresh, load.old);
}

}  // namespace

int main() {
    check<dmmt::FrontGeom<1, 1, 3, true>>("444c");  // uint8 4:4:4: the compact layout
    check<dmmt::FrontGeom<1, 1>>("444");
    check<dmmt::FrontGeom<2, 1>>("422");
    check<dmmt::FrontGeom<2, 2>>("420");
    check<dmmt::FrontGeom<1, 1, 1>>("gray");
    check<dmmt::FrontGeom<2, 1, 3, true>>("422c");
    check<dmmt::FrontGeom<2, 2, 3, true>>("420c");
    check<dmmt::FrontGeom<1, 1, 1, true>>("grayc");
    if (g_fail) fprintf(stderr, "%d checks failed\n", g_fail);
    return g_fail ? 1 : 0;
}
