// front_ycc_sub.hip -- k_front_ycc_sub: the YCbCr front kernel for planes that lie at
// a finer chroma sampling than the file is written with
// (dmmt_encode_device_ycc_subsample): 4:4:4 planes to a 4:2:2 or a 4:2:0 file, 4:2:2
// planes to a 4:2:0 file.  Everything that is not named here is front_ycc.hip's: the
// three kinds of input (plain, levels, matrix: front_ycc_common.hpp), the formats, the
// transfer, the matrix step, the range vote, the tile loop, the column pass.
//
// With (SHR, SVR) the planes' rates, (HR, VR) the file's, RX = HR / SHR and RY =
// VR / SVR -- (2, 1), (2, 2) or (1, 2); the file's HR is 2 and the planes' SVR is 1 in
// all three pairs -- the values are, at the planes' own sampling, what k_front_ycc
// feeds the DCT for planes of that sampling: transferred, and with a matrix Y', Cb',
// Cr', the luma sample at (x, y) taking the chroma position (x / SHR, y / SVR); padded
// black after that step, luma -128 outside W x H up to the file's MCU multiple Wp x
// Hp, chroma 0 outside ceil(W / SHR) x ceil(H / SVR) up to (Wp / SHR) x (Hp / SVR).
// Luma goes on as it is.  Each chroma plane p(x, y) is box-averaged to the file's
// sampling the way the reference subsamples the chroma of RGB pixels
// (subsampling.rs:102-236: x outer, y inner, the sum then divided by the count), in
// f32, every operation rounded once:
//   (2, 1)  (p(2i, j) + p(2i+1, j)) / 2
//   (1, 2)  (p(i, 2j) + p(i, 2j+1)) / 2
//   (2, 2)  (((p(2i, 2j) + p(2i, 2j+1)) + p(2i+1, 2j)) + p(2i+1, 2j+1)) / 4
// An odd plane width or height averages its last sample with the padding's 0, as the
// reference averages a padded pixel; the count is always RX * RY.
//
// The loader stages that padding by itself: YccTile<HR, VR, NV, SB, SHR, SVR>
// (ycc_load.hpp) holds 8 * RY chroma tile rows of 256 / SHR positions per plane, and
// what lies past the planes' rectangle is the pad code, which transfers to 0 -- and
// the matrix takes cb = cr = 0 to Cb' = Cr' = 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dct_quant.hpp"
#include "device_common.hpp"
#include "front_common.hpp"
#include "front_launch.hpp"
#include "front_ycc_common.hpp"
#include "jpeg_common.hpp"
#include "kernels.hpp"
#include "ycc_load.hpp"

namespace dmmt {

// front_ycc_body's shape (front_ycc.hip): one workgroup per tile of 256 luma columns
// by 8 * VR luma rows, a grid-stride loop with the next tile prefetched, FrontGeom's sT
// layout and front_column_pass, so the coefficients land where k_hist expects them.
//  staging  8 * VR luma tile rows, then per chroma plane 8 * RY tile rows of 256 / SHR
//     positions.  The largest tile, 4:4:4 -> 4:2:0 of uint16 samples, is 1584 chunks:
//     seven per thread, 25.3 KB.
//  A  the same jobs: one thread per (chroma row r of the file, chroma block c, luma
//     block column h = 0, 1).  Luma tile row r * VR + dy and the planes' chroma tile row
//     of the same index lie under each other (SVR = 1).
//     luma  the job's VR rows of 8 samples -- transfer, row pass -- as front_ycc_body.
//       matrix: first both components of the 8 / SHR plane positions under the thread's
//       own 8 luma columns, read at an LDS address that depends on h (choosing by h
//       among the elements of a wider array would index it, and put it into scratch),
//       transferred; Y' with position k / SHR of them, -128 at or past the rectangle's
//       edge.
//     chroma  the thread's component (h = 0: Cb, h = 1: Cr) at the 8 * RX plane positions
//       under the block's chroma row, in RX groups of 8 positions so that few values are
//       live at a time: per group the RY rows -- plain, levels: the component,
//       transferred; matrix: both components, transferred, the thread's one mixed and
//       clamped: the matrix runs at the planes' positions, before the average -- then
//       the 8 / RX averages in the order above.  Then the row pass and the store into
//       the component's block.
//     Every thread reads the positions it averages from LDS; no lane exchange.  (k_front's
//     pair exchanges four averaged samples over DPP because each lane had computed half
//     of both rows from its own pixels.  Here the samples are staged: the exchange would
//     save a thread half of its chroma reads and transfers, and cost it both components'
//     averages, eight selects and four DPP moves; with the matrix, where the luma rows
//     read their positions a second time, the kernel keeps within its registers only
//     because the two steps share no values.)
//  range vote  as front_ycc_body: every code a thread unpacks is of the planes'
//     rectangles or a pad code, and every sample of the rectangles is unpacked by some
//     thread (plain and levels: component h by thread h; matrix: both by both).
//  C, D  front_column_pass's integer-sample path.  Its bound (dct_quant.hpp,
//     quantize_col8_scaled) needs the DCT's inputs in [-128, 127].  Luma: as
//     front_ycc_body.  Chroma: every averaged value lies in [-128, 127] -- plain:
//     integers; levels: the transfer's clamps; matrix: ycc_clamp; the padding 0 --
//     each f32 addition is a monotone rounding, so a partial sum of n values lies in
//     [-128 n, 127 n] (both exact floats), the total in [-128 RX RY, 127 RX RY], and
//     the division by RX * RY = 2 or 4 is exact: the result lies in [-128, 127].  So
//     |DC| <= 1024 and |AC| <= 2048 to within a few ulps as before, `as i16` cannot
//     saturate and no NaN can arise (nan_possible = false).
template <int HR, int VR, int SHR, int FMT, int SB, bool NARROW, class Args>
__device__ __forceinline__ void front_ycc_sub_body(const Args& ya, size_t frame_stride, const Geom& g,
                                                   const float* __restrict__ qtab,  // [2][64] natural, as f32
                                                   int16_t* __restrict__ coef, int* __restrict__ status,
                                                   int16_t* __restrict__ coef_lo, int8_t* __restrict__ coef_hi) {
    constexpr int IN = Args::IN;
    static_assert(IN != YCC_IN_PLAIN || SB == 1, "plain frames are uint8");
    constexpr int SVR = 1, RX = HR / SHR, RY = VR / SVR;
    static_assert(HR == 2 && RX * RY > 1 && RY == VR, "4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0 or 4:2:2 -> 4:2:0");
    constexpr bool NV = FMT != YCC_PLANAR;
    constexpr int VU = FMT == YCC_NV_VU ? 1 : 0;
    using T = YccTile<HR, VR, NV, SB, SHR, SVR>;
    using G = FrontGeom<HR, VR>;  // the tile's blocks (front_common.hpp)
    constexpr int NYB = G::NYB, CB = G::CB;
    constexpr int P = 8 * RX;    // plane positions under a chroma block's row
    constexpr int NL = 8 / SHR;  // plane positions under a thread's 8 luma columns
    static_assert(8 * CB * HR == 256, "one phase-A job per thread");

    __shared__ __attribute__((aligned(16))) float sT[G::ST_FLOATS];
    __shared__ __attribute__((aligned(16))) uint8_t sRaw[T::BYTES + 16];  // (+ 16: lds_words reads 3 bytes past a row)
    __shared__ float sQ[128];
    __shared__ float sRQ[128];

    const int tid = threadIdx.x;
    const int frame = blockIdx.y;
    const size_t foff = (size_t)frame * frame_stride;  // the same offset in every plane
    const YccMems ms{ya.p0 + foff, ya.p1 + foff, ya.p2 + foff};  // (NV: p2 = p1)
    const YccDesc& d = ya.d;
    YccTransfer t{};                          // (plain: not read)
    YccMatrix m{};                            // (matrix kind only)
    uint32_t shift = 0u, max_code = 0xFFFFu;  // (uint8: neither is read)
    if constexpr (IN != YCC_IN_PLAIN) t = ya.t;
    if constexpr (IN == YCC_IN_MATRIX) m = ya.m;
    if constexpr (SB == 2) shift = ya.c.shift, max_code = ya.c.max_code;
    const bool check_range = SB == 2 && (0xFFFFu >> shift) > max_code;  // (uniform)
    uint32_t vmax = 0;  // the largest code this thread unpacked
    front_fill_qtabs<G, true>(qtab, sQ, sRQ, tid);

    // sample k of a row's words: uint8 a byte, uint16 a half >> shift
    auto code = [&](const uint32_t* w, int k) -> uint32_t {
        if constexpr (SB == 1) return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        return ((w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) >> shift;
    };
    // the sample at place `first` (0, 1) of pair k of a row of pairs (uint16: a pair is one word)
    auto pair_code = [&](const uint32_t* w, int k, int first) -> uint32_t {
        if constexpr (SB == 1) return ((w[k >> 1] >> (8 * first)) >> (16 * (k & 1))) & 0xFFu;
        return ((w[k] >> (16 * first)) & 0xFFFFu) >> shift;
    };

    uint4 raw[T::NQ];
    auto load_tile = [&](int tx0, int ty0) {
        const bool interior = ycc_tile_interior<T>(d, tx0, ty0);  // (wave-uniform)
        // uint16 tiles are up to seven chunks per thread.  What a chunk's address takes from q alone
        // -- its plane, tile row and place in the row -- does not change from tile to tile; kept in
        // registers across the tile loop, for every chunk, it made these instantiations spill.  A
        // thread index the compiler cannot see through is worked out again per tile.
        int lt = tid;
        if constexpr (SB == 2) asm volatile("" : "+v"(lt));
#pragma unroll
        for (int i = 0; i < T::NQ; ++i) {
            const int q = lt + 256 * i;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (q < T::NCHUNK) {
                if constexpr (IN == YCC_IN_PLAIN)
                    ycc_tile_chunk<T>(ms, d, tx0, ty0, interior, q, w);
                else
                    ycc_tile_chunk<T>(ms, d, tx0, ty0, interior, q, w, ya.c.luma_fill, ya.c.chroma_fill);
            }
            raw[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    };
    const int tiles_per_row = (g.mcux + G::TM - 1) / G::TM;
    const int ntiles = tiles_per_row * g.mcuy;
    if ((int)blockIdx.x < ntiles) {
        const int my = blockIdx.x / tiles_per_row;
        load_tile((blockIdx.x - my * tiles_per_row) * 256, my * G::ROWS);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int my = tile / tiles_per_row;
        const int mx0 = (tile - my * tiles_per_row) * G::TM;
        const int x0 = mx0 * 8 * G::HR, y0 = my * G::ROWS;
        front_stage<T::NCHUNK>(sRaw, tid, raw);
        __syncthreads();
        {  // prefetch the next tile's bytes; they land while this tile computes
            const int nt = tile + gridDim.x;
            if (nt < ntiles) {
                const int ny = nt / tiles_per_row;
                load_tile((nt - ny * tiles_per_row) * 256, ny * G::ROWS);
            }
        }
        // ---- A: code -> full-range value[, the matrix], the chroma average, row pass (arai.rs:97-99)
        {
            const int h = tid % HR, job = tid / HR;
            const int c = job % CB, r = job / CB;  // chroma block, chroma row of the file
            const int lx0 = c * 8 * HR + 8 * h;    // first luma column of the job
            const int cx0 = x0 / SHR;              // the tile's first plane position
            // NP plane positions from position pos0 of the tile's chroma tile row ly.  matrix: both
            // components, transferred, in b and r; else the thread's component in b
            auto positions = [&](auto np, int ly, int pos0, float* b, float* rr) {
                constexpr int NP = decltype(np)::value;
                const int cy = y0 + ly;  // (SVR = 1)
                if constexpr (NV) {
                    const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p1, (uint32_t)d.chroma_pitch, 2 * SB, cx0, cy);
                    uint32_t w[NP * SB / 2];
                    lds_words<NP * SB / 2>(sRaw, T::chroma_row(0, ly) + mis + 2 * SB * pos0, w);
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        if constexpr (IN == YCC_IN_MATRIX) {
                            const uint32_t s0 = pair_code(w, k, VU), s1 = pair_code(w, k, 1 - VU);
                            if constexpr (SB == 2) vmax = max(vmax, max(s0, s1));
                            b[k] = ycc_chroma_in<IN>(s0, t), rr[k] = ycc_chroma_in<IN>(s1, t);
                        } else {
                            const uint32_t s = pair_code(w, k, h ^ VU);  // the component's place in a pair
                            if constexpr (SB == 2) vmax = max(vmax, s);
                            b[k] = ycc_chroma_in<IN>(s, t);
                        }
                    }
                } else if constexpr (IN == YCC_IN_MATRIX) {
                    const int mb = surf_misalign32((uint32_t)(uintptr_t)ms.p1, (uint32_t)d.chroma_pitch, SB, cx0, cy);
                    const int mr = surf_misalign32((uint32_t)(uintptr_t)ms.p2, (uint32_t)d.chroma_pitch, SB, cx0, cy);
                    uint32_t wb[NP * SB / 4], wr[NP * SB / 4];
                    lds_words<NP * SB / 4>(sRaw, T::chroma_row(0, ly) + mb + SB * pos0, wb);
                    lds_words<NP * SB / 4>(sRaw, T::chroma_row(1, ly) + mr + SB * pos0, wr);
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        const uint32_t s0 = code(wb, k), s1 = code(wr, k);
                        if constexpr (SB == 2) vmax = max(vmax, max(s0, s1));
                        b[k] = ycc_chroma_in<IN>(s0, t), rr[k] = ycc_chroma_in<IN>(s1, t);
                    }
                } else {
                    const uint8_t* pl = h ? ms.p2 : ms.p1;
                    const int mis = surf_misalign32((uint32_t)(uintptr_t)pl, (uint32_t)d.chroma_pitch, SB, cx0, cy);
                    uint32_t w[NP * SB / 4];
                    lds_words<NP * SB / 4>(sRaw, T::chroma_row(h, ly) + mis + SB * pos0, w);
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        const uint32_t s = code(w, k);
                        if constexpr (SB == 2) vmax = max(vmax, s);
                        b[k] = ycc_chroma_in<IN>(s, t);
                    }
                }
            };
            // the luma rows
            [[maybe_unused]] const int nx = d.width - x0 - lx0;  // the job's luma columns inside the rectangle (<= 0: none)
#pragma unroll
            for (int dy = 0; dy < VR; ++dy) {
                const int ly = r * VR + dy;
                [[maybe_unused]] float lb[NL], lr[NL];  // matrix: Cb and Cr at position k / SHR under the row
                if constexpr (IN == YCC_IN_MATRIX) positions(std::integral_constant<int, NL>{}, ly, lx0 / SHR, lb, lr);
                const int mis = surf_misalign32((uint32_t)(uintptr_t)ms.p0, (uint32_t)d.luma_pitch, SB, x0, y0 + ly);
                uint32_t w[2 * SB];
                lds_words<2 * SB>(sRaw, T::luma_row(ly) + mis + SB * lx0, w);
                [[maybe_unused]] const int nk = y0 + ly < d.height ? nx : 0;  // samples k < nk lie inside
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t s = code(w, k);
                    if constexpr (SB == 2) vmax = max(vmax, s);
                    if constexpr (IN == YCC_IN_MATRIX) {
                        const float yy = ycc_clamp((ycc_luma_in<IN>(s, t) + m.a * lb[k / SHR]) + m.b * lr[k / SHR]);
                        v[k] = k < nk ? yy : -128.0f;
                    } else {
                        v[k] = ycc_luma_in<IN>(s, t);
                    }
                }
                arai8(v);
                front_store_row<G>(sT, (ly >> 3) * 32 + c * HR + h, (ly & 7), v);
            }
            // the thread's component (h = 0: Cb[']; 1: Cr[']) of the block's chroma row r
            [[maybe_unused]] const float m0 = h ? m.e : m.c, m1 = h ? m.f : m.d;
            float v[8];
#pragma unroll
            for (int gx = 0; gx < RX; ++gx) {  // 8 plane positions -> 8 / RX samples
                float cv[RY][8];
#pragma unroll
                for (int dy = 0; dy < RY; ++dy) {
                    [[maybe_unused]] float pr[8];
                    positions(std::integral_constant<int, 8>{}, r * RY + dy, P * c + 8 * gx, cv[dy], pr);
                    if constexpr (IN == YCC_IN_MATRIX) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) cv[dy][k] = ycc_clamp(m0 * cv[dy][k] + m1 * pr[k]);
                    }
                }
                // the box: x outer, y inner, the sum, then the division by the count (exact: by 2 or 4)
#pragma unroll
                for (int j = 0; j < 8 / RX; ++j) {
                    float s = cv[0][RX * j];
#pragma unroll
                    for (int xx = 0; xx < RX; ++xx)
#pragma unroll
                        for (int yy = 0; yy < RY; ++yy)
                            if (xx + yy > 0) s = s + cv[yy][RX * j + xx];
                    v[gx * (8 / RX) + j] = s * (1.0f / (float)(RX * RY));
                }
            }
            arai8(v);
            front_store_row<G>(sT, NYB + h * CB + c, r, v);
        }
        __syncthreads();
        front_column_pass<G, NARROW, false>(sT, sQ, sRQ, tid, false, g, frame, mx0, my, coef, coef_lo, coef_hi);
    }
    if constexpr (SB == 2) {
        // a code above 2^B - 1 (color.rs:63-65's panic): one vote per wave, its leader stores
        const bool bad = check_range && vmax > max_code;
        if (__ballot(bad)) raise_status(status, bad ? 1 : 0);
    }
}

// One argument list for the three kinds (the plain kind passes a status it never raises)
template <class Args, int HR, int VR, int SHR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_sub(Args ya, size_t frame_stride, Geom g,
                                                           const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                           int* __restrict__ status) {
    front_ycc_sub_body<HR, VR, SHR, FMT, SB, false>(ya, frame_stride, g, qtab, coef, status, nullptr, nullptr);
}
template <class Args, int HR, int VR, int SHR, int FMT, int SB, int WPE>
__global__ __launch_bounds__(256, WPE) void k_front_ycc_sub_n(Args ya, size_t frame_stride, Geom g,
                                                             const float* __restrict__ qtab, int16_t* __restrict__ coef,
                                                             int* __restrict__ status, int16_t* __restrict__ coef_lo,
                                                             int8_t* __restrict__ coef_hi) {
    front_ycc_sub_body<HR, VR, SHR, FMT, SB, true>(ya, frame_stride, g, qtab, coef, status, coef_lo, coef_hi);
}

// ============================================================== launcher

// Waves per SIMD the kernel is compiled for (register budget 512 / WPE), from the LDS
// of the tile (sT and the staged bytes) and -Rpass-analysis=kernel-resource-usage;
// DESIGN.md section 15 lists what each instantiation takes.  4:4:4 -> 4:2:0 stages
// 42 KB (uint8) or 54 KB (uint16) and 4:2:2 -> 4:2:0 of uint16 46 KB: three workgroups
// per CU of 160 KB at best, 3.  4:2:2 -> 4:2:0 of uint8 (38 KB) and 4:4:4 -> 4:2:2
// (24 to 32 KB) hold four: 4.  The matrix kind keeps ten more constants and both
// components' values: with uint16 4:4:4 planes it spilled under those budgets (a
// 4:2:0 file: some 40 registers, next to the seven prefetched chunks; a 4:2:2 file: the
// narrow twin, 5) and is compiled for one workgroup per CU less, 2 and 3.  None spills.
template <int VR, int SHR, int SB, int IN>
constexpr int front_ycc_sub_wpe() {
    if (IN == YCC_IN_MATRIX && SB == 2 && SHR == 1) return VR == 2 ? 2 : 3;
    return VR == 2 && (SHR == 1 || SB == 2) ? 3 : 4;
}

template <class Args>
static void front_ycc_sub_dispatch(const Args& ya, const YccFrames& yf, int sb, size_t frame_stride, int n_frames,
                                   const Geom& g, const Work& w, hipStream_t st, int per_cu_cap) {
    auto launch = [&](auto fmt, auto sbc, auto vr, auto shr) {
        constexpr int FMT = decltype(fmt)::value, SB = decltype(sbc)::value;
        constexpr int VR = decltype(vr)::value, SHR = decltype(shr)::value, WPE = front_ycc_sub_wpe<VR, SHR, SB, Args::IN>();
        front_launch<k_front_ycc_sub<Args, 2, VR, SHR, FMT, SB, WPE>, k_front_ycc_sub_n<Args, 2, VR, SHR, FMT, SB, WPE>>(
            g, n_frames, per_cu_cap, st, w.coef_lo, w.coef_hi, ya, frame_stride, g, w.qtab, w.coef, w.status);
    };
    using One = std::integral_constant<int, 1>;
    using Two = std::integral_constant<int, 2>;
    auto with_pair = [&](auto fmt, auto sbc) {
        if (g.vr == 1)
            launch(fmt, sbc, One{}, One{});  // 4:4:4 -> 4:2:2
        else if (yf.src_hr == 1)
            launch(fmt, sbc, Two{}, One{});  // 4:4:4 -> 4:2:0
        else
            launch(fmt, sbc, Two{}, Two{});  // 4:2:2 -> 4:2:0
    };
    auto with_sb = [&](auto fmt) {
        if constexpr (Args::IN != YCC_IN_PLAIN) {
            if (sb == 2) return with_pair(fmt, Two{});
        }
        with_pair(fmt, One{});
    };
    if (yf.format == YCC_PLANAR)
        with_sb(std::integral_constant<int, YCC_PLANAR>{});
    else if (yf.format == YCC_NV)
        with_sb(std::integral_constant<int, YCC_NV>{});
    else
        with_sb(std::integral_constant<int, YCC_NV_VU>{});
}

hipError_t launch_front_ycc_sub(const YccFrames& yf, const YccLevels* lv, const YccMatrix* mx,
                                size_t frame_stride_bytes, int n_frames, const Geom& g, const Work& w, hipStream_t st,
                                int per_cu_cap) {
    if (yf.format < YCC_PLANAR || yf.format > YCC_NV_VU || (lv && !ycc_levels_valid(*lv)) || (mx && !lv))
        return hipErrorInvalidValue;
    // a converting pair: the file 4:2:x, the planes' rows at every luma row, and finer than the file
    if (g.hr != 2 || yf.src_vr != 1 || (yf.src_hr != 1 && yf.src_hr != 2) || (yf.src_hr == 2 && g.vr == 1))
        return hipErrorInvalidValue;
    const int sb = lv ? lv->sample_bytes : 1;
    if (mx) {
        YccMxArgs ya = ycc_args<YccMxArgs>(yf, lv, g, yf.src_hr, yf.src_vr);
        ya.m = *mx;
        front_ycc_sub_dispatch(ya, yf, sb, frame_stride_bytes, n_frames, g, w, st, per_cu_cap);
    } else if (lv) {
        front_ycc_sub_dispatch(ycc_args<YccLvArgs>(yf, lv, g, yf.src_hr, yf.src_vr), yf, sb, frame_stride_bytes, n_frames,
                               g, w, st, per_cu_cap);
    } else {
        front_ycc_sub_dispatch(ycc_args<YccArgs>(yf, nullptr, g, yf.src_hr, yf.src_vr), yf, sb, frame_stride_bytes,
                               n_frames, g, w, st, per_cu_cap);
    }
    return hipGetLastError();
}

}  // namespace dmmt
