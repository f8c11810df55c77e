// kernels.hpp -- host-side launchers of the gfx950 kernels (kernels.hip, entropy.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coef_format.hpp"
#include "jpeg_common.hpp"

namespace dmmt {

// Device workspace of one launch batch (see the kernels for each buffer's role).
struct Work {
    int16_t* coef;                  // [frames][bpf][64] column-major blocks (coef_pos), emission order; narrow form: the escape store
    int16_t* coef_lo;               // narrow form (coef_format.hpp): [frames][bpf][8], zigzag 0..7; nullptr: the call is wide
    int8_t* coef_hi;                // narrow form: [frames][bpf][64] bytes at coef_pos
    int16_t* dcdiff;                // [frames][bpf]
    uint8_t* lastnz;                // [frames][bpf] zigzag position of the last non-zero AC (0: none)
    uint32_t* ac_hist;              // [frames][reps][2][256], zero between launches
    uint32_t* dc_hist;              // [frames][reps][2][16], zero between launches
    uint32_t* code_tab;             // [frames][4][256]  (len << 16) | code
    uint32_t* hdr_len;              // [frames]
    uint32_t* stage;                // [frames][nch][kChunkWordsCap] each chunk's own bit stream, MSB first
    uint32_t* chunk_bits;           // [frames][nch] bits of the chunk
    uint32_t* chunk_ff;             // [frames][nch][8] 0xFF bytes inside the chunk per alignment residue
    unsigned long long* chunk_ff8;  // [frames * nch + 2] the same eight counts one byte each (255: take chunk_ff's)
    uint32_t* chunk_edge;           // [frames][nch] first 16 bits << 16 | last 16 bits
    unsigned long long* chunk_bit0; // [frames][nch] bit offset of the chunk in its restart segment
    unsigned long long* chunk_out;  // [frames][nch] offset of the chunk's output bytes after the header
    unsigned long long* total_out;  // [frames] stuffed scan bytes incl. RST markers
    uint32_t* arrive;               // [frames][kArriveFrameWords] k_emit's finished workgroups (fused offsets), zero between launches
    int* status;                    // error words (raise_status): bit k of the error kinds -> word k; 1 value>max, 2 table, 4 category range, 16 output capacity
    const float* norm_lut;          // maxval-normalisation table
    const float* qtab;              // [2][64] f32
    const uint8_t* qtab_u8;         // [2][64] natural order, then [2][64] zigzag (the DQT bytes)
};

enum Stage { ST_FRONT = 0, ST_HIST, ST_TABLES, ST_EMIT, ST_OFFSETS, ST_STUFFWRITE, ST_COUNT };

// A device surface (dmmt_device_surfaces): format as dmmt_pixel_format
enum { SURF_RGB = 0, SURF_BGR = 1, SURF_RGBX = 2, SURF_BGRX = 3, SURF_PLANAR = 4 };
struct Surface {
    const void* plane[3];  // interleaved: plane[0] only
    size_t row_pitch;      // bytes between rows of a plane
    int format;
};
// k_front_surf's view of it
struct SurfArgs {
    const uint8_t* plane[3];
    long long pitch;  // bytes between rows
    long long span;   // readable bytes of a plane, per frame (dmmt_surface_span)
    int bgr;          // interleaved: samples 0 and 2 are B and R
};
// samples per pixel of a plane; 0: the (format, sample_bytes) pair is not supported
int surface_samples_per_pixel(int format, int sample_bytes);
// k_front over a surface (frames frame_stride_bytes apart in every plane)
hipError_t launch_front_surface(const Surface& sf, size_t frame_stride_bytes, int sample_bytes, int n_frames,
                                const Geom& g, const Work& w, hipStream_t st, int per_cu_cap = 0);

// YCbCr frames (dmmt_device_ycc): format as dmmt_ycc_format
enum { YCC_PLANAR = 0, YCC_NV = 1, YCC_NV_VU = 2 };
struct YccFrames {
    const void* plane[3];  // Y; Cb or the plane of pairs; Cr (planar only)
    size_t luma_pitch, chroma_pitch;
    int format;
    // the rates the chroma planes lie at when finer than the file's (g.hr, g.vr), the
    // converting pairs of dmmt_encode_device_ycc_subsample; 0, 0: the file's
    int src_hr, src_vr;
};
// bytes from the first byte of `plane` to one past its last, per frame; 0: a bad
// format or a plane the format does not use
size_t ycc_plane_span(int format, int plane, int width, int height, int hr, int vr, size_t luma_pitch,
                      size_t chroma_pitch);

// The sample levels of YCbCr frames (dmmt_ycc_levels): range as dmmt_ycc_range
enum { YCC_RANGE_FULL = 0, YCC_RANGE_LIMITED = 1 };
struct YccLevels {
    int range, bit_depth, sample_bytes, shift;
};
// code v -> the DCT's input: luma min(max((v - off_y) * k_y, 0), 255) - 128, chroma
// min(max((v - off_c) * k_c, -128), 127), in f32, each operation rounded once
struct YccTransfer {
    float off_y, k_y, off_c, k_c;
};
// a description k_front_ycc takes: uint8 with 8 bits, uint16 with 8..16 bits
// and shift <= 16 - bits
bool ycc_levels_valid(const YccLevels& lv);
YccTransfer ycc_levels_transfer(const YccLevels& lv);  // (host; lv valid)
// ycc_plane_span with sample_bytes bytes per sample (0: not 1 or 2)
size_t ycc_plane_span_levels(int format, int plane, int width, int height, int hr, int vr, size_t luma_pitch,
                             size_t chroma_pitch, int sample_bytes);

// The matrix YCbCr planes carry (dmmt_ycc_matrix); JFIF is BT.601, no conversion
enum { YCC_MATRIX_JFIF = 0, YCC_MATRIX_BT709 = 1, YCC_MATRIX_BT2020 = 2 };
// the step to BT.601 after the transfer, in f32, each operation rounded once, clamped to
// [-128, 127]: Y' = (y + a cb) + b cr, Cb' = c cb + d cr, Cr' = e cb + f cr
struct YccMatrix {
    float a, b, c, d, e, f;
};
// the six constants of BT709 or BT2020 (host, double precision rounded once); false:
// another matrix, JFIF included
bool ycc_matrix_coefficients(int matrix, YccMatrix* out);
// k_front_ycc (front_ycc.hip): the planes -> w.coef, as launch_front; their chroma
// sampling is g's.  lv null: uint8 full range (the plain instantiations); else any
// valid levels, and a code above 2^bits - 1 raises status bit 1.  mx (needs lv):
// that step after the transfer; null: none.  yf.src_hr set: the planes lie at (src_hr,
// src_vr), one of 4:4:4 -> 4:2:2, 4:4:4 -> 4:2:0, 4:2:2 -> 4:2:0, and k_front_ycc_sub
// (front_ycc_sub.hip, launch_front_ycc_sub) box-averages their chroma to g's sampling
hipError_t launch_front_ycc(const YccFrames& yf, const YccLevels* lv, const YccMatrix* mx, size_t frame_stride_bytes,
                            int n_frames, const Geom& g, const Work& w, hipStream_t st, int per_cu_cap = 0);
// what launch_front_ycc forwards to when yf.src_hr is set (hipErrorInvalidValue: no converting pair)
hipError_t launch_front_ycc_sub(const YccFrames& yf, const YccLevels* lv, const YccMatrix* mx,
                                size_t frame_stride_bytes, int n_frames, const Geom& g, const Work& w, hipStream_t st,
                                int per_cu_cap = 0);

// A one-channel plane (dmmt_device_gray): transfer as dmmt_gray_transfer
enum { GRAY_AS_RGB = 0, GRAY_Y_FULL_RANGE = 1 };
struct GrayPlane {
    const void* plane;
    size_t row_pitch;  // bytes between rows
    int transfer;      // GRAY_AS_RGB or GRAY_Y_FULL_RANGE: what the table holds
    const float* lut;  // device: the luma per sample value (gray_fill_lut); unused for float samples
};
// bytes from the plane's first byte to one past its last, per frame; 0: a bad description
size_t gray_plane_span(int width, int height, int sample_bytes, size_t row_pitch);
// the luma of sample values 0 .. n-1 as k_front_gray's table holds them (host)
void gray_fill_lut(float* lut, size_t n, int maxval, int transfer);
// k_front_gray (front_gray.hip): the plane -> w.coef, as launch_front; g from
// make_geom(..., ncomp = 1)
hipError_t launch_front_gray(const GrayPlane& gp, size_t frame_stride_bytes, int sample_bytes, int n_frames,
                             const Geom& g, const Work& w, hipStream_t st, int per_cu_cap = 0);

// per_cu_cap: at most this many resident k_front workgroups per CU (0: as many as
// fit, 4); a context of several lanes passes DMMT_FRONT_PER_CU_LANES
hipError_t launch_front(const void* rgb, size_t frame_stride_bytes, int sample_bytes, int n_frames, const Geom& g,
                        const Work& w, hipStream_t st, int per_cu_cap = 0);
#ifndef DMMT_FRONT_PER_CU_LANES
#define DMMT_FRONT_PER_CU_LANES 2  // k_front workgroups per CU with several lanes (profiles/r06_front_per_cu_lanes_ab.txt)
#endif
// DC differences, AC and DC histograms, last non-zero positions of the blocks in
// w.coef (check_cat: an AC -32768, which has no category, can occur)
// fuse_tables: when tables_fusable(g), the frame's last k_hist workgroup also does
// launch_tables' work (code tables, header into out), and no launch_tables follows
bool tables_fusable(const Geom& g);
// wg_cap: at most this many workgroups per launch (0: the default, DMMT_HIST_WG_CAP)
hipError_t launch_hist(int n_frames, const Geom& g, const Work& w, int check_cat, hipStream_t st,
                       bool fuse_tables = false, int bits_per_channel = 8, uint8_t* out = nullptr,
                       size_t out_stride = 0, int wg_cap = 0);
#ifndef DMMT_HIST_WG_CAP_LANES
#define DMMT_HIST_WG_CAP_LANES 512  // k_hist's cap when the context runs several lanes (profiles/r06_hist_cap_lanes_ab.txt)
#endif
hipError_t launch_tables(int n_frames, const Geom& g, const Work& w, int bits_per_channel, uint8_t* out,
                         size_t out_stride, hipStream_t st);
// fuse_offsets: when offsets_fusable(g), k_emit's last workgroup per frame also
// computes the chunk offsets (chunk_bit0, chunk_out, total_out), and no
// launch_offsets is needed; otherwise launch_offsets follows as before
constexpr int kFusedRoundChunks = 1536;       // per round of the fused scan (4K 4:4:4: 1519 chunks, one round)
constexpr int kFusedOffsetsMaxChunks = 4 * kFusedRoundChunks;  // (8K 4:2:0: 3038 chunks, two rounds)
constexpr int kArriveFrameWords = 65 * 32;  // k_emit's arrival counters per frame (Work::arrive)
bool offsets_fusable(const Geom& g);
// prio: k_emit's heavier waves raise their issue priority (a context of one lane:
// shorter frames; with several lanes it costs the others' kernels issue slots)
hipError_t launch_emit(int n_frames, const Geom& g, const Work& w, bool fuse_offsets, hipStream_t st, bool prio);
hipError_t launch_offsets(int n_frames, const Geom& g, const Work& w, hipStream_t st);
hipError_t launch_stuffwrite(int n_frames, const Geom& g, const Work& w, uint8_t* out, size_t out_stride,
                             uint32_t* out_len, hipStream_t st);
// P3 body decoding (ppm_device.hip): text [body_offset, len) -> nsamples samples of
// sample_bytes each.  The comment-free path (when ppm_fast_path) runs first and
// writes its report into host-mapped memory (24 bytes, zeroed by the caller before
// the launch: u32 '#' seen, u32 parse error, u32 sample above maxval, u32, u64 tokens
// found); counts: 4 ppm_counts_capacity(n) bytes, row_base 8 * 1024 bytes.  If it
// saw a '#', the general path redoes the body: misc (device, 24 bytes: u32 status
// (1 parse error, 2 sample above maxval), u32, u64 tokens found), maps and chunk_in
// 8 max(n, 1024) bytes each (n = ppm_chunk_count(...)).
size_t ppm_chunk_count(const uint8_t* text, size_t body_offset, size_t len);
size_t ppm_counts_capacity(long long nch);
constexpr size_t kPpmReportBytes = 32;  // one comment-free report (24 bytes used)
bool ppm_fast_path(const uint8_t* text, size_t body_offset, size_t len);
hipError_t launch_ppm_p3_fast(const uint8_t* text, size_t body_offset, size_t len, uint32_t* counts,
                              unsigned long long* row_base, void* report, void* out, int sample_bytes,
                              unsigned long long nsamples, uint32_t maxval, hipStream_t st);
hipError_t launch_ppm_p3_general(const uint8_t* text, size_t body_offset, size_t len, unsigned long long* maps,
                                 unsigned long long* chunk_in, void* misc, void* out, int sample_bytes,
                                 unsigned long long nsamples, uint32_t maxval, hipStream_t st);
// P6 samples (big-endian u16 or u8) already in device memory -> host-endian samples
// (maxval and status unused: the encoder checks the range, as for dmmt_parse_ppm)
hipError_t launch_ppm_p6(const uint8_t* samples, void* out, int sample_bytes, unsigned long long nsamples,
                         uint32_t maxval, uint32_t* status, hipStream_t st);
hipError_t launch_dct_blocks(float* data, long long nblocks, hipStream_t st);
hipError_t launch_synthetic(uint8_t* rgb, int w, int h, int n_frames, int first_frame, uint32_t seed, int row0,
                            int rows, hipStream_t st);

}  // namespace dmmt
