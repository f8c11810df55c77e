"""k_emit at eight workgroups per CU (64 VGPRs, the chunk window overlaid on the
slot area of LDS), byte for byte against the oracle at the smallest shapes that
reach every path the smaller kernel changed (profiles/STUDIES.md I):

* a last partial chunk (nb < 256);
* a chunk whose stream needs a second window on the overlaid storage, with blocks
  longer than a slot (the re-walk path into the overlaid window);
* chunks of a few bits (a window's clear of the word past the stream's end);
* restart intervals (the segmented scans of the fused offsets tail);
* 1,547 chunks: one more than a tail round of kFusedRoundChunks = 1536;
* 172,800 blocks, more than 512 * 256: every k_hist workgroup takes several
  passes, bpf not a multiple of the stride, with and without restart intervals,
  in contexts of one and of four lanes;
* four different frames in flight over four lanes.
[encoder.rs:264-404, binary_stream.rs:38-96, segment_marker_injector.rs:13-30]"""
import functools

import numpy as np
import pytest

import dmmt_jpeg
import oracle
from conftest import synthetic

pytestmark = pytest.mark.gpu


def _opts(sub, q, ri=0):
    luma, chroma = dmmt_jpeg.quality_tables(q)
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                              chroma_table=chroma, restart_interval=ri)


def _ref(rgb, sub, opts, threads=1):
    return oracle.encode(rgb, 255, sub, list(opts.luma_table), list(opts.chroma_table),
                         restart_interval=opts.restart_interval, threads=threads, parallel=threads > 1)


@functools.lru_cache(maxsize=None)
def _noise(w, h, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _encode_lanes(enc, frames, opts, lanes):
    """every frame through encode_device, one call each, over `lanes` lanes"""
    h, w = frames[0].shape[:2]
    n = len(frames)
    sub = int(opts.chroma_subsampling_preset)
    stride = (dmmt_jpeg.max_jpeg_bytes(w, h, sub) + 255) // 256 * 256
    d_in, d_out, d_len = enc.malloc(w * h * 3 * n), enc.malloc(stride * n), enc.malloc(4 * n)
    try:
        enc.h2d(d_in, np.ascontiguousarray(np.stack(frames)))
        enc.set_lanes(lanes)
        for i in range(n):
            enc.encode_device(d_in + i * w * h * 3, 1, w, h, opts, d_out + i * stride, stride, d_len + 4 * i)
        enc.synchronize()
        lens = np.frombuffer(enc.d2h(d_len, 4 * n), np.uint32)
        return [enc.d2h(d_out + i * stride, int(lens[i])) for i in range(n)]
    finally:
        enc.set_lanes(1)
        for p in (d_in, d_out, d_len):
            enc.free(p)


@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("w,h", [(16, 16), (24, 40)])
def test_partial_last_chunk(encoder, w, h, sub):
    rgb = _noise(w, h)
    for q in (50, 90):
        opts = _opts(sub, q)
        assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), opts) == _ref(rgb, sub, opts)


def test_second_window_and_rewalk_on_overlaid_storage(encoder):
    """128x128 full-range noise at q100, 4:4:4: 768 blocks in 3 chunks.  The sizes
    are confirmed from the oracle's file: more than 384 bits per block on average
    (after a generous 1 KiB for the header), so some block is longer than a slot
    of kSlotWords = 12 words and its chunk re-walks, and the fullest chunk holds more
    than 256 * 384 bits = 3 windows of kEmitWords = 1024 words"""
    rgb = _noise(128, 128)
    opts = _opts(0, 100)
    ref = _ref(rgb, 0, opts)
    assert (len(ref) - 1024) * 8 > 768 * 384
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), opts) == ref


def test_chunks_of_a_few_bits(encoder):
    """the same noise at q1 and a flat image: a window ends a few words in"""
    rgb = _noise(128, 128)
    opts = _opts(0, 1)
    ref = _ref(rgb, 0, opts)
    assert (len(ref) - 1024) * 8 < 768 * 32  # under a word per block
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), opts) == ref
    flat = np.full((128, 128, 3), 77, np.uint8)
    for q in (1, 90):
        opts = _opts(0, q)
        assert encoder.encode(dmmt_jpeg.Image.from_array(flat), opts) == _ref(flat, 0, opts)


@pytest.mark.parametrize("ri", [1, 7])
def test_restart_segments_small(encoder, ri):
    rgb = _noise(64, 64)
    opts = _opts(2, 90, ri)
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), opts) == _ref(rgb, 2, opts)


def test_tail_second_round_1547_chunks(encoder):
    w, h = 3840, 2200
    assert -(-(w // 8) * (h // 8) * 3 // 256) == 1547
    rgb = synthetic(w, h, frame=3)
    opts = _opts(0, 90)
    assert _encode_lanes(encoder, [rgb], opts, 1)[0] == _ref(rgb, 0, opts, threads=8)


@functools.lru_cache(maxsize=None)
def _qhd(ri):
    w, h = 2560, 1440
    assert (w // 8) * (h // 8) * 3 == 172800 > 512 * 256 and 172800 % (512 * 256) != 0
    rgb = synthetic(w, h, frame=17)
    opts = _opts(0, 75, ri)
    return rgb, opts, _ref(rgb, 0, opts, threads=8)


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("ri", [0, 3])
def test_hist_several_passes(encoder, ri, lanes):
    rgb, opts, ref = _qhd(ri)
    got = _encode_lanes(encoder, [rgb] * lanes, opts, lanes)
    for i, g in enumerate(got):
        assert g == ref, f"lane {i}"


def test_four_frames_over_four_lanes(encoder):
    frames = [_noise(64, 64, seed=s) // (1 + 3 * s) for s in range(4)]  # different content, different lengths
    opts = _opts(0, 90)
    got = _encode_lanes(encoder, frames, opts, 4)
    for i, (g, f) in enumerate(zip(got, frames)):
        assert g == _ref(f, 0, opts), f"lane {i}"
