"""k_stuffwrite with one chunk per wave (csrc/entropy.hip, DMMT_STUFF_WAVE_CHUNK):
wave w of workgroup b owns chunk 4 b + w, runs the chunk's prologue once, stages
passes of 1,024 bytes in its own LDS region and waits for no other wave.  Everything
byte for byte against the CPU reference; the block and chunk counts of a case are
asserted from its geometry before anything is encoded.

* 1, 4, 5 and 9 chunks: a lone wave, a full workgroup, a workgroup of one wave with
  three spare ones, two full workgroups and one more wave; 4:2:0; three frames in a
  call (the grid's second dimension).
* a chunk whose scan bytes lie just below and just above 1,024 and 2,048 (one and
  two passes, the last one a few bytes or all but a few), found by bisection of a
  noise amplitude on the reference's stream; tens of passes per wave (full-range
  noise under all-ones tables); the flat image whose tail chunk lies inside the
  previous chunk's last byte; passes dense with 0xFF.
* restart intervals 1 and 7: RSTm after a partial piece, in every wave of a
  workgroup, its last one included, and in a workgroup with spare waves.
* a restart stripe and a joined stripe of two chunks each (stripe_encode,
  stripe_write: out_len and the shared last byte of a stripe that more follow).
* an output stride one byte below dmmt_max_jpeg_bytes: DMMT_E_CAPACITY, and the
  next call with the exact stride gives the file.  (The library refuses that stride
  before any launch; the kernel's own capacity checks cannot fire through the C ABI
  while dmmt_max_jpeg_bytes bounds every file.)"""
import numpy as np
import pytest

import dmmt_jpeg
import oracle
from test_gpu_scalar_trim import _opts, _scan_bytes
from test_gpu_stripes import _joined_on_one_gpu, _striped_on_one_gpu

pytestmark = pytest.mark.gpu

CHUNK_BLOCKS = 256
MCU = {0: (8, 8, 3), 1: (16, 8, 4), 2: (16, 16, 6)}  # MCU width, height, blocks


def _geometry(w, h, sub):
    mw, mh, bpm = MCU[sub]
    blocks = -(-w // mw) * -(-h // mh) * bpm
    return blocks, -(-blocks // CHUNK_BLOCKS)


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _encode(encoder, rgb, sub, q, ri=0):
    return encoder.encode(dmmt_jpeg.Image.from_array(rgb), _opts(sub, q, ri))


def _ref(rgb, sub, q, ri=0):
    luma, chroma = dmmt_jpeg.quality_tables(q)
    return oracle.encode(rgb, 255, sub, luma, chroma, restart_interval=ri)


@pytest.mark.parametrize("w,h,chunks", [(88, 8, 1), (168, 104, 4), (176, 128, 5), (216, 208, 9)])
def test_chunk_counts(encoder, w, h, chunks):
    blocks, nch = _geometry(w, h, 0)
    assert blocks == (w // 8) * (h // 8) * 3 and nch == chunks
    rgb = _noise(w, h, w + h)
    assert _encode(encoder, rgb, 0, 90) == _ref(rgb, 0, 90)


def test_five_chunk_shape_at_420(encoder):
    assert _geometry(176, 128, 2) == (528, 3)
    rgb = _noise(176, 128, 420)
    assert _encode(encoder, rgb, 2, 90) == _ref(rgb, 2, 90)


def test_three_frames_in_a_call(encoder):
    assert _geometry(176, 128, 0) == (1056, 5)
    frames = [_noise(176, 128, 30 + i) for i in range(3)]
    frames[1][:] = 77  # a flat frame between two of noise: chunks of a few bytes
    got = encoder.encode_batch([dmmt_jpeg.Image.from_array(f) for f in frames], _opts(0, 90))
    assert [len(g) for g in got] == [len(_ref(f, 0, 90)) for f in frames]
    assert got == [_ref(f, 0, 90) for f in frames]


def _single_chunk_of(lo, hi):
    """88 x 56, 4:4:4, q90: one chunk of 231 blocks whose scan is lo..hi bytes long (before
    stuffing) -- seeded noise whose amplitude is bisected, at most 40 reference encodes"""
    w, h = 88, 56
    assert _geometry(w, h, 0) == (231, 1)
    field = np.random.default_rng(1024).uniform(-1.0, 1.0, (h, w, 3))
    a0, a1 = 0.0, 127.0
    for _ in range(40):
        a = (a0 + a1) / 2
        rgb = np.clip(np.rint(128 + a * field), 0, 255).astype(np.uint8)
        n = len(_scan_bytes(_ref(rgb, 0, 90)))
        if lo <= n <= hi:
            return rgb, n
        if n < lo:
            a0 = a
        else:
            a1 = a
    raise AssertionError(f"no amplitude gives a scan of {lo}..{hi} bytes")


@pytest.mark.parametrize("lo,hi", [(1008, 1023), (1025, 1040), (2032, 2047), (2049, 2064)])
def test_scan_bytes_around_a_pass(encoder, lo, hi):
    rgb, n = _single_chunk_of(lo, hi)
    print(n)
    assert lo <= n <= hi
    assert _encode(encoder, rgb, 0, 90) == _ref(rgb, 0, 90)


def test_tens_of_passes_per_wave(encoder):
    """128 x 128 full-range noise under all-ones tables: three chunks, each wave more
    than ten passes of 1,024 bytes"""
    assert _geometry(128, 128, 0) == (768, 3)
    rgb = _noise(128, 128, 5)
    ones = [1] * 64
    ref = oracle.encode(rgb, 255, 0, ones, ones)
    assert len(_scan_bytes(ref)) > 3 * 10 * 1024
    opts = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(0), 8, luma_table=ones, chroma_table=ones)
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), opts) == ref


def test_flat_tail_chunk_inside_the_previous_last_byte(encoder):
    """Flat 4:4:4 images of 86 and 87 MCUs: a chunk of 256 blocks of a few bits each and a
    tail chunk of 2 and 5 blocks in the next wave.  The first MCU's level moves the
    first chunk's end through a byte: a tail of two blocks that starts 1 to 4 bits
    into a byte lies inside the first chunk's last byte."""
    bad = []
    for mcus in (86, 87):
        assert _geometry(8 * mcus, 8, 0) == (3 * mcus, 2)
        for v in (0, 100, 160, 180, 190, 196, 199, 255):
            rgb = np.full((8, 8 * mcus, 3), 200, np.uint8)
            rgb[:, :8, 0] = v
            rgb[:, :8, 1:] = 255 - v
            if _encode(encoder, rgb, 0, 90) != _ref(rgb, 0, 90):
                bad.append((mcus, v))
    assert not bad, f"files differ from the oracle for (MCUs, level) {bad}"


def test_passes_dense_with_ff(encoder):
    """264 x 64, 4:4:4: the first 396 of 792 blocks hold 63 coefficients of 32767 (16 one
    bits of extra bits each), so the first chunk is several passes in which more than
    half of a wave's 16-byte pieces hold a 0xFF"""
    w, h = 264, 64
    nb, nch = _geometry(w, h, 0)
    assert (nb, nch) == (792, 4)
    rng = np.random.default_rng(255)
    coef = np.where(rng.random((nb, 64)) < 0.05, rng.integers(-20, 21, (nb, 64)), 0).astype(np.int16)
    coef[:nb // 2, 1:] = 32767
    coef[:nb // 2, 0] = 0
    luma, chroma = dmmt_jpeg.quality_tables(75)
    ref = oracle.encode_coefficients(coef, w, h, 0, luma, chroma)
    scan = _scan_bytes(ref)
    assert len(scan) > 4 * 1024
    with_ff = sum(1 for i in range(0, 1024, 16) if b"\xff" in scan[i:i + 16])
    print(with_ff)
    assert with_ff > 32
    assert encoder.encode_coefficients(coef, w, h, _opts(0, 75)) == ref


@pytest.mark.parametrize("ri,chunks", [(1, 72), (7, 11)])
def test_restart_marker_in_every_wave(encoder, ri, chunks):
    """64 x 72: 72 MCUs; the chunk grid restarts with every segment, so each segment of
    ri MCUs is a chunk that ends in a partial piece with RSTm after it -- ri 1: 18 full
    workgroups; ri 7: two full workgroups and one of three waves"""
    rgb = _noise(72, 64, 9)
    assert _geometry(72, 64, 0)[0] == 216 and -(-72 // ri) == chunks and 3 * ri <= CHUNK_BLOCKS
    ref = _ref(rgb, 0, 95, ri)
    assert sum(ref.count(bytes([0xFF, 0xD0 + m])) for m in range(8)) >= chunks - 1
    assert _encode(encoder, rgb, 0, 95, ri) == ref


def test_restart_stripes_of_two_chunks(encoder):
    """168 x 128 in two stripes of 8 MCU rows, one restart segment each: 504 blocks, two
    chunks, RSTm after the first stripe and out_len without EOI"""
    w, h = 168, 128
    assert _geometry(w, h // 2, 0) == (504, 2)
    rgb = _noise(w, h, 61)
    data, opts = _striped_on_one_gpu(rgb, 0, 90, 8, 2)
    assert opts.restart_interval == 21 * 8
    assert data == oracle.encode(rgb, 255, 0, opts.luma_table, opts.chroma_table, restart_interval=21 * 8)


def test_joined_stripes_of_two_chunks(encoder):
    """the same frame as two joined stripes: the first stripe's last byte runs on into
    the second one's first bits"""
    w, h = 168, 128
    assert _geometry(w, h // 2, 0) == (504, 2)
    rgb = _noise(w, h, 62)
    data, opts = _joined_on_one_gpu(rgb, 0, 90, 2)
    assert data == oracle.encode(rgb, 255, 0, opts.luma_table, opts.chroma_table)


def test_stride_one_byte_too_small_then_exact(encoder):
    w, h = 176, 128
    rgb = _noise(w, h, 63)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, 0)
    d_in, d_out, d_len = encoder.malloc(rgb.nbytes), encoder.malloc(cap), encoder.malloc(4)
    try:
        encoder.h2d(d_in, rgb)
        with pytest.raises(dmmt_jpeg.Error) as e:
            encoder.encode_device(d_in, 1, w, h, _opts(0, 90), d_out, cap - 1, d_len)
        assert e.value.code == -203  # DMMT_E_CAPACITY
        encoder.encode_device(d_in, 1, w, h, _opts(0, 90), d_out, cap, d_len)
        encoder.synchronize()
        n = int(np.frombuffer(encoder.d2h(d_len, 4), np.uint32)[0])
        assert encoder.d2h(d_out, n) == _ref(rgb, 0, 90)
    finally:
        for p in (d_in, d_out, d_len):
            encoder.free(p)
