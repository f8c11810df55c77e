"""The entropy walk's exits, the byte stuffing's staging and the colour
conversion's exact-half terms, byte for byte against the oracle.

* walk_block (k_emit) tests the wave's last position once per group of four
  zigzag positions and votes on a run of 16 or more before it enters the ZRL
  loop: every stopping position 1..63, ZRL counts 0 to 3 at their boundaries, and
  waves in which only some lanes have a long run.  [encoder.rs:356-404,
  categorize.rs:132-169]
* k_stuffwrite stages every 16-byte piece without a branch per byte (each byte
  at its place plus the count of 0xFF bytes before it in the piece), the 0x00
  bytes of the pieces that hold a 0xFF in a loop of their own, and stores a
  pass's ragged first and last 16 bytes one byte per lane: passes full of 0xFF,
  several passes per chunk, partial last pieces, chunks of a few bits, RSTm
  after a partial piece.  [binary_stream.rs:38-96,
  segment_marker_injector.rs:13-30]
* rgb_to_ycbcr takes its two products by 0.5 into an fma for integer samples.
  [color.rs:45-100]"""
import numpy as np
import pytest

import dmmt_jpeg
import oracle

pytestmark = pytest.mark.gpu

PF = dmmt_jpeg.PixelFormat


def _opts(sub, q, ri=0):
    luma, chroma = dmmt_jpeg.quality_tables(q)
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                              chroma_table=chroma, restart_interval=ri)


def _scan_bytes(jpeg):
    """the entropy-coded bytes of a single-scan file without restart markers, unstuffed"""
    sos = jpeg.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(jpeg[sos + 2:sos + 4], "big")
    assert jpeg[-2:] == b"\xff\xd9"
    return jpeg[start:-2].replace(b"\xff\x00", b"\xff")


# ------------------------------------------------------------------ walk exits

def _walk_blocks(K):
    """66 blocks (22 MCUs of 4:4:4: one chunk, a full wave and a wave of two) whose
    last non-zero positions are at most K.  Three end exactly at K: a dense one, one
    whose only AC coefficient is at K (a run of K - 1 zeros: (K - 1) // 16 ZRLs)
    and one with coefficients at 1 and K only.  k_emit sorts the blocks by that
    position, so K is where the second wave stops and, with three blocks there,
    where the first one stops too; both waves hold ordinary blocks next to one
    with a long run."""
    rng = np.random.default_rng(1000 + K)
    coef = np.zeros((66, 64), np.int16)
    coef[:, 0] = rng.integers(-300, 301, 66)
    last = rng.integers(0, K + 1, 66)
    last[:3] = K
    for i in range(66):
        n = int(last[i])
        if n == 0:
            continue
        body = np.where(rng.random(n) < 0.4, rng.integers(-255, 256, n), 0)
        if i % 7 == 3:
            body[rng.integers(0, n)] = int(rng.choice([-1023, 1023]))
        coef[i, 1:n + 1] = body
        coef[i, n] = int(rng.choice([-3, -1, 1, 2, 700]))
    coef[1, 1:] = 0
    coef[1, K] = -5
    coef[2, 1:] = 0
    coef[2, 1] = 9
    coef[2, K] = 1
    order = rng.permutation(66)  # the three anywhere in the chunk
    coef = coef[order]
    lastnz = [int(np.flatnonzero(np.r_[1, b[1:]])[-1]) for b in coef]
    assert max(lastnz) == K and lastnz.count(K) >= 3
    return coef


def test_walk_every_exit(encoder):
    """K = 1..63: the wave's stopping position at every group boundary and every
    place inside a group; a lone coefficient at 16, 17, 32, 33, 48, 49 and 63 gives
    0, 1, 1, 2, 2, 3 and 3 ZRLs."""
    opts = _opts(0, 90)
    luma, chroma = dmmt_jpeg.quality_tables(90)
    bad = []
    for K in range(1, 64):
        coef = _walk_blocks(K)
        ref = oracle.encode_coefficients(coef, 176, 8, 0, luma, chroma)
        if encoder.encode_coefficients(coef, 176, 8, opts) != ref:
            bad.append(K)
    assert not bad, f"files differ from the oracle for last positions {bad}"


@pytest.mark.parametrize("sub", [1, 2])
def test_walk_long_runs_among_ordinary_blocks(encoder, sub):
    """Several chunks of sparse blocks (runs of 16 and more in some lanes of every
    wave, none in most) and dense ones, luma and chroma tables mixed in a wave."""
    w, h = 256, 64
    mcus = (w // 16) * (h // (8 if sub == 1 else 16))
    nb = mcus * (4 if sub == 1 else 6)
    rng = np.random.default_rng(77 + sub)
    dense = np.where(rng.random((nb, 64)) < 0.5, rng.integers(-40, 41, (nb, 64)), 0)
    sparse = np.where(rng.random((nb, 64)) < 0.03, rng.integers(-40, 41, (nb, 64)), 0)
    coef = np.where((rng.random(nb) < 0.25)[:, None], sparse, dense).astype(np.int16)
    luma, chroma = dmmt_jpeg.quality_tables(90)
    ref = oracle.encode_coefficients(coef, w, h, sub, luma, chroma)
    assert encoder.encode_coefficients(coef, w, h, _opts(sub, 90)) == ref


# -------------------------------------------------------------------- stuffing

def test_stuff_chunks_longer_than_a_pass(encoder):
    """128x128 noise at q100, 4:4:4: three chunks of far more than one 4096-byte
    pass each (and blocks too long for k_emit's slots: the window walk)."""
    rgb = np.random.default_rng(5).integers(0, 256, (128, 128, 3), dtype=np.uint8)
    luma, chroma = dmmt_jpeg.quality_tables(100)
    ref = oracle.encode(rgb, 255, 0, luma, chroma)
    assert len(_scan_bytes(ref)) > 3 * 2 * 4096
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), _opts(0, 100)) == ref


@pytest.mark.parametrize("sub,w,h", [(0, 264, 256), (2, 528, 512)])
def test_stuff_pieces_full_of_ff(encoder, sub, w, h):
    """The 0xFF-heavy blocks of test_fused_offsets_ff_counts_past_a_byte.  The
    first 256 blocks are heavy: 63 coefficients of at least 16 bits each, so chunk 0
    holds more than 4096 bytes and, starting at bit 0 of the scan, its first pass
    is the scan's first 4096 bytes in 16-byte pieces.  More than 64 of them hold a
    0xFF (more than a wave's worth of pieces shift their bytes and add 0x00s)."""
    nl = 1 if sub == 0 else 4
    mcus = (w // (8 * (1 if sub == 0 else 2))) * (h // (8 * (1 if sub == 0 else 2)))
    nb = mcus * (nl + 2)
    rng = np.random.default_rng(255)
    coef = np.where(rng.random((nb, 64)) < 0.05, rng.integers(-20, 21, (nb, 64)), 0).astype(np.int16)
    heavy = nb // 2
    assert heavy >= 256 and 256 * 63 * 16 // 8 > 4096
    coef[:heavy, 1:] = 32767
    coef[:heavy, 0] = 0
    luma, chroma = dmmt_jpeg.quality_tables(75)
    ref = oracle.encode_coefficients(coef, w, h, sub, luma, chroma)
    scan = _scan_bytes(ref)
    with_ff = sum(1 for i in range(0, 4096, 16) if b"\xff" in scan[i:i + 16])
    assert with_ff > 64
    assert encoder.encode_coefficients(coef, w, h, _opts(sub, 75)) == ref


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_stuff_flat_image_of_eight_mcus(encoder, sub):
    """A flat 8-MCU image: one chunk of a few bits a block, a single partial piece."""
    hr, vr = (1, 1) if sub == 0 else ((2, 1) if sub == 1 else (2, 2))
    rgb = np.full((8 * vr, 64 * hr, 3), 93, np.uint8)
    luma, chroma = dmmt_jpeg.quality_tables(90)
    ref = oracle.encode(rgb, 255, sub, luma, chroma)
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), _opts(sub, 90)) == ref


def test_stuff_flat_tail_chunks(encoder):
    """Flat 4:4:4 images of 86, 87 and 93 MCUs: a first chunk of 256 blocks of a few
    bits each and a tail chunk of 2, 5 and 23 such blocks.  The first MCU's level
    changes the extra bits of the first DC differences, so the first chunk ends at
    different places of a byte: a tail of two blocks that starts 1 to 4 bits into
    a byte lies inside the first chunk's last byte."""
    luma, chroma = dmmt_jpeg.quality_tables(90)
    opts = _opts(0, 90)
    bad = []
    for mcus in (86, 87, 93):
        for v in (0, 100, 160, 180, 190, 196, 199, 255):
            rgb = np.full((8, 8 * mcus, 3), 200, np.uint8)
            rgb[:, :8, 0] = v
            rgb[:, :8, 1:] = 255 - v
            ref = oracle.encode(rgb, 255, 0, luma, chroma)
            if encoder.encode(dmmt_jpeg.Image.from_array(rgb), opts) != ref:
                bad.append((mcus, v))
    assert not bad, f"files differ from the oracle for (MCUs, level) {bad}"


@pytest.mark.parametrize("ri", [1, 7])
def test_stuff_restart_marker_after_partial_piece(encoder, ri):
    """Restart intervals: every segment ends in a partial piece that RSTm follows."""
    rgb = np.random.default_rng(9).integers(0, 256, (64, 72, 3), dtype=np.uint8)
    luma, chroma = dmmt_jpeg.quality_tables(95)
    ref = oracle.encode(rgb, 255, 0, luma, chroma, restart_interval=ri)
    assert ref.count(b"\xff\xd0") >= 1
    assert encoder.encode(dmmt_jpeg.Image.from_array(rgb), _opts(0, 95, ri)) == ref


# ---------------------------------------------------------------------- colour

def _sweep_frame(maxval):
    """256x16: R and B take each of 256 levels spread over 0..maxval (R along the
    row, B shifted by the row), G seeded noise."""
    step = maxval // 255
    x = np.arange(256)
    rgb = np.empty((16, 256, 3), np.uint16)
    rgb[:, :, 0] = (x * step)[None, :]
    rgb[:, :, 2] = ((x[None, :] * 37 + np.arange(16)[:, None] * 16) % 256) * step
    rgb[:, :, 1] = np.random.default_rng(maxval).integers(0, maxval + 1, (16, 256))
    rgb[0, 255, 0] = rgb[15, 0, 2] = maxval
    return rgb


@pytest.fixture(scope="module")
def sweep_refs():
    refs = {}
    luma, chroma = dmmt_jpeg.quality_tables(100)
    for maxval in (255, 65535, 40001):
        rgb = _sweep_frame(maxval)
        for sub in (0, 1, 2):
            refs[maxval, sub] = (rgb, oracle.forward(rgb, maxval, sub, luma, chroma),
                                 oracle.encode(rgb, maxval, sub, luma, chroma))
    return refs


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("maxval", [255, 65535, 40001])
def test_colour_half_terms(encoder, sweep_refs, maxval, sub):
    """Every coefficient of the sweep equals the oracle's through
    dmmt_forward_blocks (q100: a quantiser of 1 to 3 hides nothing), and the file
    from an interleaved B,G,R surface of the same frame equals the oracle's file
    (same tables, so the same coefficients)."""
    rgb, want_blocks, want_file = sweep_refs[maxval, sub]
    opts = _opts(sub, 100)
    got = encoder.forward_blocks(dmmt_jpeg.Image.from_array(rgb, maxval), opts)
    assert got.shape == want_blocks.shape
    assert np.array_equal(got, want_blocks), f"{np.count_nonzero(got != want_blocks)} coefficients differ"

    sb = 1 if maxval == 255 else 2
    bgr = np.ascontiguousarray(rgb[:, :, ::-1].astype(np.uint8 if sb == 1 else np.uint16))
    h, w, _ = rgb.shape
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
    d_in, d_out, d_len = encoder.malloc(bgr.nbytes), encoder.malloc(cap), encoder.malloc(4)
    try:
        encoder.h2d(d_in, bgr.view(np.uint8).reshape(-1))
        encoder.encode_device_surfaces(d_in, PF.BGR, w * 3 * sb, 1, w, h, opts, d_out, cap, d_len, maxval=maxval,
                                       sample_bytes=sb)
        encoder.synchronize()
        n = int(np.frombuffer(encoder.d2h(d_len, 4), np.uint32)[0])
        assert encoder.d2h(d_out, n) == want_file
    finally:
        for p in (d_in, d_out, d_len):
            encoder.free(p)
