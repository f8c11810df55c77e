"""Pins the CPU yardstick of the grayscale input path (tests/gray_ref.py) without the
library, for 1x1, 7x17, 33x9 and 257x33 with restart intervals 0 and 3:
  * the oracle's own JPEG decoder gives back the helper's blocks, the padding bits
    are ones, and the file has one component, one DQT and the DHT ids (0,0), (1,1);
  * the decoded blocks are the luma blocks [0::3] decoded from oracle.encode of the
    replicated image at 4:4:4 (AS_RGB), so the coefficients are the reference's;
  * Pillow reads mode L at the right size; with all-ones tables its pixels are
    within 1 level of a uint8 input, and within MAXVAL_1023_BOUND of v/1023*255;
  * three committed goldens match byte for byte."""
import importlib.util
import io
import os

import numpy as np
import pytest

import gray_ref
import oracle
from conftest import GOLDEN
from oracle import jpeg_scan

SIZES = [(1, 1), (7, 17), (33, 9), (257, 33)]
RIS = [0, 3]
ONES = [1] * 64
# Pillow against v / 1023 * 255, all-ones tables.  With uint8 input the decoded
# pixel, an integer, is within 1 level of the integer input, so the decoder's value
# before its final rounding is within 1.5 of it; a 10-bit input's luma lies between
# the integers, and the same 1.5 bounds |rounded - luma|: each is within the
# quantiser's and the integer IDCT's error (< 1) plus the final rounding (<= 0.5).
# Worst measured over the cases here: 1.37 (257x33).
MAXVAL_1023_BOUND = 1.5

_spec = importlib.util.spec_from_file_location("make_gray_fixtures", os.path.join(GOLDEN, "make_gray_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)

_cache = {}


def plane(w, h, kind):
    rng = np.random.default_rng(100 * w + h)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        return ((xx * 3 + yy * 5) % 256).astype(np.uint8)
    if kind == "u16":
        return rng.integers(0, 1024, (h, w)).astype(np.uint16)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def case(w, h, ri, kind="u8", transfer=gray_ref.AS_RGB):
    """(plane, blocks, file) of the seeded case, computed once"""
    key = (w, h, ri, kind, transfer)
    if key not in _cache:
        g = plane(w, h, kind)
        maxval = 1023 if kind == "u16" else 255
        zz = gray_ref.blocks(g, maxval, ONES, transfer)
        _cache[key] = (g, zz, gray_ref.encode_blocks(zz, w, h, ONES, ri))
    return _cache[key]


@pytest.mark.parametrize("ri", RIS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("transfer", [gray_ref.AS_RGB, gray_ref.Y_FULL_RANGE])
def test_decoder_returns_the_blocks(w, h, ri, transfer):
    _, zz, data = case(w, h, ri, transfer=transfer)
    jf, got, padding_ok = jpeg_scan.decode_coefficients(data)
    assert (jf.width, jf.height) == (w, h)
    assert padding_ok
    assert zz.shape == (-(-w // 8) * -(-h // 8), 64)
    assert got.shape == zz.shape and np.array_equal(got, zz)


@pytest.mark.parametrize("ri", RIS)
@pytest.mark.parametrize("w,h", SIZES)
def test_header_has_one_component(w, h, ri):
    _, _, data = case(w, h, ri)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    segs, i = [], 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        segs.append((data[i + 1], data[i + 4:i + 2 + n]))
        i += 2 + n
    sos = data[i:i + 10]
    kinds = [m for m, _ in segs]
    assert kinds == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4] + ([0xDD] if ri else [])
    assert segs[1][1][0] == 0 and len(segs[1][1]) == 65                      # one DQT, Tq 0
    sof = segs[2][1]
    assert len(sof) == 9 and sof[0] == 8 and sof[5:] == bytes([1, 1, 0x11, 0])  # length 11, Nf 1, 01 11 00
    assert (int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big")) == (h, w)
    ids = [(s[1][0] >> 4, s[1][0] & 15) for s in segs[3:5]]
    assert ids == [(1, 1), (0, 0)] and set(ids) == {(0, 0), (1, 1)}          # luma AC, then luma DC
    if ri:
        assert segs[5][1] == ri.to_bytes(2, "big")
    assert sos == bytes([0xFF, 0xDA, 0x00, 0x08, 0x01, 0x01, 0x01, 0x00, 0x3F, 0x00])


@pytest.mark.parametrize("ri", RIS)
@pytest.mark.parametrize("w,h", SIZES)
def test_blocks_are_the_luma_blocks_of_the_colour_file(w, h, ri):
    g, _, data = case(w, h, ri)
    colour = oracle.encode(np.repeat(g[:, :, None], 3, axis=2), 255, oracle.P444, ONES, ONES, restart_interval=ri)
    _, want, _ = jpeg_scan.decode_coefficients(colour)
    _, got, _ = jpeg_scan.decode_coefficients(data)
    assert np.array_equal(got, want[0::3])


@pytest.mark.parametrize("ri", RIS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["u8", "smooth"])
def test_pillow_reads_mode_l_within_one_level(w, h, ri, kind):
    pytest.importorskip("PIL")
    from PIL import Image
    g, _, data = case(w, h, ri, kind)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "L" and im.size == (w, h)
    err = np.abs(np.asarray(im).astype(np.int32) - g.astype(np.int32)).max()
    print(f"{w}x{h} ri {ri} {kind}: worst |pillow - input| = {err}")
    assert err <= 1, err


@pytest.mark.parametrize("ri", RIS)
@pytest.mark.parametrize("w,h", SIZES + [(20, 9)])
def test_pillow_at_maxval_1023(w, h, ri):
    pytest.importorskip("PIL")
    from PIL import Image
    g, _, data = case(w, h, ri, "u16")
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "L" and im.size == (w, h)
    err = np.abs(np.asarray(im).astype(np.float64) - g.astype(np.float64) / 1023 * 255).max()
    print(f"{w}x{h} ri {ri} maxval 1023: worst |pillow - v/1023*255| = {err:.3f}")
    assert err <= MAXVAL_1023_BOUND, err


@pytest.mark.parametrize("kind", list(fixtures.KINDS))
def test_goldens(kind):
    with open(fixtures.golden_path(kind), "rb") as f:
        assert fixtures.make(kind) == f.read()
