"""Pins the CPU yardstick of the YCbCr sample levels (tests/ycc_levels_ref.py) without
the library, for seeded random planes in every subsampling:
  1. 8 bits, full range gives exactly ycc_ref.encode's bytes, in uint8 or uint16 samples;
  2. every code of 8, 10, 12 and 16 bits, both ranges, transfers to within 2^-14 of the
     float64 formula (two roundings at magnitude <= 255, each <= 2^-17 relative to 256:
     about 4e-5 < 2^-14 = 6.1e-5; measured worst 1.42e-5);
  3. the oracle's own JPEG decoder gives back the helper's coefficients;
  4. with all-ones tables, test_ycc_reference.py's float inverse DCT reproduces the
     transferred planes (+ 128) within 2 levels -- that file's bound, for its reason: the
     quantiser's rounding, 0.5 per coefficient (measured worst 1.42);
  5. a range picked wrong or a wrong shift is off by more than that bound;
  6. three committed goldens match byte for byte."""
import importlib.util
import os

import numpy as np
import pytest

import ycc_levels_ref as lv
import ycc_ref
from conftest import GOLDEN
from oracle import jpeg_scan
from test_ycc_reference import idct_planes

SIZES = [(7, 17), (33, 9), (257, 33)]
SUBS = [0, 1, 2]
ONES = [1] * 64
# (bit_depth, shift, range): 8L, 10L (the bits at the top, P010), 10F, 12L, 16L, 16F
LEVELS = [(8, 0, lv.LIMITED), (10, 6, lv.LIMITED), (10, 0, lv.FULL), (12, 4, lv.LIMITED), (16, 0, lv.LIMITED),
          (16, 0, lv.FULL)]
LEVEL_IDS = ["8L", "10L", "10F", "12L", "16L", "16F"]

_spec = importlib.util.spec_from_file_location("make_ycc_levels_fixtures",
                                               os.path.join(GOLDEN, "make_ycc_levels_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)

_cache = {}


def case(w, h, sub, level):
    """(planes, coefficients) of the seeded case, computed once"""
    key = (w, h, sub, level)
    if key not in _cache:
        depth, shift, rng = level
        planes = lv.random_planes(w, h, sub, 1000 * sub + w + depth, depth, shift, low_bits=True)
        _cache[key] = (planes, lv.coefficients(*planes, sub, ONES, ONES, depth, shift, rng))
    return _cache[key]


def full_range_planes(planes, depth, shift, rng):
    """what an inverse DCT should give back: the transferred samples + 128, float64"""
    return [lv.luma_in(lv.codes(planes[0], shift), depth, rng).astype(np.float64) + 128.0] + \
           [lv.chroma_in(lv.codes(p, shift), depth, rng).astype(np.float64) + 128.0 for p in planes[1:]]


# ------------------------------------------------------------------ 1

@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_8_bit_full_range_is_ycc_ref(w, h, sub):
    planes = ycc_ref.random_planes(w, h, sub, 31 * sub + w)
    want = ycc_ref.encode(*planes, sub, ONES, ONES)
    assert lv.encode(*planes, sub, ONES, ONES) == want
    assert lv.encode(*[p.astype(np.uint16) for p in planes], sub, ONES, ONES, 8, 0, lv.FULL) == want
    # the bits at the top of a uint16, garbage below
    wide = [(p.astype(np.uint16) << 8) | 0xA5 for p in planes]
    assert lv.encode(*wide, sub, ONES, ONES, 8, 8, lv.FULL) == want
    q = list(range(1, 65))
    assert lv.encode(*planes, sub, q, q[::-1], restart_interval=3) == ycc_ref.encode(*planes, sub, q, q[::-1],
                                                                                     restart_interval=3)


# ------------------------------------------------------------------ 2

@pytest.mark.parametrize("rng", [lv.FULL, lv.LIMITED], ids=["full", "limited"])
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_every_code_transfers_within_2_to_the_minus_14(depth, rng):
    v = np.arange(1 << depth, dtype=np.uint32)
    for chroma, got in ((False, lv.luma_in(v, depth, rng)), (True, lv.chroma_in(v, depth, rng))):
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - lv.exact(v, depth, rng, chroma)).max()
        print(f"{depth} bits, range {rng}, chroma {chroma}: worst |f32 - f64| = {err:.3e}")
        assert err <= 2.0 ** -14, (chroma, err)
        assert got.min() >= -128 and got.max() <= 127  # the DCT's input range
    # black, white and neutral land where they should; below black and above white clamp
    m = 1 << (depth - 8)
    if rng == lv.LIMITED:
        assert lv.luma_in(np.array([0, 16 * m, 235 * m, (1 << depth) - 1]), depth, rng).tolist() == [-128, -128, 127, 127]
        assert lv.chroma_in(np.array([0, 128 * m, (1 << depth) - 1]), depth, rng).tolist() == [-128, 0, 127]
    else:
        assert lv.luma_in(np.array([0, (1 << depth) - 1]), depth, rng).tolist() == [-128, 127]
        assert lv.chroma_in(np.array([1 << (depth - 1)]), depth, rng).tolist() == [0]
    if depth == 8 and rng == lv.FULL:  # exactly v - 128: ycc_ref's contract
        assert np.array_equal(lv.luma_in(v, 8, rng), v.astype(np.float32) - 128)
        assert np.array_equal(lv.chroma_in(v, 8, rng), v.astype(np.float32) - 128)


# ------------------------------------------------------------------ 3, 4, 5

@pytest.mark.parametrize("level", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_decoder_returns_the_coefficients(w, h, sub, level):
    depth, shift, rng = level
    planes, coef = case(w, h, sub, level)
    data = lv.encode(*planes, sub, ONES, ONES, depth, shift, rng)
    jf, got, padding_ok = jpeg_scan.decode_coefficients(data)
    assert (jf.width, jf.height) == (w, h)
    assert padding_ok
    assert got.shape == coef.shape and np.array_equal(got, coef)


@pytest.mark.parametrize("level", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_idct_reproduces_the_transferred_planes(w, h, sub, level):
    depth, shift, rng = level
    planes, coef = case(w, h, sub, level)
    rec = idct_planes(coef, w, h, sub)
    for name, p, r in zip("y cb cr".split(), full_range_planes(planes, depth, shift, rng), rec):
        err = np.abs(r[:p.shape[0], :p.shape[1]] - p).max()
        print(f"{w}x{h} sub {sub} {depth} bits shift {shift} range {rng} {name}: worst |idct - transfer| = {err:.3f}")
        assert err <= 2.0, (name, err)
    # the padding: black after the transfer (luma 0, chroma 128 in full-range levels)
    y, cb, _ = rec
    if y.shape[1] > w:
        assert np.abs(y[:h, w:]).max() <= 2.0
        assert np.abs(cb[:planes[1].shape[0], planes[1].shape[1]:] - 128).max() <= 2.0


@pytest.mark.parametrize("level", LEVELS, ids=LEVEL_IDS)
@pytest.mark.parametrize("sub", SUBS)
def test_wrong_settings_are_caught(sub, level):
    """the planes decoded back do not fit the other range, nor a shift one off"""
    w, h = 33, 9
    depth, shift, rng = level
    planes, coef = case(w, h, sub, level)
    rec = idct_planes(coef, w, h, sub)
    wrong = [(depth, shift, 1 - rng)]
    if shift:  # one bit fewer: every code doubles (clamped reading them is still far off)
        wrong.append((depth, shift - 1, rng))
    if shift < 16 - depth:
        wrong.append((depth, shift + 1, rng))
    for wd, ws, wr in wrong:
        # (a wrong shift may produce codes above 2^B - 1: this is the transfer alone)
        other = [lv.luma_in(np.minimum(lv.codes(planes[0], ws), (1 << wd) - 1), wd, wr).astype(np.float64) + 128.0] + \
                [lv.chroma_in(np.minimum(lv.codes(p, ws), (1 << wd) - 1), wd, wr).astype(np.float64) + 128.0
                 for p in planes[1:]]
        for name, p, r in zip("y cb cr".split(), other, rec):
            err = np.abs(r[:p.shape[0], :p.shape[1]] - p).max()
            assert err > 2.0, (name, (wd, ws, wr), err)


# ------------------------------------------------------------------ 6

@pytest.mark.parametrize("name", sorted(fixtures.CASES))
def test_goldens(name):
    with open(fixtures.golden_path(name), "rb") as f:
        assert fixtures.make(name) == f.read()
