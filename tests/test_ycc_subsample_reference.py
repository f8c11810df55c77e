"""Pins the CPU yardstick of YCbCr planes finer than the file (tests/ycc_subsample_ref.py),
against which the GPU tests compare byte for byte:
  1. equal samplings are tests/ycc_matrix_ref.py itself;
  2. the three formulas, written out in numpy float32, against oracle.subsample_resort
     (the oracle's restatement of the reference's stage) and np_ref's block order;
  3. a known-answer 2 x 2 cell of float32 values that two other summation orders
     round differently, and how often random 10-bit limited cells do;
  4. uint8 planes against exact integer arithmetic, (sum - 128 n) / n;
  5. odd widths and heights average the last sample with the padding's 0;
  6. every averaged value stays within [-128, 127], saturated planes included;
  7. averaging is not taking the top-left sample;
  8. three committed goldens match byte for byte."""
import importlib.util
import os

import numpy as np
import pytest

import oracle
import ycc_levels_ref as lv
import ycc_matrix_ref as mx
import ycc_ref
import ycc_subsample_ref as ss
from conftest import GOLDEN
from oracle import np_ref

f32 = np.float32
ONES = [1] * 64
WIDTHS = [1, 7, 255, 256, 257, 513]
HEIGHTS = [1, 17, 33]
# (matrix, bit_depth, shift, range)
KINDS = {"u8-full": (mx.JFIF, 8, 0, lv.FULL), "P010-limited-709": (mx.BT709, 10, 6, lv.LIMITED),
         "I010-full-2020": (mx.BT2020, 10, 0, lv.FULL)}
kinds = pytest.mark.parametrize("kind", list(KINDS))
pairs = pytest.mark.parametrize("src,sub", ss.PAIRS, ids=[f"{a}to{b}" for a, b in ss.PAIRS])

_spec = importlib.util.spec_from_file_location("make_ycc_subsample_fixtures",
                                               os.path.join(GOLDEN, "make_ycc_subsample_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)


def sizes(seed):
    """a third of the width x height grid per call; three seeds cover it"""
    return [(w, h) for i, w in enumerate(WIDTHS) for j, h in enumerate(HEIGHTS) if (i + j + seed) % 3 == 0]


# ------------------------------------------------------------------ 1

@kinds
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_equal_samplings_are_the_matrix_yardstick(kind, sub):
    matrix, depth, shift, rng = KINDS[kind]
    q = [3] * 64
    for w, h in sizes(sub):
        planes = lv.random_planes(w, h, sub, 7 * w + h, depth, shift)
        assert ss.encode(*planes, sub, sub, q, ONES, matrix, depth, shift, rng) == \
            mx.encode(*planes, sub, q, ONES, matrix, depth, shift, rng), (w, h)


def test_ratios():
    assert [ss.ratios(a, b) for a, b in ss.PAIRS] == [(2, 1), (2, 2), (1, 2)]
    assert all(ss.ratios(s, s) == (1, 1) for s in (0, 1, 2))
    assert [ss.ratios(a, b) for a, b in ((1, 0), (2, 0), (2, 1))] == [None, None, None]  # upsampling


# ------------------------------------------------------------------ 2

def formula(p, rx, ry):
    """the contract's three lines, each written out"""
    p = np.asarray(p, np.float32)
    if (rx, ry) == (2, 1):
        return (p[:, 0::2] + p[:, 1::2]) / f32(2)
    if (rx, ry) == (1, 2):
        return (p[0::2, :] + p[1::2, :]) / f32(2)
    return (((p[0::2, 0::2] + p[1::2, 0::2]) + p[0::2, 1::2]) + p[1::2, 1::2]) / f32(4)


@pytest.mark.parametrize("rx,ry", [(2, 1), (1, 2), (2, 2)])
def test_the_formulas_are_the_references_stage(rx, ry):
    r = np.random.default_rng(10 * rx + ry)
    for hb, wb in ((1, 1), (2, 3), (5, 4)):
        # values as the 10-bit limited transfer leaves them: not multiples of a power of two
        p = lv.chroma_in(r.integers(64, 961, (8 * ry * hb, 8 * rx * wb)), 10, lv.LIMITED)
        want = formula(p, rx, ry)
        assert want.dtype == np.float32 and want.shape == (8 * hb, 8 * wb)
        assert np.array_equal(ss.box(p, rx, ry), want)
        got = oracle.subsample_resort(p, rx, ry, True).reshape(-1, 8, 8)
        assert np.array_equal(got, np_ref.to_blocks(want))
        assert np.array_equal(ss.averaged_blocks(p, rx, ry), got)


# ------------------------------------------------------------------ 3

def orders(tl, bl, tr, br):
    """the cell under the contract's order and under two others"""
    tl, bl, tr, br = (f32(v) for v in (tl, bl, tr, br))
    return (((tl + bl) + tr) + br) / f32(4), (((tl + tr) + bl) + br) / f32(4), ((tl + tr) + (bl + br)) / f32(4)


def test_known_answer_cell_depends_on_the_order():
    """10-bit limited chroma codes 916 (top left), 691 (bottom left), 616 (top right), 692
    (bottom right): the contract's order, a row-major walk and a pairwise tree give three
    different float32 averages"""
    tl, bl, tr, br = (f32(x) for x in lv.chroma_in(np.array([916, 691, 616, 692]), 10, lv.LIMITED))
    assert [float(x).hex() for x in (tl, bl, tr, br)] == ["0x1.cbe9240000000p+6", "0x1.978b6c0000000p+5",
                                                          "0x1.d992480000000p+4", "0x1.99d2480000000p+5"]
    contract, rows_first, pairwise = orders(tl, bl, tr, br)
    assert [float(x).hex() for x in (contract, rows_first, pairwise)] == \
        ["0x1.ed7e460000000p+5", "0x1.ed7e4a0000000p+5", "0x1.ed7e480000000p+5"]
    plane = np.zeros((16, 16), np.float32)
    plane[:2, :2] = [[tl, tr], [bl, br]]
    assert oracle.subsample_resort(plane, 2, 2, True)[0] == contract
    assert ss.box(plane, 2, 2)[0, 0] == contract
    # and through the whole composition: the planes of that cell
    y = np.zeros((2, 2), np.uint16)
    cb = (np.array([[916, 616], [691, 692]]) << 6).astype(np.uint16)
    _, cbp, _ = ss.padded_planes(y, cb, cb, 0, 2, mx.JFIF, 10, 6, lv.LIMITED)
    assert ss.averaged_blocks(cbp, 2, 2)[0, 0, 0] == contract


def test_random_limited_cells_often_depend_on_the_order():
    r = np.random.default_rng(3)
    v = lv.chroma_in(r.integers(64, 961, (4, 20000)), 10, lv.LIMITED)
    contract, rows_first, pairwise = (((v[0] + v[1]) + v[2]) + v[3]) / f32(4), \
        (((v[0] + v[2]) + v[1]) + v[3]) / f32(4), ((v[0] + v[2]) + (v[1] + v[3])) / f32(4)
    differ = np.mean((contract != rows_first) | (contract != pairwise))
    assert differ > 0.2, differ  # byte parity on such planes does test the order


# ------------------------------------------------------------------ 4

@pairs
def test_uint8_planes_against_integers(src, sub):
    rx, ry = ss.ratios(src, sub)
    n = rx * ry
    for w, h in sizes(src + sub):
        y, cb, cr = ycc_ref.random_planes(w, h, src, 31 * w + h)
        _, cbp, crp = ss.padded_planes(y, cb, cr, src, sub)
        for c, cp in ((cb, cbp), (cr, crp)):
            codes = np.full(cp.shape, 128, np.int64)  # the padding: code 128 is the value 0
            codes[:c.shape[0], :c.shape[1]] = c
            total = sum(codes[yy::ry, xx::rx] for xx in range(rx) for yy in range(ry))
            exact = (total - 128 * n) / n  # float64: exact (quarters of small integers)
            got = ss.box(cp, rx, ry)
            assert np.array_equal(got.astype(np.float64), exact), (w, h)
            assert np.array_equal(ss.averaged_blocks(cp, rx, ry), np_ref.to_blocks(got))


# ------------------------------------------------------------------ 5

@pairs
def test_odd_sizes_average_with_zero(src, sub):
    rx, ry = ss.ratios(src, sub)
    w, h = 7, 17  # 4:4:4 planes: 7 columns, 17 rows; 4:2:2 planes: 4 columns, 17 rows
    y = np.full((h, w), 100, np.uint8)
    ch, cw = ycc_ref.chroma_shape(w, h, src)
    cb = np.full((ch, cw), 228, np.uint8)  # the value 100
    cr = np.full((ch, cw), 28, np.uint8)   # -100
    _, cbp, crp = ss.padded_planes(y, cb, cr, src, sub)
    for cp, v in ((cbp, 100.0), (crp, -100.0)):
        a = ss.box(cp, rx, ry)
        full_c, full_r = cw // rx, ch // ry  # cells wholly inside
        assert np.all(a[:full_r, :full_c] == v)
        if cw % rx:
            assert np.all(a[:full_r, full_c] == v / 2)      # one column of two inside
            assert np.all(a[:, full_c + 1:] == 0)
        if ch % ry:
            assert np.all(a[full_r, :full_c] == v / 2)      # one row of two inside
            assert np.all(a[full_r + 1:, :] == 0)
        if cw % rx and ch % ry:
            assert a[full_r, full_c] == v / 4               # one sample of four, the count stays 4


# ------------------------------------------------------------------ 6

@kinds
@pairs
def test_averaged_values_stay_in_range(src, sub, kind):
    matrix, depth, shift, rng = KINDS[kind]
    rx, ry = ss.ratios(src, sub)
    top = (1 << depth) - 1
    for seed, (lo, hi) in enumerate(((0, top), (top, top), (0, 0))):  # noise, and both ends saturated
        planes = lv.random_planes(33, 17, src, seed, depth, shift, lo=lo, hi=hi)
        _, cbp, crp = ss.padded_planes(*planes, src, sub, matrix, depth, shift, rng)
        for cp in (cbp, crp):
            a = ss.box(cp, rx, ry)
            assert a.min() >= -128 and a.max() <= 127
            if matrix == mx.JFIF and lo == hi:
                assert a[0, 0] == (127 if lo else -128)  # the ends are reached exactly


# ------------------------------------------------------------------ 7

@pairs
def test_averaging_is_not_decimation(src, sub):
    rx, ry = ss.ratios(src, sub)
    w, h = 32, 16
    ch, cw = ycc_ref.chroma_shape(w, h, src)
    yy, xx = np.mgrid[:ch, :cw]
    alt = np.where((xx * (rx == 2) + yy * (ry == 2)) % 2 == 0, 228, 28).astype(np.uint8)  # +100 / -100
    y = np.full((h, w), 128, np.uint8)
    _, cbp, _ = ss.padded_planes(y, alt, alt, src, sub)
    a = ss.box(cbp, rx, ry)
    assert np.all(cbp[0::ry, 0::rx][:ch // ry, :cw // rx] == 100)   # the top-left samples
    assert np.all(a[:ch // ry, :cw // rx] == 0)                     # every cell averages out
    fsub = ycc_ref.chroma_shape(w, h, sub)
    dec = (y, alt[0::ry, 0::rx][:fsub[0], :fsub[1]], alt[0::ry, 0::rx][:fsub[0], :fsub[1]])
    assert ss.encode(y, alt, alt, src, sub, ONES, ONES) != ycc_ref.encode(*dec, sub, ONES, ONES)
    flat = np.full(fsub, 128, np.uint8)
    assert ss.encode(y, alt, alt, src, sub, ONES, ONES) == ycc_ref.encode(y, flat, flat, sub, ONES, ONES)


# ------------------------------------------------------------------ 8

@pytest.mark.parametrize("name", sorted(fixtures.CASES))
def test_goldens(name):
    with open(fixtures.golden_path(name), "rb") as f:
        assert fixtures.make(name) == f.read()
