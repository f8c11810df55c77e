"""Pins the CPU yardstick of the YCbCr matrix step (tests/ycc_matrix_ref.py):
  1. the six f32 constants of BT.709 and BT.2020 are the header's, bit for bit, and
     what dmmt_ycc_matrix_coefficients returns;
  2. the f32 step stays within n * 2^-17 of the float64 formula, n the number of f32
     roundings involved, every one at a magnitude below 256 (half an ulp there is 2^-17):
     a rounded constant times a value of at most 128 (2^-24 * 128 = 2^-17 each, two per
     output) and the operations themselves -- two products and two sums for Y' (n = 6),
     two products and one sum for Cb' and Cr' (n = 5); the clamps are exact and cannot
     widen a difference;
  3. grey planes (chroma at the centre code) give ycc_levels_ref's bytes: grey maps to grey;
  4. a colour-patch RGB image taken to BT.709 / BT.2020 YCbCr in float64, rounded to codes
     (8-bit limited, 10-bit limited at the top of a uint16, 10-bit full) and run through
     the reference lands on the float64 BT.601 YCbCr of the same RGB within the half-code
     quantisation of its inputs, 0.5 (kY + (a+b) kC) + 2^-10 for luma and
     0.5 kC (|c|+|d|) + 2^-10 (Cr': e, f) for chroma;
  5. the same planes written as they are (JFIF) miss that bound by more than 10 levels on
     saturated patches;
  6. an odd-sized 7 x 17 frame with saturated chroma has padded luma of exactly -128;
  7. three committed goldens match byte for byte."""
import importlib.util
import os

import numpy as np
import pytest

import dmmt_jpeg
import ycc_levels_ref as lv
import ycc_matrix_ref as mx
import ycc_ref
from conftest import GOLDEN

ONES = [1] * 64
HEX = {mx.BT709: ["0x1.a0115cp-4", "0x1.91906ep-3", "0x1.face1ep-1", "-0x1.c53b92p-4", "-0x1.28c470p-4",
                  "0x1.f77fecp-1"],
       mx.BT2020: ["0x1.e2dd64p-4", "0x1.b036e8p-4", "0x1.fd8c3cp-1", "-0x1.e7d3a4p-5", "-0x1.586952p-4",
                   "0x1.f3fa3ap-1"]}
DECIMAL = {mx.BT709: [0.101579, 0.196076, 0.989854, -0.110653, -0.072453, 0.983398],
           mx.BT2020: [0.117887, 0.105521, 0.995211, -0.059549, -0.084085, 0.976518]}
IDS = {mx.BT709: "709", mx.BT2020: "2020"}
matrices = pytest.mark.parametrize("matrix", mx.MATRICES, ids=[IDS[m] for m in mx.MATRICES])
# (bit_depth, shift, range)
LEVELS = {"8L": (8, 0, lv.LIMITED), "10L": (10, 6, lv.LIMITED), "10F": (10, 0, lv.FULL)}

_spec = importlib.util.spec_from_file_location("make_ycc_matrix_fixtures",
                                               os.path.join(GOLDEN, "make_ycc_matrix_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)


# ------------------------------------------------------------------ 1

@matrices
def test_constants_are_the_headers(matrix):
    want = [float.fromhex(h) for h in HEX[matrix]]
    got = mx.constants(matrix)
    assert all(isinstance(x, np.float32) for x in got)
    assert [float(x) for x in got] == want
    assert np.allclose(want, DECIMAL[matrix], rtol=0, atol=5e-7)
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    assert list(dmmt_jpeg.ycc_matrix_coefficients(matrix)) == want


@matrices
def test_constants_are_f601_times_the_inverse_of_the_source(matrix):
    """[Y' Cb' Cr'] = F601 inverse(Fsrc) [Y Cb Cr], F the RGB -> YCbCr matrix of its Kr, Kb:
    first column (1, 0, 0) -- grey maps to grey --, then (a, c, e) and (b, d, f)"""
    def forward(kr, kb):
        kg = 1.0 - kr - kb
        y = np.array([kr, kg, kb])
        return np.stack([y, (np.array([0, 0, 1.0]) - y) / (2 * (1 - kb)), (np.array([1.0, 0, 0]) - y) / (2 * (1 - kr))])
    m = forward(*mx.KR_KB[mx.JFIF]) @ np.linalg.inv(forward(*mx.KR_KB[matrix]))
    a, b, c, d, e, f = mx.constants64(matrix)
    assert np.allclose(m, [[1, a, b], [0, c, d], [0, e, f]], rtol=0, atol=1e-14)


# ------------------------------------------------------------------ 2

@matrices
def test_the_f32_step_stays_near_the_float64_formula(matrix):
    r = np.random.default_rng(5 + matrix)
    # transferred 10-bit codes of both ranges, and the corners of the cube
    y = np.concatenate([lv.luma_in(r.integers(0, 1024, 200000), 10, lv.LIMITED),
                        lv.luma_in(r.integers(0, 1024, 200000), 10, lv.FULL)])
    cb, cr = (np.concatenate([lv.chroma_in(r.integers(0, 1024, 200000), 10, lv.LIMITED),
                              lv.chroma_in(r.integers(0, 1024, 200000), 10, lv.FULL)]) for _ in range(2))
    corners = np.array([[p, q, s] for p in (-128, 127) for q in (-128, 127) for s in (-128, 127)], np.float32)
    y, cb, cr = (np.concatenate([v, corners[:, i]]) for i, v in enumerate((y, cb, cr)))
    assert y.dtype == cb.dtype == cr.dtype == np.float32
    a, b, c, d, e, f = mx.constants64(matrix)
    y64, cb64, cr64 = (v.astype(np.float64) for v in (y, cb, cr))
    exact = (np.clip(y64 + a * cb64 + b * cr64, -128, 127), np.clip(c * cb64 + d * cr64, -128, 127),
             np.clip(e * cb64 + f * cr64, -128, 127))
    # every intermediate of the step lies below 256, where half an ulp of f32 is 2^-17
    assert 128 * (1 + abs(a) + abs(b)) < 256 and 128 * (abs(c) + abs(d)) < 256 and 128 * (abs(e) + abs(f)) < 256
    for name, got, want, n in zip(("Y'", "Cb'", "Cr'"), mx.step(y, cb, cr, matrix), exact, (6, 5, 5)):
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{IDS[matrix]} {name}: worst |f32 - f64| = {err:.3e}, bound {n * 2.0 ** -17:.3e}")
        assert err <= n * 2.0 ** -17, (name, err)
        assert got.min() == -128 and got.max() == 127  # the corners clamp both ways


# ------------------------------------------------------------------ 3

@matrices
@pytest.mark.parametrize("level", sorted(LEVELS) + ["8F"])
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_grey_planes_are_written_as_they_are(sub, level, matrix):
    depth, shift, rng = LEVELS.get(level, (8, 0, lv.FULL))
    w, h = 33, 9
    y = lv.random_planes(w, h, sub, 3 + sub, depth, shift)[0]
    centre = np.full(ycc_ref.chroma_shape(w, h, sub), (1 << (depth - 1)) << shift, y.dtype)
    want = lv.encode(y, centre, centre, sub, ONES, ONES, depth, shift, rng)
    assert mx.encode(y, centre, centre, sub, ONES, ONES, matrix, depth, shift, rng) == want
    assert mx.encode(y, centre, centre, sub, ONES, ONES, mx.JFIF, depth, shift, rng) == want


# ------------------------------------------------------------------ 4, 5

# Patches of 8 x 8 pixels.  The bound of (4) is the half-code quantisation of the inputs
# alone, so every patch keeps its exact values inside the transfer's and the step's clamps
# under all three matrices: the bars are at 10% and 90% amplitude, not 0 and 100%.
LO, HI = 26.0, 230.0
BARS = {"red": (HI, LO, LO), "green": (LO, HI, LO), "blue": (LO, LO, HI), "cyan": (LO, HI, HI),
        "magenta": (HI, LO, HI), "yellow": (HI, HI, LO)}
OTHERS = {"black": (0, 0, 0), "white": (255, 255, 255), "grey": (128, 128, 128), "skin": (224, 172, 138),
          "sky": (96, 150, 220), "leaf": (60, 120, 40), "orange": (230, 120, 30), "violet": (110, 50, 170)}
PATCHES = {**BARS, **OTHERS}


def patch_image():
    rgb = np.zeros((8, 8 * len(PATCHES), 3), np.float64)
    for i, v in enumerate(PATCHES.values()):
        rgb[:, 8 * i:8 * i + 8] = v
    return rgb


def codes_of(rgb, matrix, level):
    """the planes a decoder hands over: float64 YCbCr under `matrix`, rounded to the level's codes"""
    depth, shift, rng = LEVELS[level]
    off_y, k_y, off_c, k_c = (float(x) for x in lv.constants(depth, rng))
    yy, cb, cr = mx.rgb_to_ycc64(rgb, matrix)
    dt = np.uint8 if depth == 8 else np.uint16
    planes = []
    for v, off, k in ((yy, off_y, k_y), (cb, off_c, k_c), (cr, off_c, k_c)):
        code = np.rint(off + v / k)
        assert code.min() >= 0 and code.max() <= (1 << depth) - 1
        assert np.abs(off + v / k - code).max() <= 0.5
        planes.append((code.astype(np.uint32) << shift).astype(dt))
    return planes, k_y, k_c


@matrices
@pytest.mark.parametrize("level", sorted(LEVELS))
def test_colour_patches_land_on_bt601(level, matrix):
    depth, shift, rng = LEVELS[level]
    rgb = patch_image()
    planes, k_y, k_c = codes_of(rgb, matrix, level)
    for m in (matrix, mx.JFIF):  # no patch meets a clamp: the bound below is quantisation alone
        yy, cb, cr = mx.rgb_to_ycc64(rgb, m)
        # (white's luma is 255 up to the float64 rounding of Kr + Kg + Kb)
        assert max(np.abs(cb).max(), np.abs(cr).max()) < 127 and 0 <= yy.min() and yy.max() <= 255 + 1e-9
    y601, cb601, cr601 = mx.rgb_to_ycc64(rgb, mx.JFIF)
    want = (y601 - 128.0, cb601, cr601)
    a, b, c, d, e, f = (float(x) for x in mx.constants(matrix))
    bounds = (0.5 * (k_y + (a + b) * k_c) + 2.0 ** -10, 0.5 * k_c * (abs(c) + abs(d)) + 2.0 ** -10,
              0.5 * k_c * (abs(e) + abs(f)) + 2.0 ** -10)
    got = mx.padded_planes(*planes, 0, matrix, depth, shift, rng)
    plain = mx.padded_planes(*planes, 0, mx.JFIF, depth, shift, rng)
    miss = {}
    for name, g, p, w_, bound in zip(("Y'", "Cb'", "Cr'"), got, plain, want, bounds):
        err = np.abs(g.astype(np.float64) - w_)
        print(f"{IDS[matrix]} {level} {name}: worst |reference - BT.601| = {err.max():.4f}, bound {bound:.4f}")
        assert err.max() <= bound, (name, err.max(), bound)
        off = np.abs(p.astype(np.float64) - w_) - bound  # how far the planes as they are miss it
        for i, patch in enumerate(PATCHES):
            miss[patch] = max(miss.get(patch, 0.0), float(off[:, 8 * i:8 * i + 8].max()))
    print({k: round(v, 2) for k, v in miss.items()})
    # (5) written as they are: saturated green is tens of levels off under both matrices, red
    # under BT.709; the greys are right whatever the matrix
    assert miss["green"] > 10 and max(miss[p] for p in BARS) > 10
    if matrix == mx.BT709:
        assert miss["red"] > 10
    assert all(miss[p] <= 0 for p in ("black", "white", "grey"))


# ------------------------------------------------------------------ 6

@matrices
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_padding_is_black_after_the_matrix(sub, matrix):
    w, h = 7, 17
    for level in LEVELS.values():
        depth, shift, rng = level
        top = (1 << depth) - 1
        y = lv.random_planes(w, h, sub, 9, depth, shift)[0]
        shape = ycc_ref.chroma_shape(w, h, sub)
        for cbv, crv in ((top, top), (0, top), (top, 0), (0, 0)):
            cb, cr = np.full(shape, cbv << shift, y.dtype), np.full(shape, crv << shift, y.dtype)
            yp, cbp, crp = mx.padded_planes(y, cb, cr, sub, matrix, depth, shift, rng)
            assert yp.shape[0] > h and yp.shape[1] > w
            assert np.all(yp[h:] == -128) and np.all(yp[:, w:] == -128)
            assert np.any(yp[:h, :w] != lv.padded_planes(y, cb, cr, sub, depth, shift, rng)[0][:h, :w])
            ch, cw = shape
            assert np.all(cbp[ch:] == 0) and np.all(cbp[:, cw:] == 0) and np.all(crp[ch:] == 0) and np.all(crp[:, cw:] == 0)
            assert np.all(cbp[:ch, :cw] != 0) and np.all(crp[:ch, :cw] != 0)


# ------------------------------------------------------------------ 7

@pytest.mark.parametrize("name", sorted(fixtures.CASES))
def test_goldens(name):
    with open(fixtures.golden_path(name), "rb") as f:
        assert fixtures.make(name) == f.read()
