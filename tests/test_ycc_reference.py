"""Pins the CPU yardstick of the YCbCr input path (tests/ycc_ref.py) without the
library: for seeded random planes in every subsampling, with all-ones tables,
  * the oracle's own JPEG decoder gives back the helper's coefficients;
  * a float inverse DCT of them reproduces every input plane within 2 levels (the
    quantiser's rounding, 0.5 per coefficient, measured worst case 1.43; a wrong
    level shift, plane order or emission order is off by tens);
  * Pillow decodes the file to the same Y (and, for 4:4:4, Cb and Cr) within 2 levels;
  * three committed goldens match byte for byte."""
import importlib.util
import io
import os

import numpy as np
import pytest

import ycc_ref
from conftest import GOLDEN
from oracle import jpeg_scan, np_ref

SIZES = [(7, 17), (33, 9), (257, 33)]
SUBS = [0, 1, 2]
ONES = [1] * 64

_spec = importlib.util.spec_from_file_location("make_ycc_fixtures", os.path.join(GOLDEN, "make_ycc_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)

_cache = {}


def case(w, h, sub):
    """(planes, coefficients, file) of the seeded case, computed once"""
    key = (w, h, sub)
    if key not in _cache:
        planes = ycc_ref.random_planes(w, h, sub, 1000 * sub + w)
        coef = ycc_ref.coefficients(*planes, sub, ONES, ONES)
        _cache[key] = (planes, coef, ycc_ref.encode(*planes, sub, ONES, ONES))
    return _cache[key]


def idct_planes(coef_zz, w, h, sub):
    """emission-order zigzag blocks -> the padded (y, cb, cr) sample planes, float64"""
    hr, vr = ycc_ref.rates(sub)
    wp = -(-w // (8 * hr)) * 8 * hr
    hp = -(-h // (8 * vr)) * 8 * vr
    k = np.arange(8)
    C = np.sqrt(2.0 / 8) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    C[0] = np.sqrt(1.0 / 8)
    nat = np.zeros(coef_zz.shape, np.float64)
    nat[:, np_ref.ZIGZAG] = coef_zz
    px = np.einsum("ui,nuv,vj->nij", C, nat.reshape(-1, 8, 8), C) + 128.0
    out = [np.zeros((hp, wp)), np.zeros((hp // vr, wp // hr)), np.zeros((hp // vr, wp // hr))]
    bpm = hr * vr + 2
    mcux = wp // (8 * hr)
    for e in range(px.shape[0]):
        m, b = divmod(e, bpm)
        mx, my = m % mcux, m // mcux
        if b < hr * vr:  # TL, TR, BL, BR
            bx, by, p = mx * hr + b % hr, my * vr + b // hr, out[0]
        else:
            bx, by, p = mx, my, out[1 + b - hr * vr]
        p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = px[e]
    return out


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_decoder_returns_the_coefficients(w, h, sub):
    _, coef, data = case(w, h, sub)
    jf, got, padding_ok = jpeg_scan.decode_coefficients(data)
    assert (jf.width, jf.height) == (w, h)
    assert padding_ok
    assert got.shape == coef.shape and np.array_equal(got, coef)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_idct_reproduces_the_planes(w, h, sub):
    planes, coef, _ = case(w, h, sub)
    for name, p, rec in zip("y cb cr".split(), planes, idct_planes(coef, w, h, sub)):
        err = np.abs(rec[:p.shape[0], :p.shape[1]] - p).max()
        print(f"{w}x{h} sub {sub} {name}: worst |idct - input| = {err:.3f}")
        assert err <= 2.0, (name, err)
    # the padding: luma black (0), chroma neutral (128)
    y, cb, _ = idct_planes(coef, w, h, sub)
    if y.shape[1] > w:
        assert np.abs(y[:h, w:]).max() <= 2.0 and np.abs(cb[:planes[1].shape[0], planes[1].shape[1]:] - 128).max() <= 2.0


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_pillow_decodes_the_planes(w, h, sub):
    pytest.importorskip("PIL")
    from PIL import Image
    planes, _, data = case(w, h, sub)
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", (w, h))
    im.load()
    assert im.mode == "YCbCr" and im.size == (w, h)
    got = np.asarray(im).astype(np.int32)
    n = 3 if sub == 0 else 1  # subsampled chroma comes back upsampled: not comparable
    for c in range(n):
        err = np.abs(got[:, :, c] - planes[c].astype(np.int32)).max()
        print(f"{w}x{h} sub {sub} channel {c}: worst |pillow - input| = {err}")
        assert err <= 2, (c, err)


@pytest.mark.parametrize("sub", SUBS)
def test_goldens(sub):
    with open(fixtures.golden_path(sub), "rb") as f:
        assert fixtures.make(sub) == f.read()
