"""Every front kernel family through the shared LDS layout of the row-transformed
blocks (csrc/front_layout.hpp), byte for byte against the CPU references, at the
smallest shapes that exercise it: 8 x 8 (one block of a partial tile), 256 x 8
(exactly one tile), 264 x 16 (a tile and a partial tile, two tile rows of 4:4:4 and
4:2:2), and for 4:2:0 also 16 x 16 (one MCU) and 520 x 32 (two tiles and a partial
one, two tile rows).  Each shape in every subsampling the family has and in both
block forms, wide and narrow, each on a context of its own (float samples have no
narrow form).  A layout that drops, doubles or misplaces one float of a block, in
the row stores or the column reads, changes a coefficient of noise input."""
import os

import numpy as np
import pytest

import dmmt_jpeg
import test_gpu_gray as gray
import test_gpu_surfaces as surf
import test_gpu_ycc as ycc
import test_gpu_ycc_levels as levels
import test_gpu_ycc_subsample as subsample
import ycc_ref
from dmmt_jpeg import GrayTransfer as GT
from dmmt_jpeg import PixelFormat as PF
from dmmt_jpeg import YccFormat as YF
from dmmt_jpeg import YccMatrix as M

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (256, 8), (264, 16)]
SHAPES_420 = SHAPES + [(16, 16), (520, 32)]
CTX = ["wide", "narrow"]


def shapes(sub):
    return SHAPES_420 if sub == 2 else SHAPES


@pytest.fixture(scope="module")
def q90():
    return dmmt_jpeg.quality_tables(90)


@pytest.fixture(scope="module")
def q50():
    return dmmt_jpeg.quality_tables(50)


@pytest.fixture(scope="module")
def forms():
    """one fresh context per block form"""
    ctx = {}
    for fmt in CTX:
        os.environ["DMMT_COEF_FORMAT"] = fmt
        try:
            ctx[fmt] = dmmt_jpeg.Encoder(0)
        finally:
            os.environ.pop("DMMT_COEF_FORMAT")
    yield ctx
    for enc in ctx.values():
        enc.close()


TIGHT = [(k, c) for k in ("u8", "u16", "f32") for c in CTX if not (k == "f32" and c == "narrow")]


@pytest.mark.parametrize("kind,ctx", TIGHT, ids=[f"{k}-{c}" for k, c in TIGHT])
def test_tight_rgb(forms, q90, kind, ctx):
    enc = forms[ctx]
    for sub in (0, 1, 2):
        o = surf.opts(sub, q90)
        for i, (w, h) in enumerate(shapes(sub)):
            raw, mv, samples = surf.pixels(w, h, kind, 10 * sub + i)
            host = samples if kind == "f32" else raw
            assert enc.encode(dmmt_jpeg.Image.from_array(host, mv), o) == surf.expected(raw, mv, sub, q90), (sub, w, h)


@pytest.mark.parametrize("ctx", CTX)
@pytest.mark.parametrize("fmt", [PF.BGR, PF.PLANAR], ids=["BGR", "PLANAR"])
def test_surfaces(forms, q90, fmt, ctx):
    """uint8 samples, rows one byte longer than tight: every row at another misalignment"""
    enc = forms[ctx]
    for sub in (0, 1, 2):
        o = surf.opts(sub, q90)
        for i, (w, h) in enumerate(shapes(sub)):
            raw, mv, samples = surf.pixels(w, h, "u8", 50 + 10 * sub + i)
            pitch = w * surf.spp_of(fmt) + 1
            s = surf.Surface(enc, samples[None], fmt, pitch, seed=i)
            try:
                got = surf.encode(enc, s.planes(), fmt, pitch, 1, w, h, o, mv, 1)
            finally:
                s.free()
            assert got == [surf.expected(raw, mv, sub, q90)], (sub, w, h)


@pytest.mark.parametrize("ctx", CTX)
@pytest.mark.parametrize("fmt", [YF.PLANAR, YF.NV], ids=["PLANAR", "NV12"])
def test_ycc(forms, q90, fmt, ctx):
    enc = forms[ctx]
    for sub in (0, 1, 2):
        for i, (w, h) in enumerate(shapes(sub)):
            planes = ycc_ref.random_planes(w, h, sub, 100 + 10 * sub + i)
            got = ycc.encode_frames(enc, [planes], fmt, sub, q90, 1, 16, (3, 5, 9), seed=i)
            assert got == [ycc.expected(planes, sub, q90)], (sub, w, h)


@pytest.mark.parametrize("ctx", CTX)
def test_ycc_levels(forms, q50, ctx):
    """P010: video-range 10-bit codes in the high bits of 16-bit samples"""
    enc = forms[ctx]
    for sub in (0, 1, 2):
        for i, (w, h) in enumerate(shapes(sub)):
            planes = levels.planes_for(w, h, sub, 200 + 10 * sub + i, levels.P010)
            got = levels.encode_frames(enc, [planes], YF.NV, sub, q50, levels.P010, 2, 16, (2, 6, 14))
            assert got == [levels.expected(planes, sub, q50, levels.P010)], (sub, w, h)


@pytest.mark.parametrize("ctx", CTX)
@pytest.mark.parametrize("src,sub", subsample.PAIRS, ids=subsample.PAIR_IDS)
def test_ycc_finer_than_the_file(forms, q50, src, sub, ctx):
    """planes at `src`, the file at `sub`: uint8 full-range codes, the BT.709 matrix"""
    enc = forms[ctx]
    for i, (w, h) in enumerate(shapes(sub)):
        planes = subsample.planes_for(w, h, src, 300 + 10 * sub + i, subsample.U8F)
        got = subsample.encode_frames(enc, [planes], YF.PLANAR, src, sub, q50, subsample.U8F, M.BT709, 1, 16, (3, 5, 9))
        assert got == [subsample.expected(planes, src, sub, q50, subsample.U8F, M.BT709)], (src, sub, w, h)


GRAY = [(sb, c) for sb in (1, 2, 4) for c in CTX if not (sb == 4 and c == "narrow")]


@pytest.mark.parametrize("sb,ctx", GRAY, ids=[f"sb{s}-{c}" for s, c in GRAY])
def test_gray(forms, q90, sb, ctx):
    enc = forms[ctx]
    maxval = {1: 255, 2: 1000, 4: 0}[sb]
    for i, (w, h) in enumerate(SHAPES):
        plane = gray.random_plane(w, h, sb, maxval, 400 + i)
        got = gray.encode_plane(enc, plane, q90[0], maxval=maxval, transfer=GT.AS_RGB, extra=1, lead=3 * sb, seed=i)
        gray.check(got, gray.expected(plane, maxval, q90[0]), f"{w}x{h}")
