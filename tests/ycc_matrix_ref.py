"""The CPU yardstick of the YCbCr matrix step (dmmt_encode_device_ycc_matrix) -- TEST
INFRASTRUCTURE, composed from tests/ycc_levels_ref.py, tests/ycc_ref.py and what
oracle/ exports.

The contract (include/dmmt_jpeg.h, "YCbCr matrix"): with the source's Kr, Kb,
Kg = 1 - Kr - Kb (BT.709: 0.2126, 0.0722; BT.2020: 0.2627, 0.0593) and the target's
Kr' = 0.299, Kb' = 0.114, Kg' = 0.587, in double precision, each rounded once to f32,

    a = Kb' 2(1-Kb) - Kg' 2Kb(1-Kb)/Kg        b = Kr' 2(1-Kr) - Kg' 2Kr(1-Kr)/Kg
    c = (2(1-Kb) - a) / (2(1-Kb'))            d = -b / (2(1-Kb'))
    e = -a / (2(1-Kr'))                       f = (2(1-Kr) - b) / (2(1-Kr'))

and with y, cb, cr the values ycc_levels_ref feeds the DCT, in IEEE f32, every
operation rounded once, in this order,

    Y'  = min(max((y + a*cb) + b*cr, -128), 127)
    Cb' = min(max(c*cb + d*cr, -128), 127)
    Cr' = min(max(e*cb + f*cr, -128), 127)

The luma sample at (x, y) takes the chroma position (x // hr, y // vr); the padding is
black after the matrix (luma -128 outside the rectangle whatever chroma shares the
cell, chroma 0).  JFIF is no step at all: ycc_levels_ref itself.  From there on
ycc_levels_ref's stages.  tests/test_ycc_matrix_reference.py pins this helper; the GPU
tests compare against it byte for byte."""
from __future__ import annotations

import numpy as np

import oracle
import ycc_levels_ref as lv
import ycc_ref
from oracle import np_ref

JFIF, BT709, BT2020 = 0, 1, 2
MATRICES = (BT709, BT2020)
KR_KB = {JFIF: (0.299, 0.114), BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}
f32 = np.float32


def constants64(matrix):
    """(a, b, c, d, e, f) in float64"""
    assert matrix in MATRICES
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    tr, tb, tg = 0.299, 0.114, 0.587
    a = tb * 2 * (1 - kb) - tg * 2 * kb * (1 - kb) / kg
    b = tr * 2 * (1 - kr) - tg * 2 * kr * (1 - kr) / kg
    return (a, b, (2 * (1 - kb) - a) / (2 * (1 - tb)), -b / (2 * (1 - tb)), -a / (2 * (1 - tr)),
            (2 * (1 - kr) - b) / (2 * (1 - tr)))


def constants(matrix):
    """(a, b, c, d, e, f) as float32: float64 rounded once"""
    return tuple(f32(x) for x in constants64(matrix))


def clamp(v):
    return np.minimum(np.maximum(v, f32(-128)), f32(127))


def step(y, cb, cr, matrix):
    """the float32 step on arrays of one shape (cb, cr already at the luma's positions
    for Y'): returns (Y', Cb', Cr')"""
    a, b, c, d, e, f = constants(matrix)
    y, cb, cr = (np.asarray(p, np.float32) for p in (y, cb, cr))
    yy = clamp((y + a * cb) + b * cr)
    cbb = clamp(c * cb + d * cr)
    crr = clamp(e * cb + f * cr)
    assert yy.dtype == cbb.dtype == crr.dtype == np.float32
    return yy, cbb, crr


def padded_planes(y, cb, cr, sub, matrix, bit_depth=8, shift=0, rng=lv.FULL):
    """the float32 planes the DCT sees: transferred, through the matrix, padded black"""
    yp, cbp, crp = lv.padded_planes(y, cb, cr, sub, bit_depth, shift, rng)
    if matrix == JFIF:
        return [yp, cbp, crp]
    h, w = y.shape
    hr, vr = ycc_ref.rates(sub)
    a, b, c, d, e, f = constants(matrix)
    up = lambda p: np.repeat(np.repeat(p, vr, axis=0), hr, axis=1)  # noqa: E731  (x // hr, y // vr)
    yy = clamp((yp + a * up(cbp)) + b * up(crp))
    assert yy.dtype == np.float32 and yy.shape == yp.shape
    out = np.full(yp.shape, f32(-128.0), np.float32)
    out[:h, :w] = yy[:h, :w]
    return [out, clamp(c * cbp + d * crp), clamp(e * cbp + f * crp)]


def coefficients(y, cb, cr, sub, luma_q, chroma_q, matrix, bit_depth=8, shift=0, rng=lv.FULL):
    """(nblocks, 64) int16 zigzag blocks in MCU emission order, as ycc_ref.coefficients"""
    yp, cbp, crp = padded_planes(y, cb, cr, sub, matrix, bit_depth, shift, rng)
    yb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(yp)), luma_q).reshape(-1, 64)
    cbb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(cbp)), chroma_q).reshape(-1, 64)
    crb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(crp)), chroma_q).reshape(-1, 64)
    return np_ref.interleave(yb, cbb, crb, sub, yp.shape[1] // 8)[:, np_ref.ZIGZAG]


def encode(y, cb, cr, sub, luma_q, chroma_q, matrix, bit_depth=8, shift=0, rng=lv.FULL, restart_interval=0) -> bytes:
    """the JPEG file dmmt_encode_device_ycc_matrix must write for these planes"""
    h, w = y.shape
    return oracle.encode_coefficients(coefficients(y, cb, cr, sub, luma_q, chroma_q, matrix, bit_depth, shift, rng),
                                      w, h, sub, luma_q, chroma_q, restart_interval=restart_interval)


def rgb_to_ycc64(rgb, matrix):
    """float64 full-range YCbCr (Y in 0..255, chroma centred on 0) of float64 RGB in
    0..255 under `matrix` (JFIF: BT.601)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    r, g, b = (np.asarray(rgb, np.float64)[..., i] for i in range(3))
    yy = kr * r + kg * g + kb * b
    return yy, (b - yy) / (2 * (1 - kb)), (r - yy) / (2 * (1 - kr))
