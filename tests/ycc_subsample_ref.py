"""The CPU yardstick of YCbCr planes finer than the file
(dmmt_encode_device_ycc_subsample) -- TEST INFRASTRUCTURE, composed from
tests/ycc_matrix_ref.py, tests/ycc_ref.py and what oracle/ exports.

The contract (include/dmmt_jpeg.h, "YCbCr planes finer than the file"): with (shr, svr)
the planes' rates, (hr, vr) the file's, rx = hr / shr and ry = vr / svr, the values are
what ycc_matrix_ref feeds the DCT at the PLANES' sampling (transferred, through the
matrix, the luma at (x, y) with the chroma position (x // shr, y // svr), padded black),
extended with black to the file's padded sizes: luma -128 to Wp x Hp, chroma 0 to
(Wp / shr) x (Hp / svr).  Luma goes on as it is; each chroma plane goes through
oracle.subsample_resort(plane, rx, ry, True), the oracle's restatement of the
reference's own box subsampling (subsampling.rs:102-236), whose output already is in
block order:

    (2, 1)  (p(2i, j) + p(2i+1, j)) / 2
    (1, 2)  (p(i, 2j) + p(i, 2j+1)) / 2
    (2, 2)  (((p(2i, 2j) + p(2i, 2j+1)) + p(2i+1, 2j)) + p(2i+1, 2j+1)) / 4

in float32, every operation rounded once.  From there on ycc_matrix_ref's stages.  Equal
samplings are ycc_matrix_ref itself.  tests/test_ycc_subsample_reference.py pins this
helper; the GPU tests compare against it byte for byte."""
from __future__ import annotations

import numpy as np

import oracle
import ycc_levels_ref as lv
import ycc_matrix_ref as mx
import ycc_ref
from oracle import np_ref

f32 = np.float32
PAIRS = ((0, 1), (0, 2), (1, 2))  # (planes' sampling, file's sampling) that convert
ALL_PAIRS = ((0, 0), (1, 1), (2, 2)) + PAIRS


def ratios(src, sub):
    """(rx, ry) of planes at `src` written as `sub`; None: the file would be finer"""
    shr, svr = ycc_ref.rates(src)
    hr, vr = ycc_ref.rates(sub)
    if hr % shr or vr % svr:
        return None
    return hr // shr, vr // svr


def padded_planes(y, cb, cr, src, sub, matrix=mx.JFIF, bit_depth=8, shift=0, rng=lv.FULL):
    """the float32 planes at the planes' sampling, padded black to the FILE's MCU multiple:
    (luma Hp x Wp, Cb and Cr (Hp / svr) x (Wp / shr))"""
    h, w = y.shape
    shr, svr = ycc_ref.rates(src)
    hr, vr = ycc_ref.rates(sub)
    assert ratios(src, sub) is not None
    wp = -(-w // (8 * hr)) * 8 * hr
    hp = -(-h // (8 * vr)) * 8 * vr
    yp, cbp, crp = mx.padded_planes(y, cb, cr, src, matrix, bit_depth, shift, rng)
    out = [np.full((hp, wp), f32(-128.0), np.float32)]
    out[0][:yp.shape[0], :yp.shape[1]] = yp
    for c in (cbp, crp):
        e = np.zeros((hp // svr, wp // shr), np.float32)
        e[:c.shape[0], :c.shape[1]] = c
        out.append(e)
    return out


def box(plane, rx, ry):
    """the formulas above in numpy float32: the averaged plane in raster order"""
    p = np.asarray(plane, np.float32)
    s = p[0::ry, 0::rx]
    for xx in range(rx):
        for yy in range(ry):
            if xx + yy:
                s = s + p[yy::ry, xx::rx]
    out = s / f32(rx * ry)
    assert out.dtype == np.float32
    return out


def averaged_blocks(plane, rx, ry):
    """(n, 8, 8) float32 blocks of the box-averaged plane, in block raster order: the
    reference's own stage"""
    if rx == 1 and ry == 1:
        return np_ref.to_blocks(np.asarray(plane, np.float32))
    return oracle.subsample_resort(plane, rx, ry, True).reshape(-1, 8, 8)


def coefficients(y, cb, cr, src, sub, luma_q, chroma_q, matrix=mx.JFIF, bit_depth=8, shift=0, rng=lv.FULL):
    """(nblocks, 64) int16 zigzag blocks in MCU emission order, as ycc_ref.coefficients"""
    rx, ry = ratios(src, sub)
    yp, cbp, crp = padded_planes(y, cb, cr, src, sub, matrix, bit_depth, shift, rng)
    yb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(yp)), luma_q).reshape(-1, 64)
    cbb = np_ref.quantize(np_ref.dct_blocks(averaged_blocks(cbp, rx, ry)), chroma_q).reshape(-1, 64)
    crb = np_ref.quantize(np_ref.dct_blocks(averaged_blocks(crp, rx, ry)), chroma_q).reshape(-1, 64)
    return np_ref.interleave(yb, cbb, crb, sub, yp.shape[1] // 8)[:, np_ref.ZIGZAG]


def encode(y, cb, cr, src, sub, luma_q, chroma_q, matrix=mx.JFIF, bit_depth=8, shift=0, rng=lv.FULL,
           restart_interval=0) -> bytes:
    """the JPEG file dmmt_encode_device_ycc_subsample must write for planes at `src` and
    a file at `sub`"""
    h, w = y.shape
    return oracle.encode_coefficients(coefficients(y, cb, cr, src, sub, luma_q, chroma_q, matrix, bit_depth, shift, rng),
                                      w, h, sub, luma_q, chroma_q, restart_interval=restart_interval)
