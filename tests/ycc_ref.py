"""The CPU yardstick of the YCbCr input path (dmmt_encode_device_ycc) -- TEST
INFRASTRUCTURE, composed from what oracle/ exports.

The reference has no YCbCr input, so the contract is stated in its own stages
(include/dmmt_jpeg.h, "YCbCr device frames"): uint8 full-range samples, s - 128
into the DCT, the chroma planes as given (ceil(W/hr) x ceil(H/vr)), black padding
(luma sample 0, chroma sample 128), then np_ref's block resort, Arai DCT, quantiser
and MCU order and the oracle's back half.  tests/test_ycc_reference.py pins this
helper (a decoder, an IDCT, Pillow, committed goldens); the GPU tests compare
against it byte for byte."""
from __future__ import annotations

import numpy as np

import oracle
from oracle import np_ref

PLANAR, NV, NV_VU = 0, 1, 2
FORMATS = (PLANAR, NV, NV_VU)
f32 = np.float32


def rates(sub):
    return (1 if sub == 0 else 2), (2 if sub == 2 else 1)


def chroma_shape(w, h, sub):
    """(rows, columns) of a chroma plane of a w x h frame"""
    hr, vr = rates(sub)
    return -(-h // vr), -(-w // hr)


def random_planes(w, h, sub, seed):
    """seeded random uint8 planes (y, cb, cr) of a w x h frame"""
    rng = np.random.default_rng(seed)
    ch, cw = chroma_shape(w, h, sub)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (ch, cw), dtype=np.uint8))


def padded_planes(y, cb, cr, sub):
    """the float32 planes the DCT sees: level-shifted, padded black to the MCU grid"""
    h, w = y.shape
    hr, vr = rates(sub)
    assert cb.shape == cr.shape == chroma_shape(w, h, sub), (cb.shape, cr.shape, (w, h, sub))
    wp = -(-w // (8 * hr)) * 8 * hr
    hp = -(-h // (8 * vr)) * 8 * vr
    yp = np.full((hp, wp), f32(-128.0), np.float32)
    yp[:h, :w] = y.astype(np.float32) - f32(128.0)
    out = [yp]
    for c in (cb, cr):
        cp = np.zeros((hp // vr, wp // hr), np.float32)
        cp[:c.shape[0], :c.shape[1]] = c.astype(np.float32) - f32(128.0)
        out.append(cp)
    return out


def forward_dct(y, cb, cr, sub):
    """the float32 coefficients before quantisation: the (n, 8, 8) blocks of the Y, Cb
    and Cr planes in block raster order, and the padded luma width"""
    yp, cbp, crp = padded_planes(y, cb, cr, sub)
    return (np_ref.dct_blocks(np_ref.to_blocks(yp)), np_ref.dct_blocks(np_ref.to_blocks(cbp)),
            np_ref.dct_blocks(np_ref.to_blocks(crp)), yp.shape[1])


def coefficients(y, cb, cr, sub, luma_q, chroma_q):
    """(nblocks, 64) int16 zigzag blocks in MCU emission order, interleaved as np_ref.forward does"""
    yc, cbc, crc, wp = forward_dct(y, cb, cr, sub)
    yb = np_ref.quantize(yc, luma_q).reshape(-1, 64)
    cbb = np_ref.quantize(cbc, chroma_q).reshape(-1, 64)
    crb = np_ref.quantize(crc, chroma_q).reshape(-1, 64)
    return np_ref.interleave(yb, cbb, crb, sub, wp // 8)[:, np_ref.ZIGZAG]


def encode(y, cb, cr, sub, luma_q, chroma_q, restart_interval=0) -> bytes:
    """the JPEG file dmmt_encode_device_ycc must write for these planes"""
    h, w = y.shape
    return oracle.encode_coefficients(coefficients(y, cb, cr, sub, luma_q, chroma_q), w, h, sub, luma_q, chroma_q,
                                      restart_interval=restart_interval)


def chroma_rows(cb, cr, fmt):
    """the chroma planes as the format stores them: a list of (rows, row bytes) uint8 arrays"""
    if fmt == PLANAR:
        return [np.ascontiguousarray(cb), np.ascontiguousarray(cr)]
    pair = (cb, cr) if fmt == NV else (cr, cb)
    return [np.ascontiguousarray(np.stack(pair, axis=2)).reshape(cb.shape[0], -1)]


def pack_plane(frames, pitch, lead=0, tail=0, fill=None, frame_stride=0):
    """one plane of `frames` (a list of (rows, row bytes) uint8 arrays, one per frame)
    laid into a uint8 buffer: `lead` bytes, then row r of frame f at
    lead + f * frame_stride + r * pitch; every other byte comes from `fill` (an array
    at least as long; zeros if None)"""
    nrows, rowb = frames[0].shape
    assert pitch >= rowb
    span = (nrows - 1) * pitch + rowb
    size = lead + (len(frames) - 1) * frame_stride + span + tail
    buf = np.zeros(size, np.uint8) if fill is None else np.array(fill[:size], dtype=np.uint8)
    assert buf.size == size
    for f, fr in enumerate(frames):
        for r in range(nrows):
            o = lead + f * frame_stride + r * pitch
            buf[o:o + rowb] = fr[r]
    return buf
