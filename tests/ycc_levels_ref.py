"""The CPU yardstick of the YCbCr sample levels (dmmt_encode_device_ycc_levels) --
TEST INFRASTRUCTURE, composed from tests/ycc_ref.py and what oracle/ exports.

The contract (include/dmmt_jpeg.h, "YCbCr sample levels"): a uint8 or uint16 sample
s carries the code v = s >> shift of B bits; with m = 2^(B-8), in IEEE f32, every
operation rounded once,

    FULL:     offY = 0,     kY = 255 / (2^B - 1),  offC = 2^(B-1),  kC = kY
    LIMITED:  offY = 16 m,  kY = 255 / (219 m),    offC = 128 m,    kC = 255 / (224 m)

    luma    min(max((f32(v) - offY) * kY, 0), 255) - 128
    chroma  min(max((f32(v) - offC) * kC, -128), 127)

enter the DCT; the padding is black after the transfer (luma -128, chroma 0).  From
there on ycc_ref's stages: np_ref's block resort, Arai DCT, quantiser and MCU order
and the oracle's back half.  tests/test_ycc_levels_reference.py pins this helper; the
GPU tests compare against it byte for byte."""
from __future__ import annotations

import numpy as np

import oracle
import ycc_ref
from oracle import np_ref

FULL, LIMITED = 0, 1
f32 = np.float32


def constants(bit_depth, rng):
    """(offY, kY, offC, kC) as float32, computed with float32 arithmetic"""
    B = int(bit_depth)
    assert 8 <= B <= 16 and rng in (FULL, LIMITED)
    m = f32(1 << (B - 8))
    if rng == LIMITED:
        return f32(16) * m, f32(255) / (f32(219) * m), f32(128) * m, f32(255) / (f32(224) * m)
    k = f32(255) / f32((1 << B) - 1)
    return f32(0), k, f32(1 << (B - 1)), k


def codes(s, shift):
    """the codes of samples: the low `shift` bits do not count"""
    return np.asarray(s).astype(np.uint32) >> np.uint32(shift)


def luma_in(v, bit_depth, rng):
    """float32 DCT inputs of luma codes v"""
    off, k, _, _ = constants(bit_depth, rng)
    t = (np.asarray(v).astype(np.float32) - off) * k
    assert t.dtype == np.float32
    return np.minimum(np.maximum(t, f32(0)), f32(255)) - f32(128)


def chroma_in(v, bit_depth, rng):
    """float32 DCT inputs of chroma codes v"""
    _, _, off, k = constants(bit_depth, rng)
    t = (np.asarray(v).astype(np.float32) - off) * k
    assert t.dtype == np.float32
    return np.minimum(np.maximum(t, f32(-128)), f32(127))


def exact(v, bit_depth, rng, chroma):
    """the same transfer in float64 from the exact constants (before the clamps' f32)"""
    B = int(bit_depth)
    m = float(1 << (B - 8))
    v = np.asarray(v).astype(np.float64)
    if rng == LIMITED:
        t = (v - 128 * m) * (255.0 / (224 * m)) if chroma else (v - 16 * m) * (255.0 / (219 * m))
    else:
        t = (v - float(1 << (B - 1))) * (255.0 / ((1 << B) - 1)) if chroma else v * (255.0 / ((1 << B) - 1))
    return np.clip(t, -128, 127) if chroma else np.clip(t, 0, 255) - 128


def exceeds_max(planes, bit_depth, shift):
    """a code above 2^B - 1 somewhere: DMMT_E_VALUE_EXCEEDS_MAX instead of a file"""
    return any(int(codes(p, shift).max()) > (1 << bit_depth) - 1 for p in planes)


def padded_planes(y, cb, cr, sub, bit_depth=8, shift=0, rng=FULL):
    """the float32 planes the DCT sees: transferred, padded black to the MCU grid"""
    h, w = y.shape
    hr, vr = ycc_ref.rates(sub)
    assert cb.shape == cr.shape == ycc_ref.chroma_shape(w, h, sub), (cb.shape, cr.shape, (w, h, sub))
    assert not exceeds_max((y, cb, cr), bit_depth, shift)
    wp = -(-w // (8 * hr)) * 8 * hr
    hp = -(-h // (8 * vr)) * 8 * vr
    yp = np.full((hp, wp), f32(-128.0), np.float32)
    yp[:h, :w] = luma_in(codes(y, shift), bit_depth, rng)
    out = [yp]
    for c in (cb, cr):
        cp = np.zeros((hp // vr, wp // hr), np.float32)
        cp[:c.shape[0], :c.shape[1]] = chroma_in(codes(c, shift), bit_depth, rng)
        out.append(cp)
    return out


def coefficients(y, cb, cr, sub, luma_q, chroma_q, bit_depth=8, shift=0, rng=FULL):
    """(nblocks, 64) int16 zigzag blocks in MCU emission order, as ycc_ref.coefficients"""
    yp, cbp, crp = padded_planes(y, cb, cr, sub, bit_depth, shift, rng)
    yb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(yp)), luma_q).reshape(-1, 64)
    cbb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(cbp)), chroma_q).reshape(-1, 64)
    crb = np_ref.quantize(np_ref.dct_blocks(np_ref.to_blocks(crp)), chroma_q).reshape(-1, 64)
    return np_ref.interleave(yb, cbb, crb, sub, yp.shape[1] // 8)[:, np_ref.ZIGZAG]


def encode(y, cb, cr, sub, luma_q, chroma_q, bit_depth=8, shift=0, rng=FULL, restart_interval=0) -> bytes:
    """the JPEG file dmmt_encode_device_ycc_levels must write for these planes"""
    h, w = y.shape
    return oracle.encode_coefficients(coefficients(y, cb, cr, sub, luma_q, chroma_q, bit_depth, shift, rng), w, h,
                                      sub, luma_q, chroma_q, restart_interval=restart_interval)


def random_planes(w, h, sub, seed, bit_depth=8, shift=0, sample_bytes=None, low_bits=False, lo=None, hi=None):
    """seeded random planes (y, cb, cr) whose codes are uniform in [lo, hi] (default: every
    code of bit_depth bits), as uint8 or uint16 samples = code << shift; low_bits: the
    unused low bits random as well instead of 0"""
    sb = sample_bytes if sample_bytes is not None else (1 if bit_depth == 8 and shift == 0 else 2)
    dt = np.uint8 if sb == 1 else np.uint16
    r = np.random.default_rng(seed)
    ch, cw = ycc_ref.chroma_shape(w, h, sub)
    lo = 0 if lo is None else lo
    hi = (1 << bit_depth) - 1 if hi is None else hi
    out = []
    for shape in ((h, w), (ch, cw), (ch, cw)):
        s = r.integers(lo, hi + 1, shape, dtype=np.uint32) << np.uint32(shift)
        if low_bits and shift:
            s |= r.integers(0, 1 << shift, shape, dtype=np.uint32)
        out.append(s.astype(dt))
    return tuple(out)


def chroma_rows(cb, cr, fmt):
    """the chroma planes as the format stores them: a list of (rows, row BYTES) uint8
    arrays (uint16 samples in host byte order), for ycc_ref.pack_plane"""
    if fmt == ycc_ref.PLANAR:
        planes = [np.ascontiguousarray(cb), np.ascontiguousarray(cr)]
    else:
        pair = (cb, cr) if fmt == ycc_ref.NV else (cr, cb)
        planes = [np.ascontiguousarray(np.stack(pair, axis=2)).reshape(cb.shape[0], -1)]
    return [as_bytes(p) for p in planes]


def as_bytes(plane):
    """a (rows, samples) plane as its (rows, row bytes) uint8 view"""
    p = np.ascontiguousarray(plane)
    return p.view(np.uint8).reshape(p.shape[0], -1)
