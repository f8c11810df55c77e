"""The CPU yardstick of the grayscale input path (dmmt_encode_device_gray) -- TEST
INFRASTRUCTURE, composed from what oracle/ exports.

The reference has no gray input, so the contract is stated in its own stages
(include/dmmt_jpeg.h, "grayscale frames"): one component, sampling 1x1, the blocks
in raster order.  AS_RGB: the sample v is the pixel (v, v, v) through the
reference's front half -- the luma blocks of its 4:4:4 coefficients with the luma
table given as the chroma table too; Y_FULL_RANGE: the luma blocks of the YCbCr
yardstick (s - 128).  The file is the colour header with every chroma part taken
out, and the scan the reference's coding of the single chain of blocks with tables
from the luma histograms only.  tests/test_gray_reference.py pins this helper (a
decoder, the colour oracle, Pillow, committed goldens); the GPU tests compare
against it byte for byte."""
from __future__ import annotations

import numpy as np

import oracle
import ycc_ref
from oracle.jpeg_scan import ZIGZAG

AS_RGB, Y_FULL_RANGE = 0, 1


def blocks(gray, maxval, luma_q, transfer=AS_RGB):
    """(nblocks, 64) int16 zigzag blocks of the (H, W) plane `gray`, raster order"""
    g = np.asarray(gray)
    assert g.ndim == 2
    q = list(luma_q)
    if transfer == Y_FULL_RANGE:
        assert g.dtype == np.uint8
        c = np.zeros(g.shape, np.uint8)
        return ycc_ref.coefficients(g, c, c, 0, q, q)[0::3]
    rep = np.repeat(g[:, :, None], 3, axis=2)
    if g.dtype == np.float32:
        return oracle.forward_dots(rep, oracle.P444, q, q)[0::3]
    return oracle.forward(rep, maxval, oracle.P444, q, q)[0::3]


def _tokens(blk):
    """categorize.rs:132-151: the AC part of a zigzag block as (symbol, value) pairs"""
    out, zeros = [], 0
    for v in blk[1:]:
        v = int(v)
        if v == 0:
            zeros += 1
            continue
        while zeros > 15:
            out.append((0xF0, 0))
            zeros -= 16
        out.append(((zeros << 4) | oracle.category(v), v))
        zeros = 0
    if zeros:
        out.append((0x00, 0))
    return out


def encode_blocks(zz, width, height, luma_q, restart_interval=0, bits_per_channel=8) -> bytes:
    """raster-order zigzag blocks -> the single-component file"""
    ri = int(restart_interval)
    hist = [[0] * 256, [0] * 256]  # luma DC, luma AC
    items, last = [], 0
    for e, blk in enumerate(zz):
        if ri and e % ri == 0:
            last = 0
        d = int(np.int16(int(blk[0]) - last))
        last = int(blk[0])
        toks = _tokens(blk)
        hist[0][oracle.category(d)] += 1
        for s, _ in toks:
            hist[1][s] += 1
        items.append((d, toks))
    tabs = []
    for h in hist:
        syms, lens = oracle.code_lengths(h)
        tabs.append((syms, lens, oracle.assign_codes(syms, lens)))

    out = bytearray(b"\xff\xd8")

    def seg(m, content):
        out.extend(bytes([0xFF, m]) + (len(content) + 2).to_bytes(2, "big") + bytes(content))

    seg(0xE0, b"JFIF\x00\x01\x02\x00\x00\x48\x00\x48\x00\x00")
    seg(0xDB, bytes([0] + [luma_q[z] for z in ZIGZAG]))
    seg(0xC0, bytes([bits_per_channel]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([1, 1, 0x11, 0]))
    for kind, t in ((0x11, 1), (0x00, 0)):
        syms, lens, _ = tabs[t]
        bitsc = [0] * 16
        for ln in lens:
            bitsc[ln - 1] += 1
        seg(0xC4, bytes([kind] + bitsc + syms[::-1]))  # most frequent first (encoder.rs:169-181)
    if ri:
        seg(0xDD, ri.to_bytes(2, "big"))
    seg(0xDA, bytes([1, 1, 0x01, 0, 0x3F, 0]))

    acc, nacc = 0, 0

    def put(v, n):
        nonlocal acc, nacc
        acc = (acc << n) | (v & ((1 << n) - 1))
        nacc += n
        while nacc >= 8:
            b = (acc >> (nacc - 8)) & 0xFF
            out.append(b)
            if b == 0xFF:
                out.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1

    def flush():  # 1-padding to a byte boundary, the pad byte stuffed like any other
        if nacc:
            put((1 << (8 - nacc)) - 1, 8 - nacc)

    def extra(v, c):  # category_pattern is left-aligned in 16 bits
        return oracle.category_pattern(v, c) >> (16 - c) if c else 0

    dc, ac = tabs[0][2], tabs[1][2]
    for e, (d, toks) in enumerate(items):
        if ri and e and e % ri == 0:
            flush()
            out.extend(bytes([0xFF, 0xD0 + ((e // ri - 1) & 7)]))
        c = oracle.category(d)
        put(*dc[c])
        put(extra(d, c), c)
        for s, v in toks:
            put(*ac[s])
            put(extra(v, s & 15), s & 15)
    flush()
    out.extend(b"\xff\xd9")
    return bytes(out)


def encode(gray, maxval, luma_q, transfer=AS_RGB, restart_interval=0, bits_per_channel=8) -> bytes:
    """the JPEG file dmmt_encode_device_gray must write for this plane"""
    h, w = np.asarray(gray).shape
    return encode_blocks(blocks(gray, maxval, luma_q, transfer), w, h, list(luma_q), restart_interval, bits_per_channel)


def pack_plane(frames, pitch, lead=0, tail=0, fill=None, frame_stride=0):
    """ycc_ref.pack_plane over the frames' bytes (any sample type): pitch, lead and
    frame_stride in bytes"""
    rows = [np.ascontiguousarray(f).view(np.uint8).reshape(f.shape[0], -1) for f in frames]
    return ycc_ref.pack_plane(rows, pitch, lead, tail, fill, frame_stride)
