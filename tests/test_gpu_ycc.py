"""YCbCr device frames (dmmt_encode_device_ycc): planar and NV planes encoded where
they lie, without an RGB round trip.  The expected bytes are always those of the
CPU yardstick tests/ycc_ref.py (pinned by tests/test_ycc_reference.py).  Every
plane is embedded in a larger device buffer whose other bytes -- the lead, the row
padding, the parent frame around a region of interest, the gap between frames --
are seeded random bytes that include 0xFF: none of them may reach the output."""
import ctypes
import os

import numpy as np
import pytest

import dmmt_jpeg
import ycc_ref
from dmmt_jpeg import YccFormat as YF

pytestmark = pytest.mark.gpu

FORMATS = [YF.PLANAR, YF.NV, YF.NV_VU]
SUBS = [0, 1, 2]
# both sides of the 256-column luma tile and of the 128- / 256-byte chroma tile row, odd W and H
# under 4:2:0, one and several MCU rows
SIZES = [(1, 1), (7, 17), (255, 9), (256, 1), (257, 33), (513, 17)]
ONES, ALL255 = [1] * 64, [255] * 64

_noise = None


def noise(n, seed):
    """n seeded random bytes, 0xFF among them"""
    global _noise
    if _noise is None:
        _noise = np.random.default_rng(77).integers(0, 256, 4 << 20, dtype=np.uint8)
        _noise[::7] = 0xFF
    off = (seed * 4099) % 4096
    assert off + n <= _noise.size
    return _noise[off:off + n].copy()


def opts(sub, tables, ri=0):
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=tables[0],
                                              chroma_table=tables[1], restart_interval=ri)


_ref = {}


def expected(planes, sub, tables, ri=0):
    key = (tuple(p.tobytes() for p in planes), planes[0].shape, sub, ri, tuple(tables[0]), tuple(tables[1]))
    if key not in _ref:
        _ref[key] = ycc_ref.encode(*planes, sub, tables[0], tables[1], restart_interval=ri)
    return _ref[key]


def row_bytes(w, sub, fmt):
    """(luma, chroma) bytes of a row"""
    cw = ycc_ref.chroma_shape(w, 1, sub)[1]
    return w, cw * (1 if fmt == YF.PLANAR else 2)


class Frames:
    """frames [(y, cb, cr), ...] embedded in noise: one device buffer per plane, the
    plane `lead` bytes into it, rows a pitch apart, frames `fstride` bytes apart"""

    def __init__(self, enc, frames, fmt, lpitch, cpitch, fstride=0, leads=(0, 0, 0), seed=1, tail=0):
        self.enc, self.fmt = enc, fmt
        per_plane = [[f[0] for f in frames]]
        chroma = [ycc_ref.chroma_rows(f[1], f[2], int(fmt)) for f in frames]
        for p in range(len(chroma[0])):
            per_plane.append([c[p] for c in chroma])
        self.bufs, self.ptrs = [], []
        for p, rows in enumerate(per_plane):
            pitch = lpitch if p == 0 else cpitch
            nrows, rowb = rows[0].shape
            size = leads[p] + (len(frames) - 1) * fstride + (nrows - 1) * pitch + rowb + tail
            host = ycc_ref.pack_plane(rows, pitch, leads[p], tail, noise(size, seed + 11 * p), fstride)
            d = enc.malloc(size)
            enc.h2d(d, host)
            self.bufs.append(d)
            self.ptrs.append(d + leads[p])

    def planes(self, offsets=(0, 0, 0)):
        return [p + o for p, o in zip(self.ptrs, offsets)]

    def free(self):
        for d in self.bufs:
            self.enc.free(d)


def enqueue(enc, planes, fmt, lpitch, cpitch, n, w, h, options, fstride=0, stream=None):
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, int(options.chroma_subsampling_preset))
    d_out, d_len = enc.malloc(n * cap), enc.malloc(4 * n)
    enc.encode_device_ycc(planes, fmt, lpitch, cpitch, n, w, h, options, d_out, cap, d_len, frame_stride=fstride,
                          stream=stream)
    return d_out, d_len, cap, n


def collect(enc, job):
    d_out, d_len, cap, n = job
    lens = np.frombuffer(enc.d2h(d_len, 4 * n), np.uint32)
    out = [enc.d2h(d_out + f * cap, min(int(lens[f]), cap)) for f in range(n)]
    enc.free(d_out)
    enc.free(d_len)
    return out


def encode(enc, planes, fmt, lpitch, cpitch, n, w, h, options, fstride=0):
    job = enqueue(enc, planes, fmt, lpitch, cpitch, n, w, h, options, fstride)
    try:
        enc.synchronize()
    finally:
        out = collect(enc, job)
    return out


def encode_frames(enc, frames, fmt, sub, tables, lextra=0, cextra=0, leads=(0, 0, 0), seed=1, ri=0):
    """one call for frames tightly strided by their pitches; returns the files"""
    h, w = frames[0][0].shape
    lrow, crow = row_bytes(w, sub, fmt)
    s = Frames(enc, frames, fmt, lrow + lextra, crow + cextra, leads=leads, seed=seed)
    try:
        return encode(enc, s.planes(), fmt, lrow + lextra, crow + cextra, 1, w, h, opts(sub, tables, ri))
    finally:
        s.free()


@pytest.fixture(scope="module")
def tables():
    return dmmt_jpeg.quality_tables(90)


# ------------------------------------------------------------------ the matrix

@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_every_format_at_every_pitch(encoder, tables, fmt, sub):
    for i, (w, h) in enumerate(SIZES):
        planes = ycc_ref.random_planes(w, h, sub, 100 * sub + i)
        want = expected(planes, sub, tables)
        # tight, then luma and chroma pitches that differ (+1: every row another misalignment)
        for k, (le, ce) in enumerate(((0, 0), (1, 16), (16, 1))):
            leads = ((3 * i + k) % 15 + 1, (7 * i + 5 * k) % 15 + 1, (11 * i + 3 * k + 8) % 15 + 1)  # 1..15, differing
            got = encode_frames(encoder, [planes], fmt, sub, tables, le, ce, leads, seed=i + 7 * k)
            assert got == [want], (w, h, le, ce, leads)


@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_aligned_planes_and_interior_tiles(encoder, tables, fmt):
    """769 x 49: middle tiles take the loader's interior path; leads 0 and 16"""
    w, h = 769, 49
    for sub in SUBS:
        planes = ycc_ref.random_planes(w, h, sub, 900 + sub)
        for leads in ((0, 0, 0), (16, 0, 16)):
            got = encode_frames(encoder, [planes], fmt, sub, tables, 0, 0, leads, seed=sub)
            assert got == [expected(planes, sub, tables)], (sub, leads)


@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_three_frames(encoder, tables, fmt):
    w, h, sub = 257, 17, 2
    frames = [ycc_ref.random_planes(w, h, sub, 21 + f) for f in range(3)]
    lrow, crow = row_bytes(w, sub, fmt)
    lp, cp = lrow + 1, crow + 3
    fstride = h * lp + 5  # (covers the smaller chroma planes too) not a multiple of 16
    assert fstride % 16
    s = Frames(encoder, frames, fmt, lp, cp, fstride=fstride, leads=(2, 9, 13), seed=8)
    try:
        got = encode(encoder, s.planes(), fmt, lp, cp, 3, w, h, opts(sub, tables), fstride=fstride)
    finally:
        s.free()
    assert got == [expected(f, sub, tables) for f in frames]


def test_region_of_interest_in_an_nv12_frame(encoder, tables):
    """257 x 33 windows of a 300 x 40 NV12 parent: the window's pointers (an origin
    on the chroma grid), the parent's pitches.  (0, 0) starts at the planes' first
    bytes, (42, 6) ends in the parent's last rows."""
    pw, ph, w, h, sub = 300, 40, 257, 33, 2
    py, pcb, pcr = ycc_ref.random_planes(pw, ph, sub, 40)
    lp, cp = pw + 4, 2 * 150 + 6
    s = Frames(encoder, [(py, pcb, pcr)], YF.NV, lp, cp, leads=(0, 3, 0), seed=5)
    ch, cw = ycc_ref.chroma_shape(w, h, sub)
    try:
        for x, y in [(0, 0), (2, 0), (16, 2), (10, 4), (42, 6)]:
            win = (np.ascontiguousarray(py[y:y + h, x:x + w]), np.ascontiguousarray(pcb[y // 2:y // 2 + ch, x // 2:x // 2 + cw]),
                   np.ascontiguousarray(pcr[y // 2:y // 2 + ch, x // 2:x // 2 + cw]))
            got = encode(encoder, s.planes((y * lp + x, (y // 2) * cp + (x // 2) * 2, 0)), YF.NV, lp, cp, 1, w, h,
                         opts(sub, tables))
            assert got == [expected(win, sub, tables)], (x, y)
    finally:
        s.free()


# ------------------------------------------------------------------ tables, constant planes, restart

@pytest.mark.parametrize("name", ["spec", "ones", "all255"])
def test_tables(encoder, spec_tables, name):
    t = {"spec": spec_tables, "ones": (ONES, ONES), "all255": (ALL255, ALL255)}[name]
    w, h = 257, 33
    for fmt, sub in ((YF.PLANAR, 0), (YF.NV, 2), (YF.NV_VU, 1)):
        planes = ycc_ref.random_planes(w, h, sub, 600 + sub)
        assert encode_frames(encoder, [planes], fmt, sub, t, 1, 1, (1, 2, 3)) == [expected(planes, sub, t)], (fmt, sub)


@pytest.mark.parametrize("value", [0, 255, 128])
def test_constant_planes(encoder, tables, value):
    """all 0, all 255, and constant 128 (level-shifted 0: EOB-only blocks inside the image)"""
    w, h = 257, 33
    for fmt, sub in ((YF.PLANAR, 2), (YF.NV, 0), (YF.NV_VU, 2), (YF.PLANAR, 1)):
        ch, cw = ycc_ref.chroma_shape(w, h, sub)
        planes = (np.full((h, w), value, np.uint8), np.full((ch, cw), value, np.uint8),
                  np.full((ch, cw), value, np.uint8))
        for t in (tables, (ONES, ONES)):
            assert encode_frames(encoder, [planes], fmt, sub, t, 16, 1, (5, 6, 7)) == [expected(planes, sub, t)], (fmt, sub)


def test_restart_interval(encoder, tables):
    w, h = 257, 33
    for fmt, sub in ((YF.NV, 2), (YF.PLANAR, 1), (YF.NV_VU, 0)):
        planes = ycc_ref.random_planes(w, h, sub, 77)
        got = encode_frames(encoder, [planes], fmt, sub, tables, 1, 0, (1, 1, 2), ri=7)
        assert got == [expected(planes, sub, tables, ri=7)]


# ------------------------------------------------------------------ graph cache, lanes, streams

def test_graph_cache_tells_chroma_planes_and_formats_apart(tables):
    """A context that replays captured graphs (DMMT_GRAPHS=1), one luma pointer, one
    output buffer: planar with (Cb, Cr), planar with the two chroma pointers
    swapped, the pairs as NV, the same pairs as NV_VU, NV at another chroma pitch --
    then each again, a replay.  A key without the chroma pointers, the pitches or the
    format replays another call's graph and its bytes."""
    os.environ["DMMT_GRAPHS"] = "1"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_GRAPHS")
    w, h, sub = 256, 16, 0
    y, cb, cr = ycc_ref.random_planes(w, h, sub, 12)
    pairs = noise(h * (2 * w + 2), 3)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
    ptrs = [enc.malloc(n) for n in (y.size, cb.size, cr.size, pairs.size, cap, 4)]
    d_y, d_cb, d_cr, d_pairs, d_out, d_len = ptrs
    o = opts(sub, tables)

    def nv(pitch, first):  # the component at byte `first` of each pair, rows `pitch` apart
        return np.ascontiguousarray(np.lib.stride_tricks.as_strided(pairs[first:], (h, w), (pitch, 2)))

    calls = [([d_y, d_cb, d_cr], YF.PLANAR, w, (y, cb, cr)), ([d_y, d_cr, d_cb], YF.PLANAR, w, (y, cr, cb)),
             ([d_y, d_pairs, 0], YF.NV, 2 * w, (y, nv(2 * w, 0), nv(2 * w, 1))),
             ([d_y, d_pairs, 0], YF.NV_VU, 2 * w, (y, nv(2 * w, 1), nv(2 * w, 0))),
             ([d_y, d_pairs, 0], YF.NV, 2 * w + 2, (y, nv(2 * w + 2, 0), nv(2 * w + 2, 1)))]
    want = [expected(p, sub, tables) for _, _, _, p in calls]
    assert len(set(want)) == len(want)  # the reference's outputs differ
    try:
        for d, a in zip(ptrs, (y, cb, cr, pairs)):
            enc.h2d(d, a)
        for rep in range(2):  # the second round replays every graph
            for (planes, fmt, cpitch, _), ref in zip(calls, want):
                enc.encode_device_ycc(planes, fmt, w, cpitch, 1, w, h, o, d_out, cap, d_len)
                enc.synchronize()
                n = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
                assert enc.d2h(d_out, min(n, cap)) == ref, (rep, fmt, cpitch)
    finally:
        for ptr in ptrs:
            enc.free(ptr)
        enc.close()


def test_two_lanes(encoder, tables):
    w, h, sub = 257, 33, 2
    o = opts(sub, tables)
    jobs, surfs, want = [], [], []
    try:
        encoder.set_lanes(2)
        for i, fmt in enumerate([YF.NV, YF.PLANAR, YF.NV_VU, YF.NV, YF.PLANAR]):
            planes = ycc_ref.random_planes(w, h, sub, 300 + i)
            lrow, crow = row_bytes(w, sub, fmt)
            s = Frames(encoder, [planes], fmt, lrow + 1, crow + 16, leads=(1 + i, 2 + i, 3 + i), seed=i)
            surfs.append(s)
            jobs.append(enqueue(encoder, s.planes(), fmt, lrow + 1, crow + 16, 1, w, h, o))  # NULL stream: round-robin
            want.append(expected(planes, sub, tables))
        encoder.synchronize()
        got = [collect(encoder, j)[0] for j in jobs]
        assert got == want
    finally:
        for s in surfs:
            s.free()
        encoder.set_lanes(1)  # the shared encoder's lane count, restored


def test_caller_stream(encoder, tables):
    import torch
    w, h, sub = 257, 33, 2
    planes = ycc_ref.random_planes(w, h, sub, 400)
    lrow, crow = row_bytes(w, sub, YF.NV)
    st = torch.cuda.Stream(torch.device("cuda", 0))
    s = Frames(encoder, [planes], YF.NV, lrow, crow, leads=(4, 8, 0), seed=9)
    try:
        job = enqueue(encoder, s.planes(), YF.NV, lrow, crow, 1, w, h, opts(sub, tables), stream=st.cuda_stream)
        encoder.synchronize()
        assert collect(encoder, job) == [expected(planes, sub, tables)]
    finally:
        s.free()


def test_encode_ycc_from_host_planes(encoder, tables):
    w, h = 257, 33
    for sub in SUBS:
        y, cb, cr = ycc_ref.random_planes(w, h, sub, 500 + sub)
        want = expected((y, cb, cr), sub, tables)
        o = opts(sub, tables)
        assert encoder.encode_ycc(y, cb=cb, cr=cr, options=o) == want
        assert encoder.encode_ycc(y, uv=np.stack([cb, cr], axis=2), options=o) == want
        assert encoder.encode_ycc(y, vu=np.stack([cr, cb], axis=2), options=o) == want
    with pytest.raises(ValueError):  # 4:2:0 chroma for a 4:4:4 encode
        encoder.encode_ycc(y, cb=cb, cr=cr, options=opts(0, tables))
    with pytest.raises(ValueError):
        encoder.encode_ycc(y, cb=cb, options=o)
    with pytest.raises(ValueError):
        encoder.encode_ycc(y.astype(np.uint16), cb=cb, cr=cr, options=o)


# ------------------------------------------------------------------ arguments

def test_invalid_arguments(encoder, tables):
    L = dmmt_jpeg.lib()
    w, h = 64, 16
    d = encoder.malloc(1 << 16)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, 0)
    d_out, d_len = encoder.malloc(cap), encoder.malloc(4)
    P3 = [d, d + 4096, d + 8192]

    def rc(planes, fmt, lp, cp, sub=0, sampling=None, out_stride=cap, n=1, width=w, height=h, out=d_out, ln=d_len):
        y = dmmt_jpeg.Encoder.ycc(planes, fmt, lp, cp, n, width, height, sub if sampling is None else sampling, out,
                                  out_stride, ln)
        o = opts(sub, tables).to_c()
        return L.dmmt_encode_device_ycc(encoder.handle, ctypes.byref(y), ctypes.byref(o), None)
    try:
        assert rc(P3, YF.PLANAR, w, w) == 0 and rc(P3, YF.NV, w, 2 * w) == 0 and rc([d, d + 4096, 0], YF.NV_VU, w, 2 * w) == 0
        assert L.dmmt_encode_device_ycc(encoder.handle, None, ctypes.byref(opts(0, tables).to_c()), None) == -102
        assert rc([0, d, d], YF.PLANAR, w, w) == -102                      # a needed plane is NULL
        assert rc([d, 0, d], YF.PLANAR, w, w) == -102 and rc([d, d, 0], YF.PLANAR, w, w) == -102
        assert rc([d, 0, d], YF.NV, w, 2 * w) == -102
        assert rc(P3, YF.PLANAR, w, w, n=0) == -102 and rc(P3, YF.PLANAR, w, w, n=-1) == -102
        assert rc(P3, 3, w, 2 * w) == -102 and rc(P3, -1, w, 2 * w) == -102  # format out of range
        assert rc(P3, YF.PLANAR, w, w, sub=0, sampling=2) == -102            # chroma_sampling != opt->subsampling
        assert rc(P3, YF.PLANAR, w, w // 2, sub=2, sampling=1) == -102
        assert rc(P3, YF.PLANAR, w - 1, w) == -102                           # a pitch below the row's bytes
        assert rc(P3, YF.PLANAR, w, w - 1) == -102 and rc(P3, YF.NV, w, 2 * w - 1) == -102
        assert rc(P3, YF.PLANAR, w, w // 2 - 1, sub=2) == -102 and rc(P3, YF.NV, w, w - 1, sub=1) == -102
        assert rc(P3, YF.PLANAR, w, w // 2, sub=2, out_stride=dmmt_jpeg.max_jpeg_bytes(w, h, 2)) == 0
        assert rc(P3, YF.PLANAR, (1 << 30) + 1, w) == -102                   # above DMMT_MAX_ROW_PITCH
        assert rc(P3, YF.PLANAR, w, (1 << 30) + 1) == -102
        assert rc(P3, YF.PLANAR, w, w, width=0) == -102 and rc(P3, YF.PLANAR, w, w, height=0) == -102
        assert rc(P3, YF.PLANAR, 65535, 65535, width=65535, sub=2, out_stride=1 << 40) == -102  # padded size beyond u16
        assert rc(P3, YF.PLANAR, w, w, out=0) == -102 and rc(P3, YF.PLANAR, w, w, ln=0) == -102
        assert rc(P3, YF.PLANAR, w, w, out_stride=cap - 1) == -203           # DMMT_E_CAPACITY
        encoder.synchronize()
    finally:
        for p in (d, d_out, d_len):
            encoder.free(p)
