"""Device surfaces (dmmt_encode_device_surfaces): pitched, B,G,R, 4-sample and
planar frames encoded where they lie.  The expected bytes are always the oracle's
encode of the same pixels packed as H x W x 3 R,G,B on the host (and the library's
own host encode of them).  Every surface is embedded in a larger device buffer
whose other bytes -- row padding, the X sample, the parent image around a region
of interest, the gap between frames -- are seeded random bytes that include 0xFF:
none of them may reach the output or the maxval check."""
import ctypes
import os

import numpy as np
import pytest

import dmmt_jpeg
import oracle
from dmmt_jpeg import PixelFormat as PF

pytestmark = pytest.mark.gpu

RGB, BGR, RGBX, BGRX, PLANAR = PF.RGB, PF.BGR, PF.RGBX, PF.BGRX, PF.PLANAR
# the supported matrix: (format, sample dtype)
MATRIX = [(RGB, "u8"), (RGB, "u16"), (RGB, "f32"), (BGR, "u8"), (BGR, "u16"), (BGR, "f32"), (RGBX, "u8"),
          (BGRX, "u8"), (PLANAR, "u8"), (PLANAR, "f32")]
MATRIX_IDS = [f"{f.name}-{d}" for f, d in MATRIX]
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
# 256-pixel tiles, 16-byte chunks, 8*VR-row tiles: every width and every height with every subsampling
SHAPES = [(1, 33), (7, 17), (255, 9), (256, 1), (257, 33), (513, 17), (7, 9), (1, 1)]
SUBS = [0, 1, 2]

_noise = None


def noise(n, seed):
    """n seeded random bytes, 0xFF among them"""
    global _noise
    if _noise is None:
        _noise = np.random.default_rng(99).integers(0, 256, 20 << 20, dtype=np.uint8)
        _noise[::7] = 0xFF
    off = (seed * 4099) % 4096
    assert off + n <= _noise.size
    return _noise[off:off + n].copy()


def opts(sub, tables, ri=0):
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=tables[0],
                                              chroma_table=tables[1], restart_interval=ri)


def pixels(w, h, kind, seed, n=None, maxval=None):
    """(integer pixels for the oracle, their maxval, the samples as the surface holds them)"""
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    if kind == "u16":
        mv = maxval or 1000
        raw = rng.integers(0, mv + 1, shape, dtype=np.uint16)
        return raw, mv, raw
    mv = maxval or 255
    raw = rng.integers(0, mv + 1, shape, dtype=np.uint8)
    if kind == "f32":
        return raw, mv, raw.astype(np.float32) / np.float32(mv)
    return raw, mv, raw


_ref = {}


def expected(raw, mv, sub, tables, ri=0):
    key = (raw.tobytes(), raw.shape, mv, sub, ri, tuple(tables[0]))
    if key not in _ref:
        _ref[key] = oracle.encode(raw, mv, sub, *tables, restart_interval=ri)
    return _ref[key]


def spp_of(fmt):
    return PF(fmt).samples_per_pixel()


def plane_rows(samples, fmt, seed):
    """the surface's planes as (H, W * samples_per_pixel) sample arrays"""
    h, w, _ = samples.shape
    if fmt == PLANAR:
        return [np.ascontiguousarray(samples[:, :, c]) for c in range(3)]
    s = samples[:, :, ::-1] if fmt in (BGR, BGRX) else samples
    if fmt in (RGBX, BGRX):
        x = noise(h * w, seed + 5).reshape(h, w, 1)
        s = np.concatenate([s, x.astype(samples.dtype)], axis=2)
    return [np.ascontiguousarray(s).reshape(h, -1)]


class Surface:
    """frames (n, H, W, 3) embedded in noise: per plane one device buffer, the plane
    `lead` bytes into it, rows `pitch` bytes apart, frames `fstride` bytes apart"""

    def __init__(self, enc, frames, fmt, pitch, fstride=0, leads=(0, 0, 0), seed=1, tail=0):
        self.enc, self.fmt = enc, fmt
        n, h, w, _ = frames.shape
        sb = frames.dtype.itemsize
        rowb = w * spp_of(fmt) * sb
        span = (h - 1) * pitch + rowb
        self.n, self.h, self.w, self.sb, self.pitch, self.fstride = n, h, w, sb, pitch, fstride
        self.bufs, self.ptrs, self.host = [], [], []
        per_frame = [plane_rows(frames[f], fmt, seed + f) for f in range(n)]
        for p in range(len(per_frame[0])):
            size = leads[p] + (n - 1) * fstride + span + tail
            host = noise(size, seed + 11 * p)
            for f in range(n):
                rows = per_frame[f][p].view(np.uint8).reshape(h, rowb)
                for y in range(h):
                    o = leads[p] + f * fstride + y * pitch
                    host[o:o + rowb] = rows[y]
            d = enc.malloc(size)
            enc.h2d(d, host)
            self.bufs.append(d)
            self.ptrs.append(d + leads[p])
            self.host.append(host)

    def planes(self, byte_offset=0):
        return [p + byte_offset for p in self.ptrs] if self.fmt == PLANAR else self.ptrs[0] + byte_offset

    def free(self):
        for d in self.bufs:
            self.enc.free(d)


def enqueue(enc, planes, fmt, pitch, n, w, h, options, mv, sb, fstride=0, stream=None):
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, int(options.chroma_subsampling_preset))
    d_out, d_len = enc.malloc(n * cap), enc.malloc(4 * n)
    enc.encode_device_surfaces(planes, fmt, pitch, n, w, h, options, d_out, cap, d_len, frame_stride=fstride,
                               maxval=mv, sample_bytes=sb, stream=stream)
    return d_out, d_len, cap, n


def collect(enc, job):
    d_out, d_len, cap, n = job
    lens = np.frombuffer(enc.d2h(d_len, 4 * n), np.uint32)
    out = [enc.d2h(d_out + f * cap, min(int(lens[f]), cap)) for f in range(n)]
    enc.free(d_out)
    enc.free(d_len)
    return out


def encode(enc, planes, fmt, pitch, n, w, h, options, mv, sb, fstride=0):
    job = enqueue(enc, planes, fmt, pitch, n, w, h, options, mv, sb, fstride)
    try:
        enc.synchronize()
    finally:
        out = collect(enc, job)
    return out


@pytest.fixture(scope="module")
def tables():
    return dmmt_jpeg.quality_tables(90)


# ------------------------------------------------------------------ the matrix

@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt,kind", MATRIX, ids=MATRIX_IDS)
def test_every_format_at_every_pitch(encoder, tables, fmt, kind, sub):
    o = opts(sub, tables)
    for i, (w, h) in enumerate(SHAPES):
        raw, mv, samples = pixels(w, h, kind, 100 * sub + i)
        want = expected(raw, mv, sub, tables)
        host = samples if kind == "f32" else raw
        assert encoder.encode(dmmt_jpeg.Image.from_array(host, mv), o) == want
        sb = samples.dtype.itemsize
        tight = w * spp_of(fmt) * sb
        for pitch in (tight, tight + sb, tight + 16):  # (+ sb: every row another misalignment)
            s = Surface(encoder, samples[None], fmt, pitch, seed=i + pitch)
            try:
                got = encode(encoder, s.planes(), fmt, pitch, 1, w, h, o, mv, sb)
            finally:
                s.free()
            assert got == [want], (w, h, pitch)


@pytest.mark.parametrize("fmt,kind", MATRIX, ids=MATRIX_IDS)
def test_large_pitch(encoder, tables, fmt, kind):
    """rows 1 MiB + 3 samples apart, 17 rows"""
    w, h, sub = 257, 17, 2
    raw, mv, samples = pixels(w, h, kind, 7)
    sb = samples.dtype.itemsize
    pitch = (1 << 20) + 3 * sb
    s = Surface(encoder, samples[None], fmt, pitch, seed=3)
    try:
        got = encode(encoder, s.planes(), fmt, pitch, 1, w, h, opts(sub, tables), mv, sb)
    finally:
        s.free()
    assert got == [expected(raw, mv, sub, tables)]


# ------------------------------------------------------------------ regions of interest

@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt,kind", MATRIX, ids=MATRIX_IDS)
def test_region_of_interest(encoder, tables, fmt, kind, sub):
    """257 x 33 windows of a 300 x 40 parent: the window's pointer, the parent's
    pitch.  (0, 0) starts at the parent's first byte, (43, 7) ends at its last;
    planar planes lie 0, 1 and 7 samples into their buffers."""
    pw, ph, w, h = 300, 40, 257, 33
    raw, mv, samples = pixels(pw, ph, kind, 40 + sub)
    sb = samples.dtype.itemsize
    bpp = spp_of(fmt) * sb
    pitch = pw * bpp
    s = Surface(encoder, samples[None], fmt, pitch, leads=(0, sb, 7 * sb), seed=sub)
    o = opts(sub, tables)
    try:
        for x, y in [(0, 0), (1, 0), (5, 0), (16, 0), (0, 3), (1, 3), (5, 3), (16, 3), (43, 7)]:
            win = np.ascontiguousarray(raw[y:y + h, x:x + w])
            got = encode(encoder, s.planes(y * pitch + x * bpp), fmt, pitch, 1, w, h, o, mv, sb)
            assert got == [expected(win, mv, sub, tables)], (x, y)
    finally:
        s.free()


# ------------------------------------------------------------------ several frames

@pytest.mark.parametrize("fmt,kind", MATRIX, ids=MATRIX_IDS)
def test_three_frames(encoder, tables, fmt, kind):
    w, h, sub = 257, 17, 1
    raw, mv, samples = pixels(w, h, kind, 21, n=3)
    sb = samples.dtype.itemsize
    pitch = w * spp_of(fmt) * sb + sb
    fstride = h * pitch + 5 * sb  # not a multiple of 16
    assert fstride % 16
    s = Surface(encoder, samples, fmt, pitch, fstride=fstride, seed=8)
    try:
        got = encode(encoder, s.planes(), fmt, pitch, 3, w, h, opts(sub, tables), mv, sb, fstride=fstride)
    finally:
        s.free()
    assert got == [expected(raw[f], mv, sub, tables) for f in range(3)]


# ------------------------------------------------------------------ the range check

@pytest.mark.parametrize("fmt,kind,maxval", [(RGBX, "u8", 100), (PLANAR, "u8", 100), (RGB, "u16", 1000),
                                             (BGR, "u8", 100)], ids=["RGBX", "PLANAR", "RGB-u16", "BGR"])
def test_range_check_sees_used_samples_only(encoder, tables, fmt, kind, maxval):
    """0xFF in the X sample, in the row padding and in the parent outside the window
    is no error; maxval + 1 in a used sample of the last pixel of the last row is"""
    pw, ph, w, h, x, y, sub = 300, 40, 257, 33, 5, 3, 2
    raw, mv, samples = pixels(pw, ph, kind, 60, maxval=maxval)
    hot = samples.copy()
    hot.reshape(-1)[::5] = maxval * 2 + 55  # the parent around the window: above maxval (255 for u8)
    hot[y:y + h, x:x + w] = samples[y:y + h, x:x + w]
    sb = samples.dtype.itemsize
    bpp = spp_of(fmt) * sb
    pitch = pw * bpp + 16
    o = opts(sub, tables)
    win = np.ascontiguousarray(raw[y:y + h, x:x + w])
    s = Surface(encoder, hot[None], fmt, pitch, leads=(0, 1, 7), seed=4)
    try:
        got = encode(encoder, s.planes(y * pitch + x * bpp), fmt, pitch, 1, w, h, o, mv, sb)
        assert got == [expected(win, mv, sub, tables)]
    finally:
        s.free()
    for ch in (0, 2):
        bad = hot.copy()
        bad[y + h - 1, x + w - 1, ch] = maxval + 1
        s = Surface(encoder, bad[None], fmt, pitch, leads=(0, 1, 7), seed=4)
        try:
            with pytest.raises(dmmt_jpeg.Error) as e:
                encode(encoder, s.planes(y * pitch + x * bpp), fmt, pitch, 1, w, h, o, mv, sb)
            assert e.value.code == -100
        finally:
            s.free()
    # the context stays usable
    assert encoder.encode(dmmt_jpeg.Image.from_array(win, mv), o) == expected(win, mv, sub, tables)


# ------------------------------------------------------------------ graph cache, lanes

def test_graph_cache_tells_layouts_apart(tables):
    """A context that replays captured graphs (DMMT_GRAPHS=1), one input buffer, one
    base pointer, one output buffer: RGB at pitch p, BGR at pitch p, RGB at pitch
    p + 3 (a narrower image, and the same width), planar with the same first plane
    and the other two swapped, then each again -- a replay.  Every call differs from
    another only in the format, the pitch or the second and third plane pointers:
    a key without them replays the other call's graph and its bytes."""
    os.environ["DMMT_GRAPHS"] = "1"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_GRAPHS")
    w, h, sub = 256, 17, 0
    buf = noise((h + 1) * (w * 3 + 3), 12)
    buf[buf > 250] = 250
    o = opts(sub, tables)
    p = w * 3
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
    d, d_out, d_len = enc.malloc(buf.size), enc.malloc(cap), enc.malloc(4)

    def view(width, pitch, bgr):
        a = np.lib.stride_tricks.as_strided(buf, (h, width, 3), (pitch, 3, 1))
        return np.ascontiguousarray(a[:, :, ::-1] if bgr else a)

    def planar(order):  # three w x h planes of the buffer, rows w bytes apart
        return np.stack([buf[k * w * h:(k + 1) * w * h].reshape(h, w) for k in order], axis=2)

    calls = [(d, RGB, p, w, view(w, p, False)), (d, BGR, p, w, view(w, p, True)),
             (d, RGB, p + 3, w - 1, view(w - 1, p + 3, False)), (d, RGB, p + 3, w, view(w, p + 3, False)),
             ([d, d + w * h, d + 2 * w * h], PLANAR, w, w, planar((0, 1, 2))),
             ([d, d + 2 * w * h, d + w * h], PLANAR, w, w, planar((0, 2, 1)))]
    try:
        enc.h2d(d, buf)
        for rep in range(2):  # the second round replays every graph
            for planes, fmt, pitch, width, packed in calls:
                enc.encode_device_surfaces(planes, fmt, pitch, 1, width, h, o, d_out, cap, d_len)
                enc.synchronize()
                n = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
                assert enc.d2h(d_out, min(n, cap)) == expected(packed, 255, sub, tables), (rep, fmt, pitch, width)
    finally:
        for ptr in (d, d_out, d_len):
            enc.free(ptr)
        enc.close()


def test_lanes_with_alternating_formats(tables):
    w, h, sub = 257, 33, 2
    o = opts(sub, tables)
    enc = dmmt_jpeg.Encoder(0)
    try:
        enc.set_lanes(4)
        jobs, surfs, want = [], [], []
        for i, (fmt, kind) in enumerate([MATRIX[k] for k in (0, 6, 8, 3, 7, 9, 1, 5)]):
            raw, mv, samples = pixels(w, h, kind, 300 + i)
            sb = samples.dtype.itemsize
            pitch = w * spp_of(fmt) * sb + sb
            s = Surface(enc, samples[None], fmt, pitch, leads=(0, sb, 7 * sb), seed=i)
            surfs.append(s)
            jobs.append(enqueue(enc, s.planes(), fmt, pitch, 1, w, h, o, mv, sb))  # NULL stream: round-robin
            want.append(expected(raw, mv, sub, tables))
        enc.synchronize()
        got = [collect(enc, j)[0] for j in jobs]
        for s in surfs:
            s.free()
        assert got == want
    finally:
        enc.close()


def test_restart_interval(encoder, tables):
    w, h = 257, 33
    raw, mv, samples = pixels(w, h, "u8", 77)
    pitch = w * 4 + 1
    s = Surface(encoder, samples[None], RGBX, pitch, seed=2)
    try:
        for sub in SUBS:
            got = encode(encoder, s.planes(), RGBX, pitch, 1, w, h, opts(sub, tables, ri=7), mv, 1)
            assert got == [expected(raw, mv, sub, tables, ri=7)]
    finally:
        s.free()


# ------------------------------------------------------------------ arguments

def test_invalid_arguments(encoder, tables):
    L = dmmt_jpeg.lib()
    w, h = 64, 16
    d = encoder.malloc(1 << 16)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, 0)
    d_out, d_len = encoder.malloc(cap), encoder.malloc(4)
    o = opts(0, tables).to_c()

    def rc(planes, fmt, pitch, sb=1, fstride=0, out_stride=cap, n=1):
        s = dmmt_jpeg.Encoder.surfaces(planes, fmt, pitch, n, w, h, d_out, out_stride, d_len, fstride, 255, sb)
        return L.dmmt_encode_device_surfaces(encoder.handle, ctypes.byref(s), ctypes.byref(o), None)
    try:
        assert rc(d, RGB, w * 3) == 0
        for fmt, sb in [(RGBX, 2), (BGRX, 4), (RGBX, 4), (BGRX, 2), (PLANAR, 2), (RGB, 3)]:  # outside the matrix
            assert rc([d, d + 4096, d + 8192], fmt, 4096, sb=sb) == -102, (fmt, sb)
        assert rc(d, 5, w * 3) == -102 and rc(d, -1, w * 3) == -102       # format out of range
        assert rc(0, RGB, w * 3) == -102                                   # a needed plane is NULL
        assert rc([d, 0, d + 8192], PLANAR, w) == -102 and rc([d, d + 4096, 0], PLANAR, w) == -102
        assert rc(d, RGB, w * 3 - 1) == -102 and rc(d, RGBX, w * 4 - 1) == -102  # pitch below the row
        assert rc([d, d + 4096, d + 8192], PLANAR, w - 1) == -102
        assert rc(d, RGB, w * 6 + 1, sb=2) == -102                         # pitch not a multiple of sample_bytes
        assert rc(d, RGB, w * 12 + 2, sb=4) == -102
        assert rc(d + 1, RGB, w * 6, sb=2) == -102                         # plane not aligned to sample_bytes
        assert rc([d, d + 4098, d + 8192], PLANAR, w * 4, sb=4) == -102
        assert rc(d, RGB, w * 6, sb=2, fstride=4097, n=2) == -102          # frame stride not aligned
        assert rc(d, RGB, (1 << 30) + 1) == -102                           # above DMMT_MAX_ROW_PITCH
        assert rc(d, RGB, w * 3, out_stride=cap - 1) == -203               # DMMT_E_CAPACITY
        assert rc(d, RGB, w * 3, n=0) == -102
        encoder.synchronize()
    finally:
        for p in (d, d_out, d_len):
            encoder.free(p)


# ------------------------------------------------------------------ tensors

def test_tensors(encoder, tables):
    import torch
    sub = 2
    o = opts(sub, tables)
    dev = torch.device("cuda", 0)
    w, h = 257, 33
    raw, mv, _ = pixels(w, h, "u8", 500)
    want = expected(raw, mv, sub, tables)

    chw = torch.from_numpy(np.ascontiguousarray(raw.transpose(2, 0, 1))).to(dev)
    assert encoder.encode_tensor(chw, o) == [want]
    assert encoder.encode_tensor(chw.flip(0).contiguous(), o, layout="CHW-BGR") == [want]

    rgbx = np.concatenate([raw, noise(h * w, 1).reshape(h, w, 1)], axis=2)
    assert encoder.encode_tensor(torch.from_numpy(rgbx).to(dev), o) == [want]
    hwc = torch.from_numpy(raw).to(dev)
    assert encoder.encode_tensor(hwc, o) == [want]
    assert encoder.encode_tensor(hwc.flip(2).contiguous(), o, layout="HWC-BGR") == [want]

    big_raw, _, _ = pixels(300, 40, "u8", 501)
    big = torch.from_numpy(np.ascontiguousarray(big_raw.transpose(2, 0, 1))).to(dev)
    crop = big[:, 3:36, 5:262]
    assert not crop.is_contiguous()
    assert encoder.encode_tensor(crop, o) == [expected(np.ascontiguousarray(big_raw[3:36, 5:262]), 255, sub, tables)]

    braw, _, _ = pixels(w, h, "u8", 502, n=2)
    assert encoder.encode_tensor(torch.from_numpy(braw).to(dev), o) == [expected(braw[f], 255, sub, tables)
                                                                         for f in range(2)]

    f32 = raw.astype(np.float32) / np.float32(255)
    fchw = torch.from_numpy(np.ascontiguousarray(f32.transpose(2, 0, 1))).to(dev)
    assert encoder.encode_tensor(fchw, o) == [encoder.encode(dmmt_jpeg.Image.from_array(f32), o)]

    out, lens = encoder.encode_tensor_device(chw, o)  # device tensors, nothing synchronised
    assert out.is_cuda and lens.is_cuda and out.dtype == torch.uint8
    encoder.synchronize()
    assert out[0, :int(lens[0])].cpu().numpy().tobytes() == want

    with pytest.raises(ValueError):  # stride along W is not 1
        encoder.encode_tensor(torch.from_numpy(np.ascontiguousarray(raw.transpose(2, 1, 0))).to(dev).transpose(1, 2), o)
    with pytest.raises(ValueError):
        encoder.encode_tensor(torch.from_numpy(np.ascontiguousarray(raw.transpose(1, 0, 2))).to(dev).transpose(0, 1), o)
    with pytest.raises(ValueError):
        encoder.encode_tensor(chw.cpu(), o)
    with pytest.raises(ValueError):
        encoder.encode_tensor(chw.to(torch.float64), o)
    with pytest.raises(ValueError):  # (3, H, 3): HWC or CHW?
        encoder.encode_tensor(torch.zeros((3, 8, 3), dtype=torch.uint8, device=dev), o)
