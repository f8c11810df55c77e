"""The front kernels' tile loop and k_hist's passes past the first, against the CPU
references.  A front kernel runs clamp(ntiles, 1, resident / n_frames) workgroups
per frame and k_hist at most 1024 (512 with several lanes) / n_frames: every other
test launches so few frames that a workgroup takes one tile and k_hist makes one
pass, except tight 16-byte-aligned RGB u8 and 4:4:4 k_hist.  Here one call encodes
2 x CUs frames of 290 pixels' width:

  * on a context of two lanes the front grid and k_hist's are exactly one workgroup
    per frame: it walks every tile of its frame in order -- from a full tile to the
    partial one at the right edge, on to the next tile row at another misalignment,
    down to the tile row of partial height -- and makes every k_hist pass;
  * on the session's one-lane context a front workgroup takes at least two tiles at
    a stride of up to 4 and k_hist runs two workgroups per frame.

Each case asserts this from the mirror of the grids' arithmetic
(tests/tools/loop_cases.py, held to csrc/launch_grids.hpp by
tests/test_launch_grids.py) before it encodes.  Frame f holds distinct[f % 5], five
seeded noise frames over the full range of the maxval; every output of the launch is
compared byte for byte with oracle.encode, tests/ycc_ref.py or tests/gray_ref.py.
Rows and frames are never a multiple of 16 bytes apart, and pitched planes lie in
noise that holds 0xFF."""
import os
import sys

import numpy as np
import pytest

import dmmt_jpeg
import test_gpu_gray as gray
import test_gpu_surfaces as surf
import test_gpu_ycc as ycc
import ycc_ref
from dmmt_jpeg import GrayTransfer as GT
from dmmt_jpeg import PixelFormat as PF
from dmmt_jpeg import YccFormat as YF

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import loop_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

SUBS = [0, 1, 2]
CTX = ["wide", "narrow"]
VALUE_EXCEEDS_MAX = -100  # DMMT_E_VALUE_EXCEEDS_MAX


@pytest.fixture(scope="module")
def tables():
    return dmmt_jpeg.quality_tables(90)


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def lanes_ctx():
    """two contexts of two lanes, the quantised blocks forced wide and narrow"""
    ctx = {}
    for fmt in CTX:
        os.environ["DMMT_COEF_FORMAT"] = fmt
        try:
            ctx[fmt] = dmmt_jpeg.Encoder(0)
        finally:
            os.environ.pop("DMMT_COEF_FORMAT")
        ctx[fmt].set_lanes(2)
    yield ctx
    for enc in ctx.values():
        enc.close()


class Launch:
    """device buffers of one case; run() enqueues, synchronises and reads the lengths
    first, then only each file's bytes"""

    def __init__(self, enc, n, cap):
        self.enc, self.n, self.cap, self.bufs = enc, n, cap, []
        self.d_out, self.d_len = self.upload(n * cap), self.upload(4 * n)

    def upload(self, host):
        d = self.enc.malloc(host if isinstance(host, int) else host.size)
        self.bufs.append(d)
        if not isinstance(host, int):
            self.enc.h2d(d, host)
        return d

    def run(self, call):
        call()
        self.enc.synchronize()
        lens = np.frombuffer(self.enc.d2h(self.d_len, 4 * self.n), np.uint32)
        return [self.enc.d2h(self.d_out + f * self.cap, min(int(lens[f]), self.cap)) for f in range(self.n)]

    def free(self):
        for d in self.bufs:
            self.enc.free(d)


def compare(got, want, check=None):
    """frame f against want[f % 5]; the five references differ from one another"""
    assert len(set(want)) == len(want)
    for f, data in enumerate(got):
        if data != want[f % lc.N_DISTINCT]:
            if check:
                check(data, want[f % lc.N_DISTINCT], f"frame {f}")
            first = next((i for i, (a, b) in enumerate(zip(data, want[f % lc.N_DISTINCT])) if a != b), -1)
            raise AssertionError(f"frame {f}: {len(data)} bytes against {len(want[f % lc.N_DISTINCT])}, first "
                                 f"difference at byte {first}; {sum(g != want[i % lc.N_DISTINCT] for i, g in enumerate(got))} "
                                 f"of {len(got)} frames differ")


# ------------------------------------------------------------------ the four families
# each: (enc, n_cus, ..., hot=False) -> None; with hot, one sample of maxval + 1 in the last
# frame: VALUE_EXCEEDS_MAX at synchronize, then exact again -- once in the last pixel of the
# last tile (found in the workgroup's last iteration) and once in the first pixel of the
# first tile (found in its first and carried through every later one)

def hot_pixels(w, h):
    return [(h - 1, w - 1), (0, 0)]


def expect_error_then_exact(launch, hot_calls, call_clean, want, check=None):
    for call_hot in hot_calls:
        with pytest.raises(dmmt_jpeg.Error) as e:
            launch.run(call_hot)
        assert e.value.code == VALUE_EXCEEDS_MAX
        for _ in range(2):  # the next call of either lane
            compare(launch.run(call_clean), want, check)


def run_tight(enc, n_cus, lanes, kind, maxval, sub, tables, ri=0, hot=False, seed=1):
    """dmmt_encode_device: tight interleaved R,G,B frames"""
    w, h = lc.shape(sub)
    n = 2 * n_cus
    lc.require_loops(w, h, sub, False, n, n_cus, lanes)
    raw, mv, samples = surf.pixels(w, h, kind, seed, n=lc.N_DISTINCT, maxval=maxval)
    sb = samples.dtype.itemsize
    assert (w * 3 * sb) % 16 and (w * h * 3 * sb) % 16
    want = [surf.expected(raw[i], mv, sub, tables, ri) for i in range(lc.N_DISTINCT)]
    o = surf.opts(sub, tables, ri)
    frames = samples[lc.frame_of(n)]
    L = Launch(enc, n, dmmt_jpeg.max_jpeg_bytes(w, h, sub))
    try:
        def call(d):
            return lambda: enc.encode_device(d, n, w, h, o, L.d_out, L.cap, L.d_len, maxval=mv, sample_bytes=sb)
        d_in = L.upload(frames.reshape(-1).view(np.uint8))
        if not hot:
            return compare(L.run(call(d_in)), want)
        hot_calls = []
        for y, x in hot_pixels(w, h):
            bad = frames.copy()
            bad[n - 1, y, x, 2] = mv + 1
            hot_calls.append(call(L.upload(bad.reshape(-1).view(np.uint8))))
        expect_error_then_exact(L, hot_calls, call(d_in), want)
    finally:
        L.free()


def run_surface(enc, n_cus, lanes, fmt, kind, sub, tables, maxval=None, ri=0, hot=False, seed=1):
    """dmmt_encode_device_surfaces: rows one sample longer than tight, planar planes
    0, 1 and 7 samples into their buffers, frames 5 samples past the frame's span"""
    w, h = lc.shape(sub)
    n = 2 * n_cus
    lc.require_loops(w, h, sub, False, n, n_cus, lanes)
    raw, mv, samples = surf.pixels(w, h, kind, seed, n=lc.N_DISTINCT, maxval=maxval)
    sb = samples.dtype.itemsize
    pitch = w * surf.spp_of(fmt) * sb + sb
    fstride = lc.frame_stride(h * pitch, sb)
    assert pitch % 16 and fstride % 16
    want = [surf.expected(raw[i], mv, sub, tables, ri) for i in range(lc.N_DISTINCT)]
    o = surf.opts(sub, tables, ri)
    leads = (0, sb, 7 * sb)
    L = Launch(enc, n, dmmt_jpeg.max_jpeg_bytes(w, h, sub))

    def planes_of(per_frame, last=None):
        """device pointers of the planes; last: the rows of frame n - 1 instead"""
        ptrs = []
        for p in range(len(per_frame[0])):
            rows = np.stack([lc.as_rows(f[p]) for f in per_frame])[lc.frame_of(n)]
            if last is not None:
                rows[n - 1] = lc.as_rows(last[p])
            ptrs.append(L.upload(lc.embed(rows, pitch, fstride, leads[p], seed + 11 * p)) + leads[p])
        return ptrs if fmt == PF.PLANAR else ptrs[0]

    def call(planes):
        return lambda: enc.encode_device_surfaces(planes, fmt, pitch, n, w, h, o, L.d_out, L.cap, L.d_len,
                                                  frame_stride=fstride, maxval=mv, sample_bytes=sb)
    try:
        per_frame = [surf.plane_rows(samples[i], fmt, seed + i) for i in range(lc.N_DISTINCT)]
        clean = planes_of(per_frame)
        if not hot:
            return compare(L.run(call(clean)), want)
        hot_calls = []
        for y, x in hot_pixels(w, h):
            bad = samples[(n - 1) % lc.N_DISTINCT].copy()
            bad[y, x, 2] = mv + 1
            hot_calls.append(call(planes_of(per_frame, surf.plane_rows(bad, fmt, seed + (n - 1) % lc.N_DISTINCT))))
        expect_error_then_exact(L, hot_calls, call(clean), want)
    finally:
        L.free()


def run_ycc(enc, n_cus, lanes, fmt, sub, tables, ri=0, seed=1):
    """dmmt_encode_device_ycc: every plane at its own odd pitch and lead"""
    w, h = lc.shape(sub)
    n = 2 * n_cus
    lc.require_loops(w, h, sub, False, n, n_cus, lanes)
    distinct = [ycc_ref.random_planes(w, h, sub, 10 * seed + i) for i in range(lc.N_DISTINCT)]
    want = [ycc.expected(p, sub, tables, ri) for p in distinct]
    lrow, crow = ycc.row_bytes(w, sub, fmt)
    lp, cp = lrow + 1, crow + (3 if crow % 2 == 0 else 2)
    assert lp % 2 and cp % 2 and lp != cp
    ch = ycc_ref.chroma_shape(w, h, sub)[0]
    fstride = lc.frame_stride(max(h * lp, ch * cp), 1)  # one stride for every plane
    leads = (3, 5, 9)
    L = Launch(enc, n, dmmt_jpeg.max_jpeg_bytes(w, h, sub))
    try:
        per_plane = [[d[0] for d in distinct]]
        chroma = [ycc_ref.chroma_rows(d[1], d[2], int(fmt)) for d in distinct]
        for p in range(len(chroma[0])):
            per_plane.append([c[p] for c in chroma])
        ptrs = []
        for p, rows in enumerate(per_plane):
            host = lc.embed(np.stack([lc.as_rows(r) for r in rows])[lc.frame_of(n)], lp if p == 0 else cp, fstride,
                            leads[p], seed + 11 * p)
            ptrs.append(L.upload(host) + leads[p])
        got = L.run(lambda: enc.encode_device_ycc(ptrs, fmt, lp, cp, n, w, h, ycc.opts(sub, tables, ri), L.d_out, L.cap,
                                                  L.d_len, frame_stride=fstride))
        compare(got, want)
    finally:
        L.free()


def run_gray(enc, n_cus, lanes, sb, maxval, transfer, luma, ri=0, hot=False, seed=1):
    """dmmt_encode_device_gray: rows one sample longer than tight, 3 samples into the buffer"""
    w, h = lc.shape(0, gray=True)
    n = 2 * n_cus
    lc.require_loops(w, h, 0, True, n, n_cus, lanes)
    distinct = [gray.random_plane(w, h, sb, maxval, 10 * seed + i) for i in range(lc.N_DISTINCT)]
    want = [gray.expected(p, maxval, luma, transfer, ri) for p in distinct]
    pitch, lead = (w + 1) * sb, 3 * sb
    fstride = lc.frame_stride(h * pitch, sb)
    assert pitch % 16 and fstride % 16
    o = gray.opts(luma, ri)
    L = Launch(enc, n, dmmt_jpeg.max_gray_jpeg_bytes(w, h))
    try:
        def call(d):
            return lambda: enc.encode_device_gray(d + lead, pitch, n, w, h, o, L.d_out, L.cap, L.d_len,
                                                  frame_stride=fstride, maxval=maxval, sample_bytes=sb, transfer=transfer)
        rows = np.stack([lc.as_rows(p) for p in distinct])[lc.frame_of(n)]
        d_in = L.upload(lc.embed(rows, pitch, fstride, lead, seed))
        if not hot:
            return compare(L.run(call(d_in)), want, gray.check)
        hot_calls = []
        for y, x in hot_pixels(w, h):
            bad = distinct[(n - 1) % lc.N_DISTINCT].copy()
            bad[y, x] = maxval + 1
            rows[n - 1] = lc.as_rows(bad)
            hot_calls.append(call(L.upload(lc.embed(rows, pitch, fstride, lead, seed))))
        expect_error_then_exact(L, hot_calls, call(d_in), want, gray.check)
    finally:
        L.free()


# ------------------------------------------------------------------ tight frames

TIGHT = [("u8", 255), ("u8", 100), ("u16", 1000), ("u16", 65535), ("f32", 255)]  # (maxval 100: phase A's range check)
TIGHT_CASES = [(k, m, c) for k, m in TIGHT for c in CTX if not (k == "f32" and c == "narrow")]  # f32 has no narrow twin


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("kind,maxval,ctx", TIGHT_CASES, ids=[f"{k}-{m}-{c}" for k, m, c in TIGHT_CASES])
def test_tight_frames(lanes_ctx, cus, tables, kind, maxval, ctx, sub):
    run_tight(lanes_ctx[ctx], cus, True, kind, maxval, sub, tables, seed=100 + 7 * sub)


# ------------------------------------------------------------------ surfaces

SURFACE_CASES = [(f, k, c) for f, k in surf.MATRIX for c in CTX if not (k == "f32" and c == "narrow")]


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt,kind,ctx", SURFACE_CASES, ids=[f"{f.name}-{k}-{c}" for f, k, c in SURFACE_CASES])
def test_surfaces(lanes_ctx, cus, tables, fmt, kind, ctx, sub):
    run_surface(lanes_ctx[ctx], cus, True, fmt, kind, sub, tables, seed=200 + 7 * sub)


# ------------------------------------------------------------------ YCbCr

@pytest.mark.parametrize("ctx", CTX)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt", ycc.FORMATS, ids=[f.name for f in ycc.FORMATS])
def test_ycc(lanes_ctx, cus, tables, fmt, sub, ctx):
    run_ycc(lanes_ctx[ctx], cus, True, fmt, sub, tables, seed=300 + 7 * sub)


# ------------------------------------------------------------------ gray

GRAY = [(1, 255, GT.AS_RGB), (1, 255, GT.Y_FULL_RANGE), (2, 1000, GT.AS_RGB), (4, 0, GT.AS_RGB)]
GRAY_CASES = [(s, m, t, c) for s, m, t in GRAY for c in CTX if not (s == 4 and c == "narrow")]


@pytest.mark.parametrize("sb,maxval,transfer,ctx", GRAY_CASES, ids=[f"sb{s}-{m}-{t.name}-{c}" for s, m, t, c in GRAY_CASES])
def test_gray(lanes_ctx, cus, tables, sb, maxval, transfer, ctx):
    run_gray(lanes_ctx[ctx], cus, True, sb, maxval, transfer, tables[0], seed=400 + sb)


# ------------------------------------------------------------------ restart intervals

def restart_case(enc, n_cus, lanes, tables, bpm, ri):
    """one case per blocks-per-MCU count; k_hist steps the MCU index mod the interval by
    sm mod ri per pass (sm: the stride in MCUs, 256, 85, 64 and 42 here)"""
    if bpm == 1:
        run_gray(enc, n_cus, lanes, 1, 255, GT.AS_RGB, tables[0], ri=ri, seed=500)
    elif bpm == 3:
        run_tight(enc, n_cus, lanes, "u8", 255, 0, tables, ri=ri, seed=501)
    elif bpm == 4:
        run_surface(enc, n_cus, lanes, PF.BGR, "u16", 1, tables, ri=ri, seed=502)
    else:
        run_ycc(enc, n_cus, lanes, YF.NV, 2, tables, ri=ri, seed=503)


@pytest.mark.parametrize("ctx", CTX)
@pytest.mark.parametrize("bpm,ri", [(1, 7), (1, 100), (3, 7), (3, 100), (4, 7), (4, 100), (6, 7), (6, 100), (6, 1)])
def test_restart_intervals(lanes_ctx, cus, tables, bpm, ri, ctx):
    restart_case(lanes_ctx[ctx], cus, True, tables, bpm, ri)


# ------------------------------------------------------------------ one lane: strides above 1

@pytest.mark.parametrize("family", ["tight-u16-422", "BGRX-420", "NV12", "gray-u16"])
def test_one_lane(encoder, cus, tables, family):
    """the session's context: up to 4 front workgroups per frame, each with at least
    two tiles, and two k_hist workgroups per frame (a stride of 512 blocks)"""
    if family == "tight-u16-422":
        run_tight(encoder, cus, False, "u16", 1000, 1, tables, seed=600)
    elif family == "BGRX-420":
        run_surface(encoder, cus, False, PF.BGRX, "u8", 2, tables, seed=601)
    elif family == "NV12":
        run_ycc(encoder, cus, False, YF.NV, 2, tables, seed=602)
    else:
        run_gray(encoder, cus, False, 2, 1000, GT.AS_RGB, tables[0], seed=603)


# ------------------------------------------------------------------ the error carried across iterations

@pytest.mark.parametrize("ctx", CTX)
@pytest.mark.parametrize("family", ["tight-u16", "RGBX-u8-100", "gray-u16"])
def test_sample_above_maxval_in_the_last_and_in_the_first_tile(lanes_ctx, cus, tables, family, ctx):
    """maxval + 1 in the last pixel of the last tile of the last frame, which its
    workgroup reaches only in its last iteration; then in the first pixel of the first
    tile, a finding the workgroup carries through every later iteration"""
    enc = lanes_ctx[ctx]
    if family == "tight-u16":
        run_tight(enc, cus, True, "u16", 1000, 1, tables, hot=True, seed=700)
    elif family == "RGBX-u8-100":
        run_surface(enc, cus, True, PF.RGBX, "u8", 2, tables, maxval=100, hot=True, seed=701)
    else:
        run_gray(enc, cus, True, 2, 1000, GT.AS_RGB, tables[0], hot=True, seed=702)
