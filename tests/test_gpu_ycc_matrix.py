"""The YCbCr matrix step on the device (dmmt_encode_device_ycc_matrix): BT.709 and BT.2020
planes taken to the JFIF matrix inside the front kernel.  The expected bytes are always
those of the CPU yardstick tests/ycc_matrix_ref.py (pinned by
tests/test_ycc_matrix_reference.py).  Every plane is embedded in a larger device buffer
whose other bytes -- the lead, the row padding, the gap between frames, the tail -- are
0xFF: as samples they are codes above every maximum, and none of them may reach the
output or the error check.

Block forms: the shared encoder chooses per call (DMMT_COEF_FORMAT=auto): quality 50
tables give the narrow 80-byte blocks, all-ones tables the wide ones."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dmmt_jpeg
import test_gpu_tile_loops as loops
import ycc_levels_ref as lv
import ycc_matrix_ref as mx
import ycc_ref
from dmmt_jpeg import DmmtYccLevels
from dmmt_jpeg import YccFormat as YF
from dmmt_jpeg import YccMatrix as M
from dmmt_jpeg import YccRange as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import loop_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = [YF.PLANAR, YF.NV, YF.NV_VU]
SUBS = [0, 1, 2]
MATRICES = [M.BT709, M.BT2020]
WIDTHS = [1, 7, 255, 256, 257, 513]
HEIGHTS = [1, 17, 33]
FORMS = ["narrow-q50", "wide-ones"]
ONES = [1] * 64
VALUE_EXCEEDS_MAX = -100  # DMMT_E_VALUE_EXCEEDS_MAX
INVALID_ARGUMENT = -102    # DMMT_E_INVALID_ARGUMENT


class Level:
    def __init__(self, name, depth, shift, rng, sb):
        self.name, self.depth, self.shift, self.rng, self.sb = name, depth, shift, rng, sb

    def c(self):
        return DmmtYccLevels(int(self.rng), self.depth, self.sb, self.shift)

    def __repr__(self):
        return self.name


U8F = Level("u8-full", 8, 0, R.FULL, 1)
U8L = Level("u8-limited", 8, 0, R.LIMITED, 1)
P010 = Level("P010-limited", 10, 6, R.LIMITED, 2)
I010F = Level("I010-full", 10, 0, R.FULL, 2)
LEVELS = [U8F, U8L, P010, I010F]


def opts(sub, tables, ri=0):
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=tables[0],
                                              chroma_table=tables[1], restart_interval=ri)


@pytest.fixture(scope="module")
def q50():
    return dmmt_jpeg.quality_tables(50)


_ref = {}


def expected(planes, sub, tables, level, matrix, ri=0):
    key = (tuple(p.tobytes() for p in planes), planes[0].shape, sub, ri, tuple(tables[0]), tuple(tables[1]),
           level.depth, level.shift, int(level.rng), int(matrix))
    if key not in _ref:
        _ref[key] = mx.encode(*planes, sub, tables[0], tables[1], int(matrix), level.depth, level.shift,
                              int(level.rng), restart_interval=ri)
    return _ref[key]


def planes_for(w, h, sub, seed, level, **kw):
    return lv.random_planes(w, h, sub, seed, level.depth, level.shift, sample_bytes=level.sb, **kw)


def row_bytes(w, sub, fmt, sb):
    """(luma, chroma) bytes of a row"""
    cw = ycc_ref.chroma_shape(w, 1, sub)[1]
    return w * sb, cw * (1 if fmt == YF.PLANAR else 2) * sb


class Frames:
    """frames [(y, cb, cr), ...] embedded in 0xFF bytes: one device buffer per plane, the
    plane `lead` bytes into it, rows a pitch apart, frames `fstride` bytes apart"""

    def __init__(self, enc, frames, fmt, lpitch, cpitch, fstride=0, leads=(0, 0, 0), tail=32):
        self.enc = enc
        per_plane = [[lv.as_bytes(f[0]) for f in frames]]
        chroma = [lv.chroma_rows(f[1], f[2], int(fmt)) for f in frames]
        for p in range(len(chroma[0])):
            per_plane.append([c[p] for c in chroma])
        self.bufs, self.ptrs = [], []
        for p, rows in enumerate(per_plane):
            pitch = lpitch if p == 0 else cpitch
            nrows, rowb = rows[0].shape
            size = leads[p] + (len(frames) - 1) * fstride + (nrows - 1) * pitch + rowb + tail
            host = ycc_ref.pack_plane(rows, pitch, leads[p], tail, np.full(size, 0xFF, np.uint8), fstride)
            d = enc.malloc(size)
            enc.h2d(d, host)
            self.bufs.append(d)
            self.ptrs.append(d + leads[p])

    def free(self):
        for d in self.bufs:
            self.enc.free(d)


def enqueue(enc, planes, fmt, lpitch, cpitch, n, w, h, options, level, matrix, fstride=0, stream=None):
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, int(options.chroma_subsampling_preset))
    d_out, d_len = enc.malloc(n * cap), enc.malloc(4 * n)
    enc.encode_device_ycc(planes, fmt, lpitch, cpitch, n, w, h, options, d_out, cap, d_len, frame_stride=fstride,
                          stream=stream, levels=level.c() if level is not None else None, matrix=matrix)
    return d_out, d_len, cap, n


def collect(enc, job):
    d_out, d_len, cap, n = job
    lens = np.frombuffer(enc.d2h(d_len, 4 * n), np.uint32)
    out = [enc.d2h(d_out + f * cap, min(int(lens[f]), cap)) for f in range(n)]
    enc.free(d_out)
    enc.free(d_len)
    return out


def encode(enc, planes, fmt, lpitch, cpitch, n, w, h, options, level, matrix, fstride=0):
    job = enqueue(enc, planes, fmt, lpitch, cpitch, n, w, h, options, level, matrix, fstride)
    try:
        enc.synchronize()
    finally:
        out = collect(enc, job)
    return out


def encode_frames(enc, frames, fmt, sub, tables, level, matrix, lextra=0, cextra=0, leads=(0, 0, 0), ri=0):
    """one call for one frame; returns the files"""
    h, w = frames[0][0].shape
    lrow, crow = row_bytes(w, sub, fmt, level.sb)
    s = Frames(enc, frames, fmt, lrow + lextra, crow + cextra, leads=leads)
    try:
        return encode(enc, s.ptrs, fmt, lrow + lextra, crow + cextra, 1, w, h, opts(sub, tables, ri), level, matrix)
    finally:
        s.free()


# ------------------------------------------------------------------ shapes and addressing

def shape_case(matrix, fmt, sub, form):
    return ((MATRICES.index(matrix) * 3 + int(fmt)) * 3 + sub) * 2 + FORMS.index(form)


def shape_sizes(case, li, k):
    i = case + 5 * li + 7 * k
    return i, WIDTHS[i % 6], HEIGHTS[(i // 6 + k) % 3]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
@pytest.mark.parametrize("matrix", MATRICES, ids=[m.name for m in MATRICES])
def test_shapes_levels_and_pitches(encoder, q50, matrix, fmt, sub, form):
    """every level in every matrix, format, subsampling and block form: a seeded subset of
    widths x heights (each level sees two, all cases together every width with every
    height), plane pointers at leads 2, 6 and 14 bytes, pitches tight, +2 and +16, luma !=
    chroma; uint8 planes at odd leads and pitches as well"""
    tables = {"narrow-q50": q50, "wide-ones": (ONES, ONES)}[form]
    case = shape_case(matrix, fmt, sub, form)
    extras = ((0, 0), (2, 16), (16, 2))
    for li, level in enumerate(LEVELS):
        for k in range(2):
            i, w, h = shape_sizes(case, li, k)
            planes = planes_for(w, h, sub, 100 * case + 10 * li + k, level, low_bits=True)
            le, ce = extras[(i + k) % 3]
            leads = [(2, 6, 14), (6, 14, 2), (14, 2, 6)][(k + li) % 3]
            if level.sb == 1:
                leads, le = (leads[0] + 1, leads[1], leads[2] + 1), le + ((k + li) & 1)
            got = encode_frames(encoder, [planes], fmt, sub, tables, level, matrix, le, ce, leads)
            assert got == [expected(planes, sub, tables, level, matrix)], (level, w, h, le, ce, leads)


def test_the_subset_covers_every_width_and_height():
    seen = set()
    for case in range(36):
        for li in range(len(LEVELS)):
            for k in range(2):
                seen.add(shape_sizes(case, li, k)[1:])
    assert seen == {(w, h) for w in WIDTHS for h in HEIGHTS}
    cases = {shape_case(m, f, s, fo) for m in MATRICES for f in FORMATS for s in SUBS for fo in FORMS}
    assert cases == set(range(36))


@pytest.mark.parametrize("level", [U8L, P010], ids=repr)
@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_aligned_planes_and_interior_tiles(encoder, q50, fmt, level):
    """769 x 49: middle tiles take the loader's interior path; leads 0 and 16"""
    w, h = 769, 49
    for sub in SUBS:
        matrix = MATRICES[(sub + int(fmt)) % 2]
        planes = planes_for(w, h, sub, 900 + sub, level)
        for leads in ((0, 0, 0), (16, 0, 16)):
            got = encode_frames(encoder, [planes], fmt, sub, q50, level, matrix, 0, 0, leads)
            assert got == [expected(planes, sub, q50, level, matrix)], (sub, leads)


@pytest.mark.parametrize("level", [U8F, P010], ids=repr)
@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_three_frames(encoder, q50, fmt, level):
    w, h, sub = 257, 17, 2
    matrix = MATRICES[int(fmt) % 2]
    frames = [planes_for(w, h, sub, 21 + f, level) for f in range(3)]
    lrow, crow = row_bytes(w, sub, fmt, level.sb)
    lp, cp = lrow + 2, crow + 6
    fstride = h * lp + 10  # (covers the smaller chroma planes too) whole samples, not a multiple of 16
    assert fstride % 16 and fstride % level.sb == 0
    s = Frames(encoder, frames, fmt, lp, cp, fstride=fstride, leads=(2, 6, 14))
    try:
        got = encode(encoder, s.ptrs, fmt, lp, cp, 3, w, h, opts(sub, q50), level, matrix, fstride=fstride)
    finally:
        s.free()
    assert got == [expected(f, sub, q50, level, matrix) for f in frames]


# ------------------------------------------------------------------ clamps and padding

@pytest.mark.parametrize("level", [U8F, P010], ids=repr)
@pytest.mark.parametrize("matrix", MATRICES, ids=[m.name for m in MATRICES])
def test_each_output_hits_both_clamps(encoder, q50, matrix, level):
    """planes of extreme codes only -- each sample the lowest or the highest code -- so that
    Y', Cb' and Cr' each reach -128 and 127 by clamping, as the reference planes show"""
    w, h = 65, 17
    top = (1 << level.depth) - 1
    dt = np.uint8 if level.sb == 1 else np.uint16
    for fmt, sub in ((YF.PLANAR, 2), (YF.NV, 0), (YF.NV_VU, 1)):
        r = np.random.default_rng(40 + sub)
        ch, cw = ycc_ref.chroma_shape(w, h, sub)
        planes = tuple((r.integers(0, 2, s, dtype=np.uint32) * np.uint32(top) << np.uint32(level.shift)).astype(dt)
                       for s in ((h, w), (ch, cw), (ch, cw)))
        # before the clamps: the reference's own arithmetic on the transferred planes
        yp, cbp, crp = lv.padded_planes(*planes, sub, level.depth, level.shift, int(level.rng))
        a, b, c, d, e, f = mx.constants(int(matrix))
        hr, vr = ycc_ref.rates(sub)
        up = lambda p: np.repeat(np.repeat(p, vr, axis=0), hr, axis=1)[:h, :w]  # noqa: E731
        raw = ((yp[:h, :w] + a * up(cbp)) + b * up(crp), c * cbp + d * crp, e * cbp + f * crp)
        out = mx.padded_planes(*planes, sub, int(matrix), level.depth, level.shift, int(level.rng))
        for before, after in zip(raw, out):
            assert before.min() < -128 and before.max() > 127, (fmt, sub, before.min(), before.max())
            assert after.min() == -128 and after.max() == 127
        for t in (q50, (ONES, ONES)):
            got = encode_frames(encoder, [planes], fmt, sub, t, level, matrix, 2, 16, (2, 14, 6))
            assert got == [expected(planes, sub, t, level, matrix)], (fmt, sub)


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("w,h", [(7, 17), (257, 33)])
def test_padding_is_black_under_saturated_chroma(encoder, q50, w, h, sub):
    """constant saturated chroma: the cells the odd width and height cut share a chroma
    sample that would light the padded luma; it stays -128"""
    for i, (level, matrix, fmt) in enumerate(((U8F, M.BT709, YF.NV), (P010, M.BT2020, YF.PLANAR),
                                              (U8L, M.BT2020, YF.NV_VU))):
        top = (1 << level.depth) - 1
        dt = np.uint8 if level.sb == 1 else np.uint16
        ch, cw = ycc_ref.chroma_shape(w, h, sub)
        y = planes_for(w, h, sub, 50 + i, level)[0]
        cb = np.full((ch, cw), top << level.shift, dt)
        cr = np.full((ch, cw), 0, dt) if i % 2 else np.full((ch, cw), top << level.shift, dt)
        planes = (y, cb, cr)
        yp = mx.padded_planes(*planes, sub, int(matrix), level.depth, level.shift, int(level.rng))[0]
        assert np.all(yp[h:] == -128) and np.all(yp[:, w:] == -128) and yp.shape[0] > h and yp.shape[1] > w
        assert np.any(yp[:h, :w] != lv.padded_planes(*planes, sub, level.depth, level.shift, int(level.rng))[0][:h, :w])
        for t in (q50, (ONES, ONES)):
            got = encode_frames(encoder, [planes], fmt, sub, t, level, matrix, 2, 2, (2, 6, 14))
            assert got == [expected(planes, sub, t, level, matrix)], (level, matrix, fmt)


# ------------------------------------------------------------------ errors

@pytest.mark.parametrize("where", ["luma", "chroma"])
@pytest.mark.parametrize("fmt,sub", [(YF.PLANAR, 2), (YF.NV, 2), (YF.NV_VU, 0), (YF.PLANAR, 1)],
                         ids=["I420", "NV12", "NV42", "I422"])
def test_a_code_above_the_maximum(encoder, q50, fmt, sub, where):
    """10 bits at the bottom of a uint16: one sample 1024 inside the rectangle is
    DMMT_E_VALUE_EXCEEDS_MAX at synchronize; the same sample in the pitch padding is not"""
    w, h = 263, 19
    level, matrix = I010F, MATRICES[sub % 2]
    planes = planes_for(w, h, sub, 70 + sub, level)
    want = expected(planes, sub, q50, level, matrix)
    lrow, crow = row_bytes(w, sub, fmt, 2)
    lp, cp = lrow + 16, crow + 16
    o = opts(sub, q50)
    p = 0 if where == "luma" else 1 + (sub == 1)  # (the second chroma plane once, for planar)
    npl = 3 if fmt == YF.PLANAR else 2
    if p >= npl:
        p = 1
    for y, x in ((0, 0), (planes[p].shape[0] - 1, planes[p].shape[1] - 1)):
        s = Frames(encoder, [planes], fmt, lp, cp, leads=(2, 6, 14))
        try:
            pitch = lp if p == 0 else cp
            step = 2 if p == 0 or fmt == YF.PLANAR else 4  # bytes between samples of a component
            first = 2 if (p and fmt == YF.NV_VU) else 0    # Cb is the second of a Cr,Cb pair
            inside = s.ptrs[p] + y * pitch + x * step + first
            rowb = lrow if p == 0 else crow
            padding = s.ptrs[p] + y * pitch + rowb  # the first sample after the row
            # as laid: the padding is 0xFFFF everywhere, beyond the maximum
            assert encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, o, level, matrix) == [want]
            encoder.h2d(padding, np.array([1024], np.uint16))
            assert encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, o, level, matrix) == [want]
            encoder.h2d(inside, np.array([1024], np.uint16))
            with pytest.raises(dmmt_jpeg.Error) as e:
                encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, o, level, matrix)
            assert e.value.code == VALUE_EXCEEDS_MAX, (y, x)
            encoder.h2d(inside, np.array([1023], np.uint16))  # the largest code is fine, and the error is gone
            fixed = [q.copy() for q in planes]
            if p == 0 or fmt == YF.PLANAR:
                fixed[p][y, x] = 1023
            else:
                fixed[1][y, x] = 1023  # the pairs' first component of interest: Cb
            assert encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, o, level, matrix) == \
                [expected(fixed, sub, q50, level, matrix)]
        finally:
            s.free()


def test_an_unknown_matrix_is_refused(encoder, q50):
    w, h, sub = 16, 16, 0
    planes = planes_for(w, h, sub, 1, U8F)
    s = Frames(encoder, [planes], YF.PLANAR, w, w)
    try:
        for bad in (3, -1, 1 << 20):
            with pytest.raises(dmmt_jpeg.Error) as e:
                encode(encoder, s.ptrs, YF.PLANAR, w, w, 1, w, h, opts(sub, q50), U8F, bad)
            assert e.value.code == INVALID_ARGUMENT
    finally:
        s.free()


# ------------------------------------------------------------------ JFIF is the existing calls

@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_jfif_is_the_levels_call_and_the_plain_call(encoder, q50, fmt):
    w, h = 257, 33
    L = dmmt_jpeg.lib()
    for sub in SUBS:
        for level in (None, U8L, P010):
            eff = level if level is not None else U8F
            planes = planes_for(w, h, sub, 80 + sub, eff, low_bits=True)
            lrow, crow = row_bytes(w, sub, fmt, eff.sb)
            lp, cp = lrow + eff.sb, crow + 3 * eff.sb
            s = Frames(encoder, [planes], fmt, lp, cp, leads=(2, 4, 6))
            cap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
            d_out, d_len = encoder.malloc(cap), encoder.malloc(4)
            try:
                y = encoder.ycc(s.ptrs, fmt, lp, cp, 1, w, h, sub, d_out, cap, d_len)
                oc = opts(sub, q50).to_c()
                lc_ = ctypes.byref(level.c()) if level is not None else None
                calls = [lambda: L.dmmt_encode_device_ycc_matrix(encoder.handle, ctypes.byref(y), lc_, int(M.JFIF),
                                                                 ctypes.byref(oc), None),
                         lambda: L.dmmt_encode_device_ycc_levels(encoder.handle, ctypes.byref(y), lc_,
                                                                 ctypes.byref(oc), None)]
                if level is None:
                    calls.append(lambda: L.dmmt_encode_device_ycc(encoder.handle, ctypes.byref(y), ctypes.byref(oc),
                                                                  None))
                outs = []
                for call in calls:
                    assert call() == 0
                    encoder.synchronize()
                    n = int(np.frombuffer(encoder.d2h(d_len, 4), np.uint32)[0])
                    outs.append(encoder.d2h(d_out, min(n, cap)))
                want = lv.encode(*planes, sub, q50[0], q50[1], eff.depth, eff.shift, int(eff.rng))
                assert all(o == want for o in outs), (sub, level)
                assert want == expected(planes, sub, q50, eff, M.JFIF)
            finally:
                s.free()
                encoder.free(d_out)
                encoder.free(d_len)


# ------------------------------------------------------------------ tile loops

def run_matrix_loop(enc, n_cus, fmt, sub, tables, level, matrix, seed):
    """2 x CUs small frames per call on a context of two lanes (tests/test_gpu_tile_loops.py's
    run_ycc with levels and a matrix): one workgroup per frame walks every tile, the prefetch
    included"""
    w, h = lc.shape(sub)
    n = 2 * n_cus
    lc.require_loops(w, h, sub, False, n, n_cus, True)
    distinct = [planes_for(w, h, sub, 10 * seed + i, level, low_bits=True) for i in range(lc.N_DISTINCT)]
    want = [expected(p, sub, tables, level, matrix) for p in distinct]
    sb = level.sb
    lrow, crow = row_bytes(w, sub, fmt, sb)
    lp, cp = lrow + sb, crow + 3 * sb
    assert lp % 16 and cp % 16 and lp != cp
    ch = ycc_ref.chroma_shape(w, h, sub)[0]
    fstride = lc.frame_stride(max(h * lp, ch * cp), sb)  # one stride for every plane
    leads = (2, 6, 10)
    L = loops.Launch(enc, n, dmmt_jpeg.max_jpeg_bytes(w, h, sub))
    try:
        per_plane = [[lv.as_bytes(d[0]) for d in distinct]]
        chroma = [lv.chroma_rows(d[1], d[2], int(fmt)) for d in distinct]
        for p in range(len(chroma[0])):
            per_plane.append([c[p] for c in chroma])
        ptrs = []
        for p, rows in enumerate(per_plane):
            host = lc.embed(np.stack(rows)[lc.frame_of(n)], lp if p == 0 else cp, fstride, leads[p], seed + 11 * p)
            ptrs.append(L.upload(host) + leads[p])
        got = L.run(lambda: enc.encode_device_ycc(ptrs, fmt, lp, cp, n, w, h, opts(sub, tables), L.d_out, L.cap,
                                                  L.d_len, frame_stride=fstride, levels=level.c(), matrix=matrix))
        loops.compare(got, want)
    finally:
        L.free()


lanes_ctx = loops.lanes_ctx
cus = loops.cus


@pytest.mark.parametrize("ctx", loops.CTX)
@pytest.mark.parametrize("level", [U8L, P010], ids=repr)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
def test_tile_loops(lanes_ctx, cus, q50, fmt, sub, level, ctx):
    # (P010 planes in noise: shift = 16 - 10, no code can exceed the maximum)
    matrix = MATRICES[(int(fmt) + sub) % 2]
    run_matrix_loop(lanes_ctx[ctx], cus, fmt, sub, q50, level, matrix, seed=800 + 7 * sub)


# ------------------------------------------------------------------ graph cache, lanes, restart, host planes, stripes

def test_graph_cache_tells_matrices_apart():
    """A context that replays captured graphs (DMMT_GRAPHS=1), the same pointers, pitches,
    levels and output buffer: JFIF, 709, 2020 -- then each again, a replay.  A key without
    the matrix replays another call's graph and its bytes."""
    os.environ["DMMT_GRAPHS"] = "1"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_GRAPHS")
    w, h, sub = 256, 16, 2
    tables = (ONES, ONES)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
    ch, cw = ycc_ref.chroma_shape(w, h, sub)
    o = opts(sub, tables)
    try:
        for level in (P010, U8F):  # (U8F with JFIF: NULL levels, the plain kernel's key)
            planes = planes_for(w, h, sub, 12, level, low_bits=True)
            order = [M.JFIF, M.BT709, M.BT2020]
            want = [expected(planes, sub, tables, level, m) for m in order]
            assert len(set(want)) == 3
            ptrs = [enc.malloc(p.nbytes) for p in planes] + [enc.malloc(cap), enc.malloc(4)]
            d_out, d_len = ptrs[3], ptrs[4]
            try:
                for d, a in zip(ptrs, planes):
                    enc.h2d(d, a)
                for rep in range(2):  # the second round replays every graph
                    for m, ref in zip(order, want):
                        enc.encode_device_ycc(ptrs[:3], YF.PLANAR, level.sb * w, level.sb * cw, 1, w, h, o, d_out, cap,
                                              d_len, levels=None if level is U8F else level.c(), matrix=m)
                        enc.synchronize()
                        n = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
                        assert enc.d2h(d_out, min(n, cap)) == ref, (rep, level, m)
            finally:
                for ptr in ptrs:
                    enc.free(ptr)
    finally:
        enc.close()


def test_four_lanes_with_alternating_matrices_and_levels(encoder, q50):
    w, h, sub = 257, 33, 2
    o = opts(sub, q50)
    jobs, surfs, want = [], [], []
    try:
        encoder.set_lanes(4)
        for i in range(9):
            level = [P010, U8L, I010F, None][i % 4]  # None: NULL levels
            matrix = [M.BT709, M.JFIF, M.BT2020][i % 3]
            fmt = FORMATS[(i // 2) % 3]
            eff = level if level is not None else U8F
            planes = planes_for(w, h, sub, 300 + i, eff, low_bits=True)
            lrow, crow = row_bytes(w, sub, fmt, eff.sb)
            s = Frames(encoder, [planes], fmt, lrow + 2, crow + 16, leads=(2, 6, 14))
            surfs.append(s)
            jobs.append(enqueue(encoder, s.ptrs, fmt, lrow + 2, crow + 16, 1, w, h, o, level, matrix))  # round-robin
            want.append(expected(planes, sub, q50, eff, matrix))
        encoder.synchronize()
        got = [collect(encoder, j)[0] for j in jobs]
        assert got == want
    finally:
        for s in surfs:
            s.free()
        encoder.set_lanes(1)  # the shared encoder's lane count, restored


def test_restart_interval(encoder, q50):
    w, h = 257, 33
    for fmt, sub, level, matrix in ((YF.NV, 2, P010, M.BT2020), (YF.PLANAR, 1, U8L, M.BT709),
                                    (YF.NV_VU, 0, U8F, M.BT709)):
        planes = planes_for(w, h, sub, 77, level)
        got = encode_frames(encoder, [planes], fmt, sub, q50, level, matrix, 2, 0, (2, 2, 6), ri=7)
        assert got == [expected(planes, sub, q50, level, matrix, ri=7)]


def test_encode_ycc_from_host_planes(encoder, q50):
    w, h = 257, 33
    for sub in SUBS:
        o = opts(sub, q50)
        y, cb, cr = planes_for(w, h, sub, 500 + sub, P010, low_bits=True)
        want = expected((y, cb, cr), sub, q50, P010, M.BT2020)
        kw = dict(options=o, bit_depth=10, shift=6, range=R.LIMITED, matrix=M.BT2020)
        assert encoder.encode_ycc(y, cb=cb, cr=cr, **kw) == want
        assert encoder.encode_ycc(y, uv=np.stack([cb, cr], axis=2), **kw) == want
        assert encoder.encode_ycc(y, vu=np.stack([cr, cb], axis=2), **kw) == want
        y8, cb8, cr8 = planes_for(w, h, sub, 510 + sub, U8F)
        assert encoder.encode_ycc(y8, cb=cb8, cr=cr8, options=o, matrix=M.BT709) == \
            expected((y8, cb8, cr8), sub, q50, U8F, M.BT709)
        assert encoder.encode_ycc(y8, cb=cb8, cr=cr8, options=o) == ycc_ref.encode(y8, cb8, cr8, sub, q50[0], q50[1])
    with pytest.raises(dmmt_jpeg.Error):
        encoder.encode_ycc(y8, cb=cb8, cr=cr8, options=o, matrix=7)


def test_the_call_invalidates_a_pending_stripe(encoder, q50):
    """as every other encoding call (tests/test_gpu_sequences.py): after a matrix call the
    stripe's next step is refused, and a fresh analyze works again"""
    w, h, sub = 64, 16, 0
    o = opts(sub, q50, ri=8)  # one MCU row per restart interval
    rgb = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    d_rgb, d_out = encoder.malloc(rgb.size), encoder.malloc(1 << 20)
    planes = planes_for(w, h, sub, 3, P010)
    try:
        encoder.h2d(d_rgb, rgb)
        st = encoder.stripe(d_rgb, w, h, 0, 2)
        hist = encoder.stripe_analyze(st, o)
        assert encode_frames(encoder, [planes], YF.NV, sub, q50, P010, M.BT709) == \
            [expected(planes, sub, q50, P010, M.BT709)]
        with pytest.raises(dmmt_jpeg.Error) as e:
            encoder.stripe_encode(hist, d_out, 1 << 20)
        assert e.value.code == -102
        hist = encoder.stripe_analyze(st, o)
        n = encoder.stripe_encode(hist, d_out, 1 << 20)
        encoder.synchronize()
        import oracle
        assert encoder.d2h(d_out, n) == oracle.encode(rgb, 255, sub, q50[0], q50[1], restart_interval=8)
    finally:
        encoder.free(d_rgb)
        encoder.free(d_out)
