"""YCbCr planes finer than the file on the device (dmmt_encode_device_ycc_subsample): 4:4:4
planes written as 4:2:2 or 4:2:0 files, 4:2:2 planes as 4:2:0 files, their chroma
box-averaged inside the front kernel.  The expected bytes are always those of the CPU
yardstick tests/ycc_subsample_ref.py (pinned by tests/test_ycc_subsample_reference.py).
Every plane is embedded in a larger device buffer whose other bytes -- the lead, the row
padding, the gap between frames, the tail -- are 0xFF: as samples they are codes above
every maximum, and none of them may reach the output or the error check.

Block forms: the shared encoder chooses per call (DMMT_COEF_FORMAT=auto): quality 50
tables give the narrow 80-byte blocks, all-ones tables the wide ones.  Helpers:
tests/test_gpu_ycc_matrix.py's and tests/test_gpu_tile_loops.py's, imported."""
import ctypes
import os

import numpy as np
import pytest

import dmmt_jpeg
import test_gpu_tile_loops as loops
import test_gpu_ycc_matrix as gm
import ycc_levels_ref as lv
import ycc_matrix_ref as mx
import ycc_ref
import ycc_subsample_ref as ss
from dmmt_jpeg import YccFormat as YF
from dmmt_jpeg import YccMatrix as M
from test_gpu_ycc_matrix import I010F, ONES, P010, U8F, U8L, Frames, collect, opts, planes_for, row_bytes

lc = gm.lc

pytestmark = pytest.mark.gpu

FORMATS = gm.FORMATS
PAIRS = list(ss.PAIRS)  # (planes' sampling, file's sampling)
PAIR_IDS = ["444to422", "444to420", "422to420"]
FORMS = gm.FORMS
WIDTHS, HEIGHTS = gm.WIDTHS, gm.HEIGHTS
P210 = P010  # the same levels; the planes are 4:2:2
LEVELS = [U8F, U8L, P010, I010F]
MATS = [M.JFIF, M.BT709, M.BT2020]
VALUE_EXCEEDS_MAX = -100
pairs = pytest.mark.parametrize("src,sub", PAIRS, ids=PAIR_IDS)
formats = pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])


@pytest.fixture(scope="module")
def q50():
    return dmmt_jpeg.quality_tables(50)


_ref = {}


def expected(planes, src, sub, tables, level, matrix, ri=0):
    key = (tuple(p.tobytes() for p in planes), planes[0].shape, src, sub, ri, tuple(tables[0]), tuple(tables[1]),
           level.depth, level.shift, int(level.rng), int(matrix))
    if key not in _ref:
        _ref[key] = ss.encode(*planes, src, sub, tables[0], tables[1], int(matrix), level.depth, level.shift,
                              int(level.rng), restart_interval=ri)
    return _ref[key]


def enqueue(enc, ptrs, fmt, lpitch, cpitch, n, w, h, src, options, level, matrix, fstride=0, stream=None):
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, int(options.chroma_subsampling_preset))  # the FILE's bound
    d_out, d_len = enc.malloc(n * cap), enc.malloc(4 * n)
    enc.encode_device_ycc(ptrs, fmt, lpitch, cpitch, n, w, h, options, d_out, cap, d_len, frame_stride=fstride,
                          stream=stream, levels=level.c() if level is not None else None, matrix=matrix,
                          chroma_sampling=src)
    return d_out, d_len, cap, n


def encode(enc, ptrs, fmt, lpitch, cpitch, n, w, h, src, options, level, matrix, fstride=0):
    job = enqueue(enc, ptrs, fmt, lpitch, cpitch, n, w, h, src, options, level, matrix, fstride)
    try:
        enc.synchronize()
    finally:
        out = collect(enc, job)
    return out


def encode_frames(enc, frames, fmt, src, sub, tables, level, matrix, lextra=0, cextra=0, leads=(0, 0, 0), ri=0):
    """one call for the frames' first; the planes lie at `src`; returns the files"""
    h, w = frames[0][0].shape
    lrow, crow = row_bytes(w, src, fmt, level.sb)
    s = Frames(enc, frames, fmt, lrow + lextra, crow + cextra, leads=leads)
    try:
        return encode(enc, s.ptrs, fmt, lrow + lextra, crow + cextra, 1, w, h, src, opts(sub, tables, ri), level, matrix)
    finally:
        s.free()


# ------------------------------------------------------------------ shapes and addressing

def shape_case(pair, fmt, form):
    return (PAIRS.index(pair) * 3 + int(fmt)) * 2 + FORMS.index(form)


def shape_sizes(case, li, k):
    i = case + 5 * li + 7 * k
    return i, WIDTHS[i % 6], HEIGHTS[(i // 6 + k) % 3]


@pytest.mark.parametrize("form", FORMS)
@formats
@pairs
def test_shapes_levels_matrices_and_pitches(encoder, q50, src, sub, fmt, form):
    """every level in every pair, format and block form: a seeded subset of widths x heights
    (each level sees two, all cases together every width with every height), the matrix
    going round JFIF, 709, 2020, plane pointers at leads 2, 6 and 14 bytes, pitches tight, +2
    and +16, luma != chroma; uint8 planes at odd leads and pitches as well"""
    tables = {"narrow-q50": q50, "wide-ones": (ONES, ONES)}[form]
    case = shape_case((src, sub), fmt, form)
    extras = ((0, 0), (2, 16), (16, 2))
    for li, level in enumerate(LEVELS):
        for k in range(2):
            i, w, h = shape_sizes(case, li, k)
            matrix = MATS[(case + li + k) % 3]
            planes = planes_for(w, h, src, 100 * case + 10 * li + k, level, low_bits=True)
            le, ce = extras[(i + k) % 3]
            leads = [(2, 6, 14), (6, 14, 2), (14, 2, 6)][(k + li) % 3]
            if level.sb == 1:
                leads, le = (leads[0] + 1, leads[1], leads[2] + 1), le + ((k + li) & 1)
            got = encode_frames(encoder, [planes], fmt, src, sub, tables, level, matrix, le, ce, leads)
            assert got == [expected(planes, src, sub, tables, level, matrix)], (level, matrix, w, h, le, ce, leads)


def test_the_subset_covers_every_width_height_and_matrix():
    seen, mats = set(), set()
    for case in range(18):
        for li in range(len(LEVELS)):
            for k in range(2):
                seen.add(shape_sizes(case, li, k)[1:])
                mats.add((li, (case + li + k) % 3))
    assert seen == {(w, h) for w in WIDTHS for h in HEIGHTS}
    assert mats == {(li, m) for li in range(4) for m in range(3)}  # every level meets every matrix
    assert {shape_case(p, f, fo) for p in PAIRS for f in FORMATS for fo in FORMS} == set(range(18))


@pytest.mark.parametrize("level", [U8F, P010], ids=repr)
@formats
def test_aligned_planes_and_interior_tiles(encoder, q50, fmt, level):
    """512 x 32: whole tiles, two tile rows of the 4:2:2 file; leads 0 and 16: the first
    tile starts at the planes' first byte, or takes the loader's interior path"""
    w, h = 512, 32
    for (src, sub), matrix in zip(PAIRS, MATS):
        planes = planes_for(w, h, src, 900 + sub, level)
        for leads in ((0, 0, 0), (16, 16, 16)):
            got = encode_frames(encoder, [planes], fmt, src, sub, q50, level, matrix, 0, 0, leads)
            assert got == [expected(planes, src, sub, q50, level, matrix)], (src, sub, leads)


@pytest.mark.parametrize("level", [U8L, P210], ids=repr)
@pairs
def test_three_frames(encoder, q50, src, sub, level):
    w, h = 257, 17
    fmt = FORMATS[(src + sub) % 3]
    matrix = MATS[sub]
    frames = [planes_for(w, h, src, 21 + f, level) for f in range(3)]
    lrow, crow = row_bytes(w, src, fmt, level.sb)
    lp, cp = lrow + 2, crow + 6
    fstride = lc.frame_stride(h * max(lp, cp), level.sb)  # past every plane's span; whole samples, no multiple of 16
    assert fstride % 16 and fstride % level.sb == 0
    s = Frames(encoder, frames, fmt, lp, cp, fstride=fstride, leads=(2, 6, 14))
    try:
        got = encode(encoder, s.ptrs, fmt, lp, cp, 3, w, h, src, opts(sub, q50), level, matrix, fstride=fstride)
    finally:
        s.free()
    assert got == [expected(f, src, sub, q50, level, matrix) for f in frames]


@pytest.mark.parametrize("sub", [1, 2])
@formats
def test_region_of_interest_at_an_odd_origin(encoder, q50, fmt, sub):
    """a 61 x 19 rectangle at (3, 5) of 4:4:4 parent planes: the planes' chroma grid has no
    parity, the averaging cells start at the rectangle's first sample; the bytes are those
    of the cropped planes"""
    pw, ph, x, y, w, h = 80, 30, 3, 5, 61, 19
    for level, matrix in ((U8F, M.JFIF), (P010, M.BT709)):
        parent = planes_for(pw, ph, 0, 600 + sub, level, low_bits=True)
        crop = tuple(np.ascontiguousarray(p[y:y + h, x:x + w]) for p in parent)
        lrow, crow = row_bytes(pw, 0, fmt, level.sb)
        s = Frames(encoder, [parent], fmt, lrow, crow, leads=(2, 6, 14))
        try:
            step = level.sb if fmt == YF.PLANAR else 2 * level.sb
            ptrs = [s.ptrs[0] + y * lrow + x * level.sb] + [p + y * crow + x * step for p in s.ptrs[1:]]
            got = encode(encoder, ptrs, fmt, lrow, crow, 1, w, h, 0, opts(sub, q50), level, matrix)
        finally:
            s.free()
        assert got == [expected(crop, 0, sub, q50, level, matrix)], (level, matrix)


@pairs
def test_padded_luma_is_black_under_saturated_chroma(encoder, q50, src, sub):
    w, h = 7, 17
    for i, (level, matrix, fmt) in enumerate(((U8F, M.BT709, YF.NV), (P010, M.BT2020, YF.PLANAR))):
        top = (1 << level.depth) - 1
        dt = np.uint8 if level.sb == 1 else np.uint16
        ch, cw = ycc_ref.chroma_shape(w, h, src)
        y = planes_for(w, h, src, 50 + i, level)[0]
        cb = np.full((ch, cw), top << level.shift, dt)
        cr = np.full((ch, cw), 0, dt) if i % 2 else cb.copy()
        planes = (y, cb, cr)
        yp = ss.padded_planes(*planes, src, sub, int(matrix), level.depth, level.shift, int(level.rng))[0]
        assert np.all(yp[h:] == -128) and np.all(yp[:, w:] == -128) and yp.shape[0] > h and yp.shape[1] > w
        for t in (q50, (ONES, ONES)):
            got = encode_frames(encoder, [planes], fmt, src, sub, t, level, matrix, 2, 2, (2, 6, 14))
            assert got == [expected(planes, src, sub, t, level, matrix)], (level, matrix, fmt)


# ------------------------------------------------------------------ errors

@pytest.mark.parametrize("where", ["luma", "chroma"])
@formats
@pairs
def test_a_code_above_the_maximum(encoder, q50, src, sub, fmt, where):
    """10 bits at the bottom of a uint16, odd width and height: one sample 1024 in the first
    or in the last sample of a plane -- chroma: of the odd last row and column, which is
    averaged with padding -- is DMMT_E_VALUE_EXCEEDS_MAX at synchronize; the same sample in
    the pitch padding is not"""
    w, h = 263, 19
    level, matrix = I010F, MATS[(src + sub + int(fmt)) % 3]
    planes = planes_for(w, h, src, 70 + sub, level)
    want = expected(planes, src, sub, q50, level, matrix)
    lrow, crow = row_bytes(w, src, fmt, 2)
    lp, cp = lrow + 16, crow + 16
    o = opts(sub, q50)
    comp = (src + sub + int(fmt)) % 2  # chroma: Cb or Cr
    p = 0 if where == "luma" else (1 + comp if fmt == YF.PLANAR else 1)
    for y, x in ((0, 0), (planes[p].shape[0] - 1, planes[p].shape[1] - 1)):
        s = Frames(encoder, [planes], fmt, lp, cp, leads=(2, 6, 14))
        try:
            pitch = lp if p == 0 else cp
            step = 2 if p == 0 or fmt == YF.PLANAR else 4  # bytes between samples of a component
            first = 2 * (comp ^ (1 if fmt == YF.NV_VU else 0)) if p and fmt != YF.PLANAR else 0  # its place in a pair
            inside = s.ptrs[p] + y * pitch + x * step + first
            padding = s.ptrs[p] + y * pitch + (lrow if p == 0 else crow)  # the first sample after the row
            assert encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, src, o, level, matrix) == [want]
            encoder.h2d(padding, np.array([1024], np.uint16))
            assert encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, src, o, level, matrix) == [want]
            encoder.h2d(inside, np.array([1024], np.uint16))
            with pytest.raises(dmmt_jpeg.Error) as e:
                encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, src, o, level, matrix)
            assert e.value.code == VALUE_EXCEEDS_MAX, (y, x)
            encoder.h2d(inside, np.array([1023], np.uint16))  # the largest code is fine, and the error is gone
            fixed = [q.copy() for q in planes]
            fixed[0 if p == 0 else 1 + comp][y, x] = 1023
            assert encode(encoder, s.ptrs, fmt, lp, cp, 1, w, h, src, o, level, matrix) == \
                [expected(fixed, src, sub, q50, level, matrix)]
        finally:
            s.free()


# ------------------------------------------------------------------ equal samplings are the matrix call

@formats
def test_equal_samplings_are_the_matrix_call(encoder, q50, fmt):
    w, h = 257, 33
    L = dmmt_jpeg.lib()
    for sub in (0, 1, 2):
        for level, matrix in ((None, M.JFIF), (U8L, M.BT709), (P010, M.BT2020), (P010, M.JFIF)):
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
                outs = []
                for fn in (L.dmmt_encode_device_ycc_subsample, L.dmmt_encode_device_ycc_matrix):
                    assert fn(encoder.handle, ctypes.byref(y), lc_, int(matrix), ctypes.byref(oc), None) == 0
                    encoder.synchronize()
                    n = int(np.frombuffer(encoder.d2h(d_len, 4), np.uint32)[0])
                    outs.append(encoder.d2h(d_out, min(n, cap)))
                    encoder.h2d(d_out, np.zeros(64, np.uint8))
                want = mx.encode(*planes, sub, q50[0], q50[1], int(matrix), eff.depth, eff.shift, int(eff.rng))
                assert outs == [want, want], (sub, level, matrix)
                assert want == expected(planes, sub, sub, q50, eff, matrix)
            finally:
                s.free()
                encoder.free(d_out)
                encoder.free(d_len)


# ------------------------------------------------------------------ tile loops

def run_subsample_loop(enc, n_cus, fmt, src, sub, tables, level, matrix, seed):
    """2 x CUs small frames per call on a context of two lanes (tests/test_gpu_ycc_matrix.py's
    run_matrix_loop with planes at `src`): one workgroup per frame walks every tile, the
    prefetch included"""
    w, h = lc.shape(sub)
    n = 2 * n_cus
    lc.require_loops(w, h, sub, False, n, n_cus, True)
    distinct = [planes_for(w, h, src, 10 * seed + i, level, low_bits=True) for i in range(lc.N_DISTINCT)]
    want = [expected(p, src, sub, tables, level, matrix) for p in distinct]
    sb = level.sb
    lrow, crow = row_bytes(w, src, fmt, sb)
    lp, cp = lrow + sb, crow + 3 * sb
    assert lp % 16 and cp % 16 and lp != cp
    ch = ycc_ref.chroma_shape(w, h, src)[0]
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
                                                  L.d_len, frame_stride=fstride, levels=level.c(), matrix=matrix,
                                                  chroma_sampling=src))
        loops.compare(got, want)
    finally:
        L.free()


lanes_ctx = loops.lanes_ctx
cus = loops.cus


@pytest.mark.parametrize("ctx", loops.CTX)
@pytest.mark.parametrize("level", [U8L, P210], ids=repr)
@pairs
def test_tile_loops(lanes_ctx, cus, q50, src, sub, level, ctx):
    # (P010 / P210 planes in noise: shift = 16 - 10, no code can exceed the maximum)
    fmt = FORMATS[(src + sub + (level is P210)) % 3]
    matrix = MATS[(src + sub + (ctx == "narrow")) % 3]
    run_subsample_loop(lanes_ctx[ctx], cus, fmt, src, sub, q50, level, matrix, seed=800 + 7 * sub + src)


# ------------------------------------------------------------------ graph cache, lanes, restart, host planes, stripes

def test_graph_cache_tells_samplings_apart():
    """A context that replays captured graphs (DMMT_GRAPHS=1), the same pointers, pitches,
    levels and output buffer, the file 4:2:0: the planes read as 4:2:0, as 4:2:2 and as 4:4:4
    -- then each again, a replay.  A key without the planes' sampling replays another
    call's graph and its bytes."""
    os.environ["DMMT_GRAPHS"] = "1"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_GRAPHS")
    w, h, sub = 256, 16, 2
    tables = (ONES, ONES)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
    o = opts(sub, tables)
    try:
        for level, matrix in ((P010, M.BT709), (U8F, M.JFIF)):
            sb = level.sb
            # 4:4:4 buffers; read as 4:2:2 or 4:2:0 at the same pitch, they show their first columns / rows
            planes = planes_for(w, h, 0, 12, level, low_bits=True)
            views = {0: planes, 1: (planes[0], planes[1][:, :w // 2], planes[2][:, :w // 2]),
                     2: (planes[0], planes[1][:h // 2, :w // 2], planes[2][:h // 2, :w // 2])}
            order = [2, 1, 0]
            want = [expected(tuple(np.ascontiguousarray(p) for p in views[src]), src, sub, tables, level, matrix)
                    for src in order]
            assert len(set(want)) == 3
            ptrs = [enc.malloc(p.nbytes) for p in planes] + [enc.malloc(cap), enc.malloc(4)]
            d_out, d_len = ptrs[3], ptrs[4]
            try:
                for d, a in zip(ptrs, planes):
                    enc.h2d(d, a)
                for rep in range(2):  # the second round replays every graph
                    for src, ref in zip(order, want):
                        enc.encode_device_ycc(ptrs[:3], YF.PLANAR, sb * w, sb * w, 1, w, h, o, d_out, cap, d_len,
                                              levels=None if level is U8F else level.c(), matrix=matrix,
                                              chroma_sampling=None if src == sub and rep else src)
                        enc.synchronize()
                        n = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
                        assert enc.d2h(d_out, min(n, cap)) == ref, (rep, level, src)
            finally:
                for ptr in ptrs:
                    enc.free(ptr)
    finally:
        enc.close()


def test_four_lanes_with_alternating_pairs_and_levels(encoder, q50):
    w, h = 257, 33
    jobs, surfs, want = [], [], []
    try:
        encoder.set_lanes(4)
        for i in range(9):
            src, sub = PAIRS[i % 3]
            level = [P010, U8L, I010F, None][i % 4]  # None: NULL levels
            matrix = MATS[(i // 2) % 3]
            fmt = FORMATS[(i // 2) % 3]
            eff = level if level is not None else U8F
            planes = planes_for(w, h, src, 300 + i, eff, low_bits=True)
            lrow, crow = row_bytes(w, src, fmt, eff.sb)
            s = Frames(encoder, [planes], fmt, lrow + 2, crow + 16, leads=(2, 6, 14))
            surfs.append(s)
            jobs.append(enqueue(encoder, s.ptrs, fmt, lrow + 2, crow + 16, 1, w, h, src, opts(sub, q50), level, matrix))
            want.append(expected(planes, src, sub, q50, eff, matrix))
        encoder.synchronize()
        got = [collect(encoder, j)[0] for j in jobs]
        assert got == want
    finally:
        for s in surfs:
            s.free()
        encoder.set_lanes(1)  # the shared encoder's lane count, restored


def test_restart_interval(encoder, q50):
    w, h = 257, 33
    for (src, sub), fmt, level, matrix in zip(PAIRS, (YF.NV, YF.PLANAR, YF.NV_VU), (P010, U8L, U8F),
                                              (M.BT2020, M.BT709, M.JFIF)):
        planes = planes_for(w, h, src, 77, level)
        got = encode_frames(encoder, [planes], fmt, src, sub, q50, level, matrix, 2, 0, (2, 2, 6), ri=7)
        assert got == [expected(planes, src, sub, q50, level, matrix, ri=7)]


def test_encode_ycc_from_host_planes(encoder, q50):
    w, h = 257, 33
    P = dmmt_jpeg.ChromaSubsamplingPreset
    for src, sub in PAIRS:
        o = opts(sub, q50)
        y, cb, cr = planes_for(w, h, src, 500 + sub, P010, low_bits=True)
        want = expected((y, cb, cr), src, sub, q50, P010, M.BT2020)
        kw = dict(options=o, bit_depth=10, shift=6, range=dmmt_jpeg.YccRange.LIMITED, matrix=M.BT2020,
                  chroma_sampling=P(src))
        assert encoder.encode_ycc(y, cb=cb, cr=cr, **kw) == want
        assert encoder.encode_ycc(y, uv=np.stack([cb, cr], axis=2), **kw) == want
        assert encoder.encode_ycc(y, vu=np.stack([cr, cb], axis=2), **kw) == want
        y8, cb8, cr8 = planes_for(w, h, src, 510 + sub, U8F)
        assert encoder.encode_ycc(y8, cb=cb8, cr=cr8, options=o, chroma_sampling=src) == \
            expected((y8, cb8, cr8), src, sub, q50, U8F, M.JFIF)
        with pytest.raises(ValueError):  # the shapes go by the planes' sampling
            encoder.encode_ycc(y8, cb=cb8, cr=cr8, options=o)
        with pytest.raises(dmmt_jpeg.Error):  # a file finer than the planes
            f8 = planes_for(w, h, sub, 1, U8F)
            encoder.encode_ycc(*f8[:1], cb=f8[1], cr=f8[2], options=opts(src, q50), chroma_sampling=sub)
    y8, cb8, cr8 = planes_for(w, h, 2, 520, U8F)  # a value that equals the preset: today's bytes
    assert encoder.encode_ycc(y8, cb=cb8, cr=cr8, options=opts(2, q50), chroma_sampling=2) == \
        ycc_ref.encode(y8, cb8, cr8, 2, q50[0], q50[1])


def test_the_call_invalidates_a_pending_stripe(encoder, q50):
    """as every other encoding call (tests/test_gpu_sequences.py): after a subsample call the
    stripe's next step is refused, and a fresh analyze works again"""
    w, h = 64, 16
    o = opts(0, q50, ri=8)  # one MCU row per restart interval
    rgb = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    d_rgb, d_out = encoder.malloc(rgb.size), encoder.malloc(1 << 20)
    planes = planes_for(w, h, 0, 3, P010)
    try:
        encoder.h2d(d_rgb, rgb)
        st = encoder.stripe(d_rgb, w, h, 0, 2)
        hist = encoder.stripe_analyze(st, o)
        assert encode_frames(encoder, [planes], YF.NV, 0, 2, q50, P010, M.BT709) == \
            [expected(planes, 0, 2, q50, P010, M.BT709)]
        with pytest.raises(dmmt_jpeg.Error) as e:
            encoder.stripe_encode(hist, d_out, 1 << 20)
        assert e.value.code == -102
        hist = encoder.stripe_analyze(st, o)
        n = encoder.stripe_encode(hist, d_out, 1 << 20)
        encoder.synchronize()
        import oracle
        assert encoder.d2h(d_out, n) == oracle.encode(rgb, 255, 0, q50[0], q50[1], restart_interval=8)
    finally:
        encoder.free(d_rgb)
        encoder.free(d_out)
