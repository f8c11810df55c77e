"""Grayscale device frames (dmmt_encode_device_gray): a one-channel plane encoded
where it lies as a single-component file.  The expected bytes are always those of
the CPU yardstick tests/gray_ref.py (pinned by tests/test_gray_reference.py).  Every
plane is embedded in a larger device buffer whose other bytes -- the lead, the row
padding, the parent frame around a region of interest, the gap between frames --
are seeded random bytes that include 0xFF: none of them may reach the output.  On a
mismatch the message says whether the decoded blocks differ (the front half:
k_front_gray) or only the bytes (the back half: tables, header, emission)."""
import ctypes
import os

import numpy as np
import pytest

import dmmt_jpeg
import gray_ref
import oracle
from conftest import synthetic
from dmmt_jpeg import GrayTransfer as GT
from oracle import jpeg_scan

pytestmark = pytest.mark.gpu

ONES, ALL255 = [1] * 64, [255] * 64
WIDTHS = [1, 7, 255, 256, 257, 513]   # both sides of the 256-column tile
HEIGHTS = [1, 8, 9, 17, 33]           # 513 x 33: 325 blocks, past one 256-block chunk
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32}

_noise = None


def noise(n, seed):
    """n seeded random bytes, 0xFF among them"""
    global _noise
    if _noise is None:
        _noise = np.random.default_rng(78).integers(0, 256, 4 << 20, dtype=np.uint8)
        _noise[::7] = 0xFF
    off = (seed * 4099) % 4096
    assert off + n <= _noise.size
    return _noise[off:off + n].copy()


def opts(luma, ri=0):
    # (the chroma table and the subsampling are ignored by a gray call)
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(2), 8, luma_table=list(luma),
                                              chroma_table=ALL255, restart_interval=ri)


def random_plane(w, h, sb, maxval, seed):
    rng = np.random.default_rng(seed)
    if sb == 4:
        return rng.random((h, w), dtype=np.float32)
    return rng.integers(0, maxval + 1, (h, w)).astype(DTYPES[sb])


_ref = {}


def expected(plane, maxval, luma, transfer=GT.AS_RGB, ri=0):
    key = (plane.tobytes(), plane.shape, plane.dtype.str, maxval, tuple(luma), int(transfer), ri)
    if key not in _ref:
        _ref[key] = gray_ref.encode(plane, maxval, luma, int(transfer), ri)
    return _ref[key]


def check(got, want, what=""):
    """byte equality; the message tells the front half from the back half"""
    if got == want:
        return
    try:
        _, gb, _ = jpeg_scan.decode_coefficients(got)
        _, wb, _ = jpeg_scan.decode_coefficients(want)
        if gb.shape != wb.shape:
            where = f"{gb.shape[0]} decoded blocks against {wb.shape[0]} (front half)"
        elif not np.array_equal(gb, wb):
            blk = int(np.argwhere((gb != wb).any(axis=1))[0, 0])
            where = f"the decoded blocks differ, first at block {blk} (front half)"
        else:
            where = "the decoded blocks agree, only the bytes differ (back half)"
    except Exception as e:  # the output does not even decode
        where = f"the output does not decode ({type(e).__name__}: {e}): back half"
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {first}; {where}")


class Plane:
    """frames embedded in noise: one device buffer, the plane `lead` bytes into it,
    rows `pitch` bytes apart, frames `fstride` bytes apart"""

    def __init__(self, enc, frames, pitch, lead=0, fstride=0, seed=1, tail=0):
        self.enc = enc
        h, w = frames[0].shape
        size = lead + (len(frames) - 1) * fstride + (h - 1) * pitch + w * frames[0].itemsize + tail
        host = gray_ref.pack_plane(frames, pitch, lead, tail, noise(size, seed), fstride)
        self.buf = enc.malloc(size)
        enc.h2d(self.buf, host)
        self.ptr = self.buf + lead

    def free(self):
        self.enc.free(self.buf)


def enqueue(enc, ptr, pitch, n, w, h, options, sb=1, maxval=255, transfer=GT.AS_RGB, fstride=0, stream=None):
    cap = dmmt_jpeg.max_gray_jpeg_bytes(w, h)
    d_out, d_len = enc.malloc(n * cap), enc.malloc(4 * n)
    enc.encode_device_gray(ptr, pitch, n, w, h, options, d_out, cap, d_len, frame_stride=fstride, maxval=maxval,
                           sample_bytes=sb, transfer=transfer, stream=stream)
    return d_out, d_len, cap, n


def collect(enc, job):
    d_out, d_len, cap, n = job
    lens = np.frombuffer(enc.d2h(d_len, 4 * n), np.uint32)
    out = [enc.d2h(d_out + f * cap, min(int(lens[f]), cap)) for f in range(n)]
    enc.free(d_out)
    enc.free(d_len)
    return out


def encode(enc, ptr, pitch, n, w, h, options, **kw):
    job = enqueue(enc, ptr, pitch, n, w, h, options, **kw)
    try:
        enc.synchronize()
    finally:
        out = collect(enc, job)
    return out


def encode_plane(enc, plane, luma, maxval=255, transfer=GT.AS_RGB, extra=0, lead=0, ri=0, seed=1):
    """one frame, rows `extra` samples longer than the image's, `lead` bytes into its buffer"""
    h, w = plane.shape
    sb = plane.itemsize
    s = Plane(enc, [plane], (w + extra) * sb, lead, seed=seed)
    try:
        return encode(enc, s.ptr, (w + extra) * sb, 1, w, h, opts(luma, ri), sb=sb, maxval=maxval, transfer=transfer)[0]
    finally:
        s.free()


@pytest.fixture(scope="module")
def q75():
    return dmmt_jpeg.quality_tables(75)[0]


@pytest.fixture(scope="module")
def q90():
    return dmmt_jpeg.quality_tables(90)[0]


# ------------------------------------------------------------------ sizes, placement

@pytest.mark.parametrize("w", WIDTHS)
def test_sizes_at_every_pitch_and_lead(encoder, q75, w):
    for i, h in enumerate(HEIGHTS):
        plane = random_plane(w, h, 1, 255, 1000 * w + h)
        want = expected(plane, 255, q75)
        for extra, lead in ((0, 0), (0, 1), (1, 3), (13, 15)):
            got = encode_plane(encoder, plane, q75, extra=extra, lead=lead, seed=i + 3 * extra)
            check(got, want, f"{w}x{h} pitch +{extra} lead {lead}")


@pytest.mark.parametrize("sb,maxval,transfer", [(1, 255, GT.AS_RGB), (1, 255, GT.Y_FULL_RANGE), (2, 255, GT.AS_RGB),
                                                (2, 1023, GT.AS_RGB), (2, 65535, GT.AS_RGB), (4, 0, GT.AS_RGB)])
def test_samples_and_transfers(encoder, q75, sb, maxval, transfer):
    for (w, h), extra, lead in (((257, 33), 1, 3), ((513, 9), 13, 15), ((7, 17), 0, 1), ((769, 25), 0, 16)):
        plane = random_plane(w, h, sb, maxval, 50 * sb + w)
        for luma in (q75, ONES):  # (narrow under the auto rule for integer samples, wide)
            got = encode_plane(encoder, plane, luma, maxval, transfer, extra, lead * sb if sb > 1 else lead, seed=w)
            check(got, expected(plane, maxval, luma, transfer), f"sb {sb} maxval {maxval} transfer {transfer} {w}x{h}")


def test_three_frames_with_a_gap(encoder, q90):
    w, h = 257, 17
    for sb, maxval in ((1, 255), (2, 1023)):
        frames = [random_plane(w, h, sb, maxval, 21 + f) for f in range(3)]
        pitch = (w + 1) * sb
        fstride = h * pitch + 5 * sb  # not a multiple of 16
        assert fstride % 16
        s = Plane(encoder, frames, pitch, lead=3 * sb, fstride=fstride, seed=8)
        try:
            got = encode(encoder, s.ptr, pitch, 3, w, h, opts(q90), sb=sb, maxval=maxval, fstride=fstride)
        finally:
            s.free()
        for f in range(3):
            check(got[f], expected(frames[f], maxval, q90), f"frame {f} sb {sb}")


def test_region_of_interest(encoder, q90):
    """257 x 33 windows of a 300 x 40 parent: the window's pointer, the parent's pitch;
    (0, 0) starts at the plane's first byte, (43, 7) ends at its last"""
    pw, ph, w, h = 300, 40, 257, 33
    parent = random_plane(pw, ph, 1, 255, 40)
    pitch = pw + 4
    s = Plane(encoder, [parent], pitch, lead=0, seed=5)
    try:
        for x, y in [(0, 0), (1, 0), (16, 2), (10, 4), (43, 7)]:
            win = np.ascontiguousarray(parent[y:y + h, x:x + w])
            got = encode(encoder, s.ptr + y * pitch + x, pitch, 1, w, h, opts(q90))[0]
            check(got, expected(win, 255, q90), f"window at ({x}, {y})")
    finally:
        s.free()


# ------------------------------------------------------------------ samples

def test_sample_above_maxval_is_reported_and_the_context_survives(encoder, q75):
    w, h = 257, 9
    for sb, maxval in ((1, 200), (2, 1023)):
        plane = random_plane(w, h, sb, maxval, 60 + sb)
        bad = plane.copy()
        bad[h - 1, w - 1] = maxval + 1
        with pytest.raises(dmmt_jpeg.Error) as e:
            encode_plane(encoder, bad, q75, maxval)
        assert e.value.code == -100
        check(encode_plane(encoder, plane, q75, maxval), expected(plane, maxval, q75), f"after the error, sb {sb}")
    # the noise around the plane holds 0xFF > maxval: it never reaches the range check
    plane = random_plane(w, h, 1, 200, 63)
    check(encode_plane(encoder, plane, q75, 200, extra=13, lead=15), expected(plane, 200, q75), "noise above maxval")


def test_float_dots_outside_the_unit_range(encoder, q75):
    """values outside [0, 1], NaN and magnitudes whose coefficients reach category 15"""
    w, h = 257, 17
    rng = np.random.default_rng(5)
    plane = (rng.random((h, w), dtype=np.float32) * 3 - 1).astype(np.float32)
    plane[0:8, 8:16] = np.float32(15.0)                  # DC about 8 * 15 * 255: category 15
    plane[8:16, 16:24] = np.float32(-14.0)
    plane[3, 40] = np.float32(np.nan)                    # a NaN takes its block to 0 (quantizer.rs)
    plane[9, 100:103] = np.float32(-0.0), np.float32(1e-40), np.float32(2.0)
    zz = gray_ref.blocks(plane, 0, ONES)
    assert np.abs(zz.astype(np.int32)).max() >= 1 << 14 and zz.min() > -32768
    for luma in (ONES, q75):
        check(encode_plane(encoder, plane, luma, 0, extra=1, lead=4), expected(plane, 0, luma), "float dots")


def test_float_infinities_end_as_the_reference_does(encoder):
    """+Inf and -Inf saturate the quantiser at 32767 / -32768; -32768 has no category
    (categorize.rs:25-30): the yardstick raises there and synchronize reports -101"""
    w, h = 33, 9
    plane = np.random.default_rng(6).random((h, w), dtype=np.float32)
    plane[2, 3] = np.float32(np.inf)
    plane[4, 20] = np.float32(-np.inf)
    zz = gray_ref.blocks(plane, 0, ONES)
    if (zz == -32768).any():
        with pytest.raises(dmmt_jpeg.Error) as e:
            encode_plane(encoder, plane, ONES, 0)
        assert e.value.code == -101
    else:
        check(encode_plane(encoder, plane, ONES, 0), expected(plane, 0, ONES), "infinities")
    ok = random_plane(w, h, 4, 0, 7)
    check(encode_plane(encoder, ok, ONES, 0), expected(ok, 0, ONES), "after the infinities")


# ------------------------------------------------------------------ tables, constant and noise images, restart

@pytest.mark.parametrize("name", ["ones", "q75", "all255"])
def test_tables(encoder, q75, name):
    luma = {"ones": ONES, "q75": q75, "all255": ALL255}[name]
    for sb, maxval, transfer in ((1, 255, GT.AS_RGB), (1, 255, GT.Y_FULL_RANGE), (2, 1023, GT.AS_RGB)):
        plane = random_plane(513, 33, sb, maxval, 600 + sb)
        check(encode_plane(encoder, plane, luma, maxval, transfer, 1, 3 * sb), expected(plane, maxval, luma, transfer),
              f"{name} sb {sb} transfer {transfer}")


@pytest.mark.parametrize("fmt", ["wide", "narrow"])
def test_coef_format_contexts(q75, fmt):
    os.environ["DMMT_COEF_FORMAT"] = fmt
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_COEF_FORMAT")
    try:
        for sb, maxval, luma in ((1, 255, q75), (1, 255, ONES), (2, 1023, ONES), (4, 0, q75)):
            plane = random_plane(513, 33, sb, maxval, 700 + sb)
            check(encode_plane(enc, plane, luma, maxval, extra=1, lead=sb), expected(plane, maxval, luma),
                  f"{fmt} sb {sb}")
    finally:
        enc.close()


@pytest.mark.parametrize("value", [0, 128, 255])
def test_constant_image(encoder, q75, value):
    """one DC symbol and one AC symbol (EOB) -- or, with the padding's edge, a few"""
    for w, h in ((256, 16), (257, 33), (8, 8)):
        plane = np.full((h, w), value, np.uint8)
        for transfer in (GT.AS_RGB, GT.Y_FULL_RANGE):
            for luma in (q75, ONES):
                check(encode_plane(encoder, plane, luma, 255, transfer, 16, 5), expected(plane, 255, luma, transfer),
                      f"constant {value} {w}x{h} transfer {transfer}")


def test_noise_image(encoder):
    plane = noise(513 * 33, 9).reshape(33, 513)
    for luma in (ONES, ALL255):
        check(encode_plane(encoder, plane, luma, extra=1, lead=1), expected(plane, 255, luma), "noise")


@pytest.mark.parametrize("ri", [1, 3, 300, 1000])
def test_restart_intervals(encoder, q75, ri):
    """513 x 33 has 325 blocks: intervals inside a chunk, across the chunk boundary and
    larger than the frame"""
    plane = random_plane(513, 33, 1, 255, 77)
    for luma in (q75, ONES):
        check(encode_plane(encoder, plane, luma, extra=1, lead=1, ri=ri), expected(plane, 255, luma, ri=ri), f"ri {ri}")


def test_separate_tables_kernel(q75):
    os.environ["DMMT_FUSE_TABLES"] = "0"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_FUSE_TABLES")
    try:
        for (w, h), ri in (((513, 33), 0), ((257, 9), 3), ((1, 1), 0)):
            plane = random_plane(w, h, 1, 255, 88 + w)
            for luma in (q75, ONES):
                check(encode_plane(enc, plane, luma, extra=1, lead=1, ri=ri), expected(plane, 255, luma, ri=ri),
                      f"k_tables {w}x{h} ri {ri}")
        const = np.full((16, 16), 128, np.uint8)
        check(encode_plane(enc, const, q75, transfer=GT.Y_FULL_RANGE), expected(const, 255, q75, GT.Y_FULL_RANGE),
              "k_tables constant")
    finally:
        enc.close()


# ------------------------------------------------------------------ lanes, graph cache

def test_four_lanes_gray_and_colour_interleaved(encoder):
    """round-robin over four lanes, gray and colour calls of one size alternating: a
    lane's workspace serves both kinds in turn (its chroma histograms and code tables
    must survive the gray calls)"""
    w, h, sub = 257, 33, 0
    luma, chroma = dmmt_jpeg.quality_tables(80)
    o = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma, chroma_table=chroma)
    ccap = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
    jobs, bufs = [], []
    try:
        encoder.set_lanes(4)
        for i in range(14):  # lane i % 4 sees gray, colour, gray, ... or colour, gray, ...
            if (i + i // 4) % 2 == 0:
                plane = random_plane(w, h, 1, 255, 300 + i)
                s = Plane(encoder, [plane], w + 1, lead=1 + i, seed=i)
                bufs.append(s.buf)
                jobs.append(("gray", enqueue(encoder, s.ptr, w + 1, 1, w, h, o), expected(plane, 255, luma)))
            else:
                rgb = synthetic(w, h, frame=50 + i)
                d_in, d_out, d_len = encoder.malloc(rgb.nbytes), encoder.malloc(ccap), encoder.malloc(4)
                bufs.append(d_in)
                encoder.h2d(d_in, rgb)
                encoder.encode_device(d_in, 1, w, h, o, d_out, ccap, d_len)
                jobs.append(("colour", (d_out, d_len, ccap, 1), oracle.encode(rgb, 255, sub, luma, chroma)))
        encoder.synchronize()
        for i, (kind, job, want) in enumerate(jobs):
            got = collect(encoder, job)[0]
            if kind == "gray":
                check(got, want, f"call {i} (gray)")
            else:
                assert got == want, f"call {i} (colour)"
    finally:
        encoder.set_lanes(1)
        for b in bufs:
            encoder.free(b)


def test_graph_cache_tells_gray_from_colour_and_the_transfers_apart(q90):
    """A context that replays captured graphs (DMMT_GRAPHS=1), one input pointer, one
    output buffer: a gray call, a 4:4:4 colour call of the same size, a gray call at
    another pitch with the other transfer -- then each again, a replay.  A key without
    the component count, the transfer or the pitch replays another call's graph."""
    os.environ["DMMT_GRAPHS"] = "1"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_GRAPHS")
    w, h = 64, 16
    luma, chroma = dmmt_jpeg.quality_tables(90)
    o = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(0), 8, luma_table=luma, chroma_table=chroma)
    data = noise(w * h * 3, 3)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, 0)
    assert cap >= dmmt_jpeg.max_gray_jpeg_bytes(w, h)
    d_in, d_out, d_len = enc.malloc(data.size), enc.malloc(cap), enc.malloc(4)
    g1 = data[:w * h].reshape(h, w)
    g2 = np.ascontiguousarray(np.lib.stride_tricks.as_strided(data, (h, w), (w + 8, 1)))
    want = [expected(g1, 255, luma), oracle.encode(data.reshape(h, w, 3), 255, 0, luma, chroma),
            expected(g2, 255, luma, GT.Y_FULL_RANGE)]
    assert len(set(want)) == len(want)
    calls = [lambda: enc.encode_device_gray(d_in, w, 1, w, h, o, d_out, cap, d_len),
             lambda: enc.encode_device(d_in, 1, w, h, o, d_out, cap, d_len),
             lambda: enc.encode_device_gray(d_in, w + 8, 1, w, h, o, d_out, cap, d_len, transfer=GT.Y_FULL_RANGE)]
    try:
        enc.h2d(d_in, data)
        for rep in range(2):  # the second round replays every graph
            for i, (call, ref) in enumerate(zip(calls, want)):
                call()
                enc.synchronize()
                n = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
                got = enc.d2h(d_out, min(n, cap))
                if i == 1:
                    assert got == ref, (rep, "colour")
                else:
                    check(got, ref, f"round {rep} call {i}")
    finally:
        for p in (d_in, d_out, d_len):
            enc.free(p)
        enc.close()


def test_caller_stream(encoder, q90):
    import torch
    w, h = 257, 33
    plane = random_plane(w, h, 1, 255, 400)
    st = torch.cuda.Stream(torch.device("cuda", 0))
    s = Plane(encoder, [plane], w, lead=4, seed=9)
    try:
        job = enqueue(encoder, s.ptr, w, 1, w, h, opts(q90), stream=st.cuda_stream)
        encoder.synchronize()
        check(collect(encoder, job)[0], expected(plane, 255, q90), "caller stream")
    finally:
        s.free()


# ------------------------------------------------------------------ Python and C entry points

def test_encode_gray_from_host_arrays(encoder, q75):
    o = opts(q75)
    for sb, maxval in ((1, 255), (2, 1023), (4, 0)):
        plane = random_plane(257, 33, sb, maxval, 500 + sb)
        check(encoder.encode_gray(plane, maxval, o), expected(plane, maxval, q75), f"encode_gray sb {sb}")
    plane = random_plane(33, 9, 1, 255, 510)
    check(encoder.encode_gray(plane, options=o, transfer=GT.Y_FULL_RANGE), expected(plane, 255, q75, GT.Y_FULL_RANGE),
          "encode_gray Y_FULL_RANGE")
    with pytest.raises(ValueError):
        encoder.encode_gray(np.zeros((4, 4, 3), np.uint8), options=o)
    with pytest.raises(ValueError):
        encoder.encode_gray(np.zeros((4, 4), np.int32), options=o)


def test_encode_tensor_hw_on_a_strided_view(encoder, q75):
    import torch
    o = opts(q75)
    parent = torch.from_numpy(noise(3 * 40 * 300, 4).reshape(3, 40, 300).copy()).cuda()
    view = parent[:, 3:36, 11:268]  # (3, 33, 257): a batch of windows, rows 300 apart
    got = encoder.encode_tensor(view, o, layout="HW")
    host = view.cpu().numpy()
    assert len(got) == 3
    for f in range(3):
        check(got[f], expected(np.ascontiguousarray(host[f]), 255, q75), f"tensor frame {f}")
    one = encoder.encode_tensor(view[1], o, layout="hw", transfer=GT.Y_FULL_RANGE)
    check(one[0], expected(np.ascontiguousarray(host[1]), 255, q75, GT.Y_FULL_RANGE), "2-D tensor")
    with pytest.raises(ValueError):  # nothing about the inferred layouts changes: a 2-D tensor is not guessed
        encoder.encode_tensor(view[1], o)
    with pytest.raises(ValueError):
        encoder.encode_tensor(view[:, :, ::2], o, layout="HW")
    with pytest.raises(ValueError):  # a transfer means nothing to a colour layout
        encoder.encode_tensor(parent.permute(1, 2, 0), o, layout="HWC", transfer=GT.Y_FULL_RANGE)


def test_c_entry_point_for_a_host_image(encoder, q75):
    L = dmmt_jpeg.lib()
    o = opts(q75, ri=5).to_c()
    for sb, maxval, transfer in ((1, 255, GT.AS_RGB), (2, 1023, GT.AS_RGB), (1, 255, GT.Y_FULL_RANGE)):
        plane = random_plane(257, 17, sb, maxval, 520 + sb)
        im = dmmt_jpeg.DmmtGrayImage(257, 17, maxval, sb, plane.ctypes.data, int(transfer))
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        assert L.dmmt_jpeg_encode_gray(encoder.handle, ctypes.byref(im), ctypes.byref(o), ctypes.byref(out),
                                       ctypes.byref(n)) == 0
        got = ctypes.string_at(out.value, n.value)
        L.dmmt_free(out)
        check(got, expected(plane, maxval, q75, transfer, ri=5), f"dmmt_jpeg_encode_gray sb {sb}")
    bad = plane.copy()
    bad[0, 0] = 255
    bad_im = dmmt_jpeg.DmmtGrayImage(257, 17, 200, 1, bad.ctypes.data, 0)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.dmmt_jpeg_encode_gray(encoder.handle, ctypes.byref(bad_im), ctypes.byref(o), ctypes.byref(out),
                                   ctypes.byref(n)) == -100 and not out.value


# ------------------------------------------------------------------ arguments

def test_invalid_arguments(encoder, q75):
    L = dmmt_jpeg.lib()
    w, h = 64, 16
    d = encoder.malloc(1 << 16)
    cap = dmmt_jpeg.max_gray_jpeg_bytes(w, h)
    d_out, d_len = encoder.malloc(cap), encoder.malloc(4)

    def rc(ptr=d, pitch=w, n=1, width=w, height=h, out=d_out, out_stride=cap, ln=d_len, fstride=0, maxval=255, sb=1,
           transfer=0, o=None):
        g = dmmt_jpeg.Encoder.gray(ptr, pitch, n, width, height, out, out_stride, ln, fstride, maxval, sb, transfer)
        o = o if o is not None else opts(q75).to_c()
        return L.dmmt_encode_device_gray(encoder.handle, ctypes.byref(g), ctypes.byref(o), None)
    try:
        encoder.h2d(d, np.zeros(1 << 16, np.uint8))
        assert rc() == 0 and rc(sb=2, pitch=2 * w) == 0 and rc(sb=4, pitch=4 * w) == 0 and rc(transfer=1) == 0
        junk = opts(q75).to_c()  # subsampling and chroma_q are ignored
        junk.subsampling = 7
        junk.chroma_q[5] = 0
        assert rc(o=junk) == 0
        assert L.dmmt_encode_device_gray(encoder.handle, None, ctypes.byref(opts(q75).to_c()), None) == -102
        assert rc(ptr=0) == -102 and rc(out=0) == -102 and rc(ln=0) == -102
        assert rc(n=0) == -102 and rc(n=-1) == -102
        assert rc(width=0) == -102 and rc(height=0) == -102                      # an empty image
        assert rc(width=65535, pitch=65535, out_stride=1 << 40) == -102           # padded size beyond u16
        assert rc(pitch=w - 1) == -102 and rc(sb=2, pitch=2 * w - 2) == -102      # a pitch below the row's bytes
        assert rc(sb=2, pitch=2 * w + 1) == -102 and rc(sb=4, pitch=4 * w + 2) == -102  # not a multiple of the sample
        assert rc(sb=2, pitch=2 * w, ptr=d + 1) == -102 and rc(sb=2, pitch=2 * w, fstride=4097) == -102
        assert rc(pitch=(1 << 30) + 1) == -102                                   # above DMMT_MAX_ROW_PITCH
        assert rc(sb=0) == -102 and rc(sb=3, pitch=3 * w) == -102 and rc(sb=8, pitch=8 * w) == -102
        assert rc(transfer=1, sb=2, pitch=2 * w) == -102 and rc(transfer=1, sb=4, pitch=4 * w) == -102
        assert rc(transfer=2) == -102 and rc(transfer=-1) == -102                # an unknown transfer
        assert rc(maxval=0) == -102 and rc(maxval=0, sb=2, pitch=2 * w) == -102  # v / 0: integer AS_RGB samples
        assert rc(maxval=0, transfer=1) == 0 and rc(maxval=0, sb=4, pitch=4 * w) == 0  # (maxval unused there)
        zero = opts(q75).to_c()
        zero.luma_q[3] = 0
        assert rc(o=zero) == -102
        assert rc(out_stride=cap - 1) == -203                                    # DMMT_E_CAPACITY
        encoder.synchronize()
    finally:
        for p in (d, d_out, d_len):
            encoder.free(p)
