"""Seeded sweep of mixed call sequences on ONE context (GPU; the short run is
tests/test_gpu_sequences.py::test_seeded_sequences_short, a long one is not part of
the suite).  Where fuzz_parity.py checks one call at a time, every step here runs on
the context the steps before it left behind: asynchronous device encodes of every
entry point, sample type and table set stay in flight on the lanes and on callers'
streams while the synchronous entry points and the stripe protocol run among them,
lanes are added and dropped, and a call whose samples exceed maxval must surface
exactly once and spoil nothing else.  Every output is compared byte for byte with
its CPU reference (oracle, tests/ycc_ref.py, tests/gray_ref.py, the host PPM reader).
  python tests/tools/sequence_fuzz.py --steps 5000 --seed 1 [--minutes 5]
Prints one JSON line per 250 steps and a summary line; exits 1 on the first
mismatch (the failing step in the line).

The schedule (draw_schedule) depends on the seed alone and needs no GPU; this file
also holds the building blocks the sequence tests share: Job (one asynchronous
call and its reference), sync_op, striped_file and invalidated_stripe."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dmmt-jpeg-encoder_amd"), os.path.join(ROOT, "tests")]
import dmmt_jpeg  # noqa: E402
import gray_ref  # noqa: E402  (checker)
import oracle  # noqa: E402  (checker)
import ycc_ref  # noqa: E402  (checker)
from dmmt_jpeg import GrayTransfer, PixelFormat, YccFormat  # noqa: E402
from oracle.synth import synthetic  # noqa: E402

# an asynchronous call per entry point, sample type and maxval
ASYNC_KINDS = ("rgb_u8", "rgb_u8_mv100", "rgb_u16", "rgb_u16_mv1000", "rgb_f32", "bgrx_pitched", "planar_f32", "nv12",
               "i444_pitched", "gray_u16_mv4095", "gray_y")
# the synchronous entry points (they run on lane 0 and return their result)
SYNC_KINDS = ("encode", "encode_batch", "forward_blocks", "encode_coefficients", "dct_transform", "read_ppm_device",
              "convert_ppm_batch", "encode_gray", "encode_ycc")
STRIPE_KINDS = ("stripe_restart", "stripe_joined", "stripe_invalidated")
CONTROL_KINDS = ("synchronize", "set_lanes", "bad_maxval")
ALL_KINDS = ASYNC_KINDS + SYNC_KINDS + STRIPE_KINDS + CONTROL_KINDS
# q90: the narrow coefficient form (with escapes on noise); q100 and f32 dots: the wide form
QUALITIES = (50, 75, 90, 100)
MAX_OUTSTANDING = 12
INVALID_ARGUMENT = -102

MCU_W = {0: 8, 1: 16, 2: 16}
MCU_H = {0: 8, 1: 8, 2: 16}
# what runs between analyze and the later stripe step, and must invalidate the stripe
INVALIDATORS = ("encode_small", "encode_large", "encode_coefficients", "forward_blocks", "encode_gray",
                "encode_device")
STRIPE_MODES = ("restart", "joined_edges", "joined_measure", "joined_write")


def options(sub, q, ri=0):
    luma, chroma = dmmt_jpeg.quality_tables(q)
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                               chroma_table=chroma, restart_interval=ri)


def pixels(seed, n, h, w, maxval, content="noise"):
    """(n, h, w, 3) integer frames with samples in [0, maxval]: seeded noise, or the
    synthetic frames scaled to maxval"""
    dt = np.uint8 if maxval < 256 else np.uint16
    if content == "noise":
        return np.random.default_rng(seed).integers(0, maxval + 1, (n, h, w, 3)).astype(dt)
    s = np.stack([synthetic(w, h, frame=seed % 1000 + i) for i in range(n)]).astype(np.uint32)
    return (s * maxval // 255).astype(dt)


def _filler(seed, size):
    """seeded bytes around and between the rows of a pitched plane, 0xFF among them"""
    f = np.random.default_rng(seed ^ 0x5EED).integers(0, 256, size, dtype=np.uint8)
    f[::7] = 0xFF
    return f


def _pitched(frames, pitch, fstride, seed):
    """the uint8 buffer of a plane: frames (a list of 2-d sample arrays) with rows `pitch`
    and frames `fstride` bytes apart, filler everywhere else"""
    rows = [np.ascontiguousarray(f).view(np.uint8).reshape(f.shape[0], -1) for f in frames]
    size = (len(rows) - 1) * fstride + (rows[0].shape[0] - 1) * pitch + rows[0].shape[1]
    return ycc_ref.pack_plane(rows, pitch, 0, 0, _filler(seed, size), fstride)


def effective_sub(spec):
    """the subsampling a call of spec's kind runs with: NV12 and I444 name theirs, a
    gray frame has one component"""
    kind = spec["kind"]
    return {"nv12": 2, "i444_pitched": 0}.get(kind, 0 if kind.startswith("gray") else spec["sub"])


class Job:
    """One asynchronous call on an Encoder: the input uploaded at construction (no
    free and no copy between submit() calls, so consecutive submits stay in flight),
    submit(stream) enqueues, mismatch() compares every frame with the CPU reference
    once the context has been synchronised, free() releases the device memory.
    spec: kind (ASYNC_KINDS), w, h, n, sub, q, ri, seed, content; bad=True declares
    maxval 100 over samples up to 255 (rgb_u8 only)."""

    def __init__(self, enc, spec):
        self.enc, self.spec = enc, dict(spec)
        s = self.spec
        kind, w, h, n, seed = s["kind"], s["w"], s["h"], s.get("n", 1), s["seed"]
        content = s.get("content", "noise")
        self.bad = bool(s.get("bad"))
        self.n = n
        self.gray = kind.startswith("gray")
        self.sub = sub = effective_sub(s)
        self.opts = o = options(sub, s["q"], s.get("ri", 0))
        luma, chroma, ri = o.luma_table, o.chroma_table, o.restart_interval
        self.cap = dmmt_jpeg.max_gray_jpeg_bytes(w, h) if self.gray else dmmt_jpeg.max_jpeg_bytes(w, h, sub)
        self.bufs = []
        self._refs = None

        def up(a):
            a = np.ascontiguousarray(a)
            d = enc.malloc(a.nbytes)
            self.bufs.append(d)
            enc.h2d(d, a)
            return d

        if kind in ("rgb_u8", "rgb_u8_mv100", "rgb_u16", "rgb_u16_mv1000", "rgb_f32"):
            mv = {"rgb_u8": 255, "rgb_u8_mv100": 100, "rgb_u16": 65535, "rgb_u16_mv1000": 1000, "rgb_f32": 255}[kind]
            raw = pixels(seed, n, h, w, 255 if self.bad else mv, content)
            if self.bad:
                assert kind == "rgb_u8"
                raw[0, 0, 0, 0] = 255
                mv = 100
            samples = raw.astype(np.float32) / np.float32(mv) if kind == "rgb_f32" else raw
            d, sb = up(samples), samples.dtype.itemsize
            self._enqueue = lambda st: enc.encode_device(d, n, w, h, o, self.d_out, self.cap, self.d_len, maxval=mv,
                                                         sample_bytes=sb, stream=st)
            self._make_refs = lambda: [oracle.encode(raw[f], mv, sub, luma, chroma, restart_interval=ri)
                                       for f in range(n)]
        elif kind == "bgrx_pitched":
            raw = pixels(seed, n, h, w, 255, content)
            x = _filler(seed + 1, n * h * w).reshape(n, h, w, 1)
            bgrx = np.concatenate([raw[..., ::-1], x], axis=3).reshape(n, h, w * 4)
            pitch = w * 4 + 4 * (seed % 5)
            fstride = pitch * h + 16 if n > 1 else 0
            d = up(_pitched(list(bgrx), pitch, fstride, seed))
            self._enqueue = lambda st: enc.encode_device_surfaces(d, PixelFormat.BGRX, pitch, n, w, h, o, self.d_out,
                                                                  self.cap, self.d_len, frame_stride=fstride,
                                                                  stream=st)
            self._make_refs = lambda: [oracle.encode(raw[f], 255, sub, luma, chroma, restart_interval=ri)
                                       for f in range(n)]
        elif kind == "planar_f32":
            raw = pixels(seed, n, h, w, 255, content)
            dots = raw.astype(np.float32) / np.float32(255)
            pitch = w * 4 + 4 * (seed % 3)
            fstride = pitch * h + 8 if n > 1 else 0
            planes = [up(_pitched([dots[f, :, :, c] for f in range(n)], pitch, fstride, seed + c)) for c in range(3)]
            self._enqueue = lambda st: enc.encode_device_surfaces(planes, PixelFormat.PLANAR, pitch, n, w, h, o,
                                                                  self.d_out, self.cap, self.d_len,
                                                                  frame_stride=fstride, sample_bytes=4, stream=st)
            self._make_refs = lambda: [oracle.encode(raw[f], 255, sub, luma, chroma, restart_interval=ri)
                                       for f in range(n)]
        elif kind in ("nv12", "i444_pitched"):
            fmt = YccFormat.NV if kind == "nv12" else YccFormat.PLANAR
            ycc = [self._ycc_planes(seed + f, w, h, sub, content) for f in range(n)]
            stored = [ycc_ref.chroma_rows(cb, cr, fmt) for _, cb, cr in ycc]
            lp = w + seed % 7
            cp = stored[0][0].shape[1] + seed % 3
            fstride = max(lp * h, cp * stored[0][0].shape[0]) + 32 if n > 1 else 0
            planes = [up(_pitched([y for y, _, _ in ycc], lp, fstride, seed))]
            for k in range(len(stored[0])):
                planes.append(up(_pitched([st[k] for st in stored], cp, fstride, seed + 1 + k)))
            self._enqueue = lambda st: enc.encode_device_ycc(planes, fmt, lp, cp, n, w, h, o, self.d_out, self.cap,
                                                             self.d_len, frame_stride=fstride, stream=st)
            self._make_refs = lambda: [ycc_ref.encode(y, cb, cr, sub, luma, chroma, ri) for y, cb, cr in ycc]
        elif self.gray:
            if kind == "gray_u16_mv4095":
                mv, transfer = 4095, GrayTransfer.AS_RGB
            else:
                assert kind == "gray_y"
                mv, transfer = 255, GrayTransfer.Y_FULL_RANGE
            g = pixels(seed, n, h, w, mv, content)[..., 0]
            sb = g.dtype.itemsize
            pitch = (w + seed % 5) * sb
            fstride = pitch * h + 4 * sb if n > 1 else 0
            d = up(_pitched(list(g), pitch, fstride, seed))
            self._enqueue = lambda st: enc.encode_device_gray(d, pitch, n, w, h, o, self.d_out, self.cap, self.d_len,
                                                              frame_stride=fstride, maxval=mv, sample_bytes=sb,
                                                              transfer=transfer, stream=st)
            self._make_refs = lambda: [gray_ref.encode(g[f], mv, luma, int(transfer), ri) for f in range(n)]
        else:
            raise ValueError(kind)
        self.d_out = enc.malloc(n * self.cap)
        self.d_len = enc.malloc(4 * n)
        self.bufs += [self.d_out, self.d_len]

    @staticmethod
    def _ycc_planes(seed, w, h, sub, content):
        if content == "noise":
            return ycc_ref.random_planes(w, h, sub, seed)
        hr, vr = ycc_ref.rates(sub)
        s = synthetic(w, h, frame=seed % 1000)
        return (np.ascontiguousarray(s[:, :, 0]), np.ascontiguousarray(s[::vr, ::hr, 1]),
                np.ascontiguousarray(s[::vr, ::hr, 2]))

    def submit(self, stream=None):
        self.enc.h2d(self.d_len, np.zeros(self.n, np.uint32))  # a call that writes nothing leaves no file
        self._enqueue(stream)

    def references(self):
        if self._refs is None:
            self._refs = self._make_refs()
        return self._refs

    def outputs(self):
        lens = np.frombuffer(self.enc.d2h(self.d_len, 4 * self.n), np.uint32)
        return [self.enc.d2h(self.d_out + f * self.cap, min(int(lens[f]), self.cap)) for f in range(self.n)]

    def mismatch(self):
        """None when every frame's file is the reference's, else the first frame that differs"""
        for f, (got, want) in enumerate(zip(self.outputs(), self.references())):
            if got != want:
                return dict(frame=f, got_bytes=len(got), want_bytes=len(want), **self.spec)
        return None

    def free(self):
        for d in self.bufs:
            self.enc.free(d)
        self.bufs = []


# ------------------------------------------------------------------ synchronous entry points

def p3_text(rgb, maxval, seed):
    """a P3 file of rgb with seeded separators"""
    rng = np.random.default_rng(seed)
    seps = [b" ", b"\n", b"  ", b"\t", b" \n"]
    vals = rgb.reshape(-1).tolist()
    pick = rng.integers(0, len(seps), len(vals))
    body = b"".join(b"%d" % v + seps[int(k)] for v, k in zip(vals, pick))
    return b"P3\n%d %d\n%d\n" % (rgb.shape[1], rgb.shape[0], maxval) + body


def sync_op(enc, s):
    """One synchronous entry point (s["kind"] of SYNC_KINDS) on the context as it is,
    compared with its CPU reference; None, or what differed."""
    kind, w, h, sub, seed = s["kind"], s["w"], s["h"], s["sub"], s["seed"]
    content = s.get("content", "noise")
    o = options(sub, s["q"], s.get("ri", 0))
    luma, chroma, ri = o.luma_table, o.chroma_table, o.restart_interval
    mv = (255, 255, 1000, 65535, 100)[seed % 5]
    if kind == "encode":
        rgb = pixels(seed, 1, h, w, mv, content)[0]
        samples = rgb.astype(np.float32) / np.float32(mv) if seed % 3 == 0 else rgb  # Image<f32> dots among them
        got = enc.encode(dmmt_jpeg.Image.from_array(samples, mv), o)
        return None if got == oracle.encode(rgb, mv, sub, luma, chroma, restart_interval=ri) else "file differs"
    if kind == "encode_batch":  # mixed geometry: the equal neighbours share launches
        shapes = [(h, w), (h, w), (max(1, h // 2), w + 3), (h, w)]
        imgs = [pixels(seed + i, 1, hh, ww, mv, content)[0] for i, (hh, ww) in enumerate(shapes)]
        outs = enc.encode_batch([dmmt_jpeg.Image.from_array(a, mv) for a in imgs], o)
        for i, (a, out) in enumerate(zip(imgs, outs)):
            if out != oracle.encode(a, mv, sub, luma, chroma, restart_interval=ri):
                return f"file {i} of the batch differs"
        return None
    if kind == "forward_blocks":
        rgb = pixels(seed, 1, h, w, mv, content)[0]
        got = enc.forward_blocks(dmmt_jpeg.Image.from_array(rgb, mv), o)
        want = oracle.forward(rgb, mv, sub, luma, chroma)
        return None if got.shape == want.shape and np.array_equal(got, want) else "blocks differ"
    if kind == "encode_coefficients":
        coef = oracle.forward(pixels(seed, 1, h, w, 255, content)[0], 255, sub, luma, chroma)
        got = enc.encode_coefficients(coef, w, h, o)
        want = oracle.encode_coefficients(coef, w, h, sub, luma, chroma, restart_interval=ri)
        return None if got == want else "file differs"
    if kind == "dct_transform":
        blocks = np.random.default_rng(seed).uniform(-128, 127, (max(1, (w * h) // 64), 64)).astype(np.float32)
        got = enc.dct_transform(blocks)
        want = np.stack([oracle.dct_block(b) for b in blocks])
        return None if np.array_equal(got.view(np.uint32), want.view(np.uint32)) else "coefficients differ"
    if kind == "read_ppm_device":
        pmv = 255 if seed % 2 else 1000
        data = p3_text(pixels(seed, 1, h, w, pmv, content)[0], pmv, seed)
        got = enc.read_ppm_device(data)
        want = dmmt_jpeg.PPMImageReader(data).read_image()
        same = (got.width, got.height, got.maxval) == (want.width, want.height, want.maxval) and \
            np.array_equal(got.samples, want.samples)
        return None if same else "samples differ from the host reader's"
    if kind == "convert_ppm_batch":
        return _convert_batch(enc, s, o)
    if kind == "encode_gray":
        if seed % 2:
            g, gmv, transfer = pixels(seed, 1, h, w, 4095, content)[0, :, :, 0], 4095, GrayTransfer.AS_RGB
        else:
            g, gmv, transfer = pixels(seed, 1, h, w, 255, content)[0, :, :, 0], 255, GrayTransfer.Y_FULL_RANGE
        got = enc.encode_gray(g, gmv, o, transfer)
        return None if got == gray_ref.encode(g, gmv, luma, int(transfer), ri) else "file differs"
    if kind == "encode_ycc":
        y, cb, cr = Job._ycc_planes(seed, w, h, sub, content)
        if seed % 2:
            got = enc.encode_ycc(y, cb=cb, cr=cr, options=o)
        else:
            got = enc.encode_ycc(y, uv=np.stack([cb, cr], axis=2), options=o)
        return None if got == ycc_ref.encode(y, cb, cr, sub, luma, chroma, ri) else "file differs"
    raise ValueError(kind)


def _convert_batch(enc, s, o):
    """dmmt_convert_ppm_device_batch of three files: a P3 file, a P6 file and a P3 file
    with one sample above its maxval (its code, and a size of zero)"""
    w, h, sub, seed = s["w"], s["h"], s["sub"], s["seed"]
    a = pixels(seed, 1, h, w, 255, s.get("content", "noise"))[0]
    b = pixels(seed + 1, 1, max(1, h // 2), w + 1, 255)[0]
    c = pixels(seed + 2, 1, 5, 9, 200)[0]
    c[2, 3, 1] = 250
    datas = [p3_text(a, 255, seed), b"P6 %d %d 255\n" % (b.shape[1], b.shape[0]) + b.tobytes(), p3_text(c, 200, seed)]
    want = [(0, a, 255), (0, b, 255), (-100, c, 200)]  # -100: DMMT_E_VALUE_EXCEEDS_MAX
    allocs, files = [], []
    try:
        for data in datas:
            hdr = dmmt_jpeg.parse_ppm_header(data)
            cap = dmmt_jpeg.max_jpeg_bytes(hdr.width, hdr.height, sub)
            d_text, d_out, d_len = enc.malloc(len(data)), enc.malloc(cap), enc.malloc(4)
            allocs += [d_text, d_out, d_len]
            enc.h2d(d_text, np.frombuffer(data, np.uint8))
            enc.h2d(d_len, np.array([0xFFFFFFFF], np.uint32))
            files.append((d_text, len(data), hdr, d_out, cap, d_len))
        codes = enc.convert_ppm_device_batch(files, o, check=False)
        if codes != [code for code, _, _ in want]:
            return f"per-file codes {codes}"
        for i, ((_, _, _, d_out, cap, d_len), (code, rgb, mv)) in enumerate(zip(files, want)):
            size = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
            if code:
                if size != 0:
                    return f"file {i} failed and has size {size}"
            elif enc.d2h(d_out, min(size, cap)) != oracle.encode(rgb, mv, sub, o.luma_table, o.chroma_table,
                                                               restart_interval=o.restart_interval):
                return f"file {i} differs"
        return None
    finally:
        for p in allocs:
            enc.free(p)


# ------------------------------------------------------------------ the stripe protocol on one context

def stripe_options(w, sub, q, joined, rows_per_interval=1):
    return options(sub, q, 0 if joined else -(-w // MCU_W[sub]) * rows_per_interval)


class Stripes:
    """An image cut into MCU-row stripes, each stripe's rows and output buffer in
    device memory of one context"""

    def __init__(self, enc, rgb, sub, opts, n_stripes, rows_per_interval=1):
        self.enc, self.opts = enc, opts
        h, w, _ = rgb.shape
        mcuy = -(-h // MCU_H[sub])
        self.items, self.bufs = [], []
        for r in range(n_stripes):
            row0, rows = dmmt_jpeg.stripe_rows(mcuy, n_stripes, r, rows_per_interval)
            px = np.ascontiguousarray(rgb[row0 * MCU_H[sub]:min((row0 + rows) * MCU_H[sub], h)])
            d_in = enc.malloc(px.nbytes)
            self.bufs.append(d_in)
            enc.h2d(d_in, px)
            st = enc.stripe(d_in, w, h, row0, rows)
            cap = enc.stripe_max_bytes(st, opts)
            d_out = enc.malloc(cap)
            self.bufs.append(d_out)
            self.items.append((st, d_out, cap))

    def free(self):
        for d in self.bufs:
            self.enc.free(d)
        self.bufs = []


def striped_file(enc, rgb, sub, q, n_stripes, joined, rows_per_interval=1, between=lambda: None):
    """The whole stripe protocol on ONE context, which holds one analysed stripe at a
    time: a first pass of dmmt_stripe_analyze over the stripes for the histograms (and
    the edge DCs), then every stripe analysed again and taken through its later steps.
    between() runs between any two steps of one stripe.  Returns (file, options)."""
    o = stripe_options(rgb.shape[1], sub, q, joined, rows_per_interval)
    S = Stripes(enc, rgb, sub, o, n_stripes, rows_per_interval)
    try:
        parts = []
        if not joined:
            total = np.zeros(dmmt_jpeg.STRIPE_HIST_WORDS, np.uint64)
            for st, _, _ in S.items:
                total += enc.stripe_analyze(st, o)
            for st, d_out, cap in S.items:
                enc.stripe_analyze(st, o)
                between()
                parts.append(enc.d2h(d_out, enc.stripe_encode(total, d_out, cap)))
            return b"".join(parts), o
        hists, edges = [], []
        for st, _, _ in S.items:
            hists.append(enc.stripe_analyze(st, o))
            between()
            edges.append(enc.stripe_dc_edges())
        prevs = [[0, 0, 0]] + [edges[r - 1][1] for r in range(1, n_stripes)]
        total = np.zeros(dmmt_jpeg.STRIPE_HIST_WORDS, np.uint64)
        for r in range(n_stripes):
            total += dmmt_jpeg.Encoder.stripe_fix_dc_hist(hists[r], edges[r][0], prevs[r]) if r else hists[r]
        heads = []
        for r, (st, d_out, cap) in enumerate(S.items):
            enc.stripe_analyze(st, o)
            between()
            heads.append(enc.stripe_measure(total, prevs[r], d_out, cap))
        bits, f16 = [b for b, _ in heads], [f for _, f in heads]
        for r, (st, d_out, cap) in enumerate(S.items):
            enc.stripe_analyze(st, o)
            between()
            enc.stripe_measure(total, prevs[r], d_out, cap)
            between()
            parts.append(enc.d2h(d_out, enc.stripe_write(*dmmt_jpeg.stripe_seam(bits, f16, r))))
        return b"".join(parts), o
    finally:
        S.free()


def invalidated_stripe(enc, rgb, sub, q, mode, x):
    """dmmt_stripe_analyze of the image's first stripe (of two), x() -- a call that
    encodes or transforms on the same context --, then the stripe's next step for
    `mode` (STRIPE_MODES), every argument of which is valid: it must return
    DMMT_E_INVALID_ARGUMENT, before any launch.  None, or what happened instead."""
    joined = mode != "restart"
    o = stripe_options(rgb.shape[1], sub, q, joined)
    S = Stripes(enc, rgb, sub, o, 2)
    try:
        st, d_out, cap = S.items[0]
        hist = enc.stripe_analyze(st, o)
        if mode == "joined_write":
            enc.stripe_measure(hist, [0, 0, 0], d_out, cap)
        x()
        step = {"restart": lambda: enc.stripe_encode(hist, d_out, cap), "joined_edges": enc.stripe_dc_edges,
                "joined_measure": lambda: enc.stripe_measure(hist, [0, 0, 0], d_out, cap),
                "joined_write": lambda: enc.stripe_write(0, 0, 0)}[mode]
        try:
            step()
        except dmmt_jpeg.Error as e:
            return None if e.code == INVALID_ARGUMENT else f"code {e.code}"
        return "the stripe step ran on an invalidated stripe"
    finally:
        S.free()


def invalidator(enc, name, seed, job=None):
    """x for invalidated_stripe: INVALIDATORS by name, on images of sizes other than the
    stripe's; "encode_device" submits `job`"""
    o = options(seed % 3, QUALITIES[seed % 4])

    def run():
        if name == "encode_device":
            job.submit(None)
            return
        if name == "encode_gray":
            enc.encode_gray(pixels(seed, 1, 20, 28, 255)[0, :, :, 0], 255, o)
            return
        w, h = (24, 16) if name == "encode_small" else (200, 136) if name == "encode_large" else (56, 40)
        rgb = pixels(seed, 1, h, w, 255)[0]
        if name in ("encode_small", "encode_large"):
            enc.encode(dmmt_jpeg.Image.from_array(rgb), o)
        elif name == "forward_blocks":
            enc.forward_blocks(dmmt_jpeg.Image.from_array(rgb), o)
        elif name == "encode_coefficients":
            coef = oracle.forward(rgb, 255, int(o.chroma_subsampling_preset), o.luma_table, o.chroma_table)
            enc.encode_coefficients(coef, w, h, o)
        else:
            raise ValueError(name)
    return run


# ------------------------------------------------------------------ the schedule and the sweep

def draw_schedule(steps: int, seed: int, max_side: int = 96):
    """The steps of a sweep, from the seed alone (no GPU, no library).  Each step: op
    (a kind of ALL_KINDS) with its geometry, tables, restart interval, frame count,
    content and stream, and in_flight: the asynchronous calls enqueued and not yet
    synchronised when the step has made its own enqueue (0 after a step that
    synchronises the device: synchronize, set_lanes, encode_gray, encode_ycc and
    convert_ppm_batch do)."""
    rng = np.random.default_rng(seed)
    sched, unchecked, in_flight = [], 0, 0
    for i in range(steps):
        big = rng.random() < 0.25
        s = dict(step=i, seed=int(rng.integers(1, 1 << 30)),
                 w=int(rng.integers(1, (max_side if big else 40) + 1)),
                 h=int(rng.integers(1, (max_side if big else 40) + 1)),
                 sub=int(rng.integers(0, 3)), q=int(QUALITIES[int(rng.integers(0, len(QUALITIES)))]),
                 ri=int((0, 0, 1, 7, int(rng.integers(2, 40)))[int(rng.integers(0, 5))]),
                 n=int((1, 1, 3, 2)[int(rng.integers(0, 4))]),
                 content=("noise", "synthetic")[int(rng.integers(0, 2))],
                 stream=int((0, 0, 0, 1, 2)[int(rng.integers(0, 5))]), lanes=int(rng.integers(1, 5)),
                 x=INVALIDATORS[int(rng.integers(0, len(INVALIDATORS)))],
                 mode=STRIPE_MODES[int(rng.integers(0, len(STRIPE_MODES)))])
        r, pick = rng.random(), rng.random()
        if unchecked >= MAX_OUTSTANDING or r < 0.07:
            s["kind"] = "synchronize"
        elif r < 0.12:
            s["kind"] = "set_lanes"
        elif r < 0.16:
            s["kind"] = "bad_maxval"
        elif r < 0.60:
            s["kind"] = ASYNC_KINDS[int(pick * len(ASYNC_KINDS))]
        elif r < 0.86:
            s["kind"] = SYNC_KINDS[int(pick * len(SYNC_KINDS))]
        else:
            s["kind"] = STRIPE_KINDS[int(pick * len(STRIPE_KINDS))]
        kind = s["kind"]
        enqueues = kind in ASYNC_KINDS or kind == "bad_maxval" or (kind == "stripe_invalidated" and
                                                                  s["x"] == "encode_device")
        if enqueues:
            unchecked += 1
            in_flight += 1
        s["in_flight"] = in_flight
        if kind in ("synchronize", "set_lanes"):
            unchecked = in_flight = 0
        elif kind in ("encode_gray", "encode_ycc", "convert_ppm_batch"):
            in_flight = 0
        sched.append(s)
    return sched


def schedule_summary(sched):
    """how often every kind occurs, and the steps that ran among two or more calls in flight"""
    counts = {k: 0 for k in ALL_KINDS}
    for s in sched:
        counts[s["kind"]] += 1
    busy = sum(1 for s in sched if s["kind"] not in ("synchronize", "set_lanes") and s["in_flight"] >= 2)
    return {"counts": counts, "steps_with_two_in_flight": busy}


class _Sweep:
    def __init__(self):
        self.enc = dmmt_jpeg.Encoder(0)
        self.jobs = []
        self.bad_pending = False
        self.streams = None

    def stream(self, k):
        if not k:
            return None
        if self.streams is None:
            import torch
            self.streams = [torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)]
        return self.streams[k - 1].cuda_stream

    def raised_once(self, call):
        """call() with the pending bad call's error allowed to surface in it, once: the
        result of the clean repeat then"""
        try:
            return call(), None
        except dmmt_jpeg.Error as e:
            if not (self.bad_pending and e.name == "ValueExceedsMax"):
                return None, f"{e}"
            self.bad_pending = False
        try:
            return call(), None
        except dmmt_jpeg.Error as e:
            return None, f"raised again: {e}"

    def drain(self):
        """synchronize (the pending error exactly once), then check and free everything outstanding"""
        _, err = self.raised_once(self.enc.synchronize)
        if err:
            return err
        if self.bad_pending:
            return "the bad call's error was never raised"
        for job in self.jobs:
            bad = None if job.bad else job.mismatch()
            if bad:
                return bad
        for job in self.jobs:
            job.free()
        self.jobs = []
        return None

    def enqueue(self, s, **over):
        job = Job(self.enc, {**s, **over})
        self.jobs.append(job)
        return job

    def step(self, s):
        kind, enc = s["kind"], self.enc
        if kind == "synchronize":
            return self.drain()
        if kind == "set_lanes":
            err = self.drain()
            enc.set_lanes(s["lanes"])
            return err
        if kind == "bad_maxval":
            self.enqueue(s, kind="rgb_u8", content="noise", bad=True, w=max(s["w"], 4)).submit(self.stream(s["stream"]))
            self.bad_pending = True
            return None
        if kind in ASYNC_KINDS:
            self.enqueue(s).submit(self.stream(s["stream"]))
            return None
        if kind in ("encode_gray", "encode_ycc"):  # (they synchronise the context themselves)
            res, err = self.raised_once(lambda: sync_op(enc, s))
            return err or res
        if kind in SYNC_KINDS:
            return sync_op(enc, s)
        rgb = pixels(s["seed"], 1, max(s["h"], 2 * MCU_H[s["sub"]]), s["w"], 255, s["content"])[0]
        if kind == "stripe_invalidated":
            job = self.enqueue(s, kind="rgb_u8") if s["x"] == "encode_device" else None
            x = invalidator(enc, s["x"], s["seed"], job)
            if s["x"] == "encode_gray":  # (it synchronises the context itself)
                inner = x
                x = lambda: self.raised_once(inner)  # noqa: E731
            return invalidated_stripe(enc, rgb, s["sub"], s["q"], s["mode"], x)
        mcuy = -(-rgb.shape[0] // MCU_H[s["sub"]])
        n_stripes = 1 + s["seed"] % min(mcuy, 4)

        def benign():
            d = enc.malloc(24 * 16 * 3)
            enc.fill_synthetic(d, 24, 16, 1)
            enc.h2d(d, np.frombuffer(enc.d2h(d, 64), np.uint8))
            enc.free(d)
        data, o = striped_file(enc, rgb, s["sub"], s["q"], n_stripes, kind == "stripe_joined", between=benign)
        want = oracle.encode(rgb, 255, s["sub"], o.luma_table, o.chroma_table, restart_interval=o.restart_interval)
        return None if data == want else "the stripes' file differs"


def run(steps: int, seed: int, max_side: int = 96, minutes: float = 0, log=print):
    """The sweep; returns its summary dict (the count of every kind that ran, the
    steps that ran with two or more calls in flight), or the failing step under
    "mismatch"."""
    sched = draw_schedule(steps, seed, max_side)
    sweep = _Sweep()
    t0 = time.time()
    done = []
    try:
        for s in sched:
            if minutes and time.time() - t0 > 60 * minutes:
                break
            err = sweep.step(s)
            if err:
                return {"mismatch": dict(s, what=err)}
            done.append(s)
            if len(done) % 250 == 0:
                log(json.dumps({"steps": len(done), "seconds": round(time.time() - t0, 1),
                                **schedule_summary(done)}))
        err = sweep.drain()
        if err:
            return {"mismatch": dict(step="final synchronize", what=err)}
    finally:
        sweep.enc.close()
    return {"summary": "every output identical to its CPU reference", "steps": len(done), "seed": seed,
            "seconds": round(time.time() - t0, 1), **schedule_summary(done)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--minutes", type=float, default=0, help="stop early after this long (0 = no limit)")
    ap.add_argument("--max-side", type=int, default=96)
    a = ap.parse_args()
    res = run(a.steps, a.seed, a.max_side, a.minutes, log=lambda line: print(line, flush=True))
    print(json.dumps(res), flush=True)
    sys.exit(1 if "mismatch" in res else 0)


if __name__ == "__main__":
    main()
