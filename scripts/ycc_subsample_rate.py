#!/usr/bin/env python3
"""Encode rate of YCbCr device frames whose chroma planes are finer than the file
(dmmt_encode_device_ycc_subsample), file 4:2:0:
  i444_u8         planar 4:4:4 uint8 full range (I444)
  nv16_u8         4:2:2 uint8 full range, a plane of Cb,Cr pairs (NV16)
  p210_709        4:2:2, 10 bits at the top of a uint16, limited range, BT.709 (P210)
each against two things timed in the same run:
  control   the existing call at 4:2:0 on planes averaged beforehand (I420, NV12, P010 +
            BT.709): the parent's kernel, which reads 1.5 bytes per pixel where the
            converting kernel reads 3 (4:4:4) or 2 (4:2:2);
  repack    what a caller does today: a torch pass that averages the chroma to NV12 --
            for P210 to 8-bit BT.601 full range -- followed by dmmt_encode_device_ycc.

Frames are resident in HBM: 4 distinct synthetic RGB frames converted once by torch,
before anything is timed.  Per configuration (4K and 1080p, q75):
  one lane    everything on one torch stream handed to the library; ms per frame from
              device events around `--frames` encodes, after a warm-up of the same shape
  four lanes  NULL stream, round-robin over four lanes; host-timed from the first enqueue
              to dmmt_ctx_synchronize (the repack runs on one lane only: its torch
              kernels need the caller's stream)
The variants alternate within a cycle; each variant's control runs first and last in
every cycle: its first-to-last spread is the noise floor beside which the ratio variant /
control is reported.  The last frame of every variant, control and repack is compared
with the bytes of the CPU yardsticks (tests/ycc_subsample_ref.py, tests/ycc_matrix_ref.py).

  python scripts/ycc_subsample_rate.py --out profiles/ycc_subsample_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dmmt-jpeg-encoder_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402

import dmmt_jpeg  # noqa: E402
import ycc_matrix_ref as mx  # noqa: E402
import ycc_subsample_ref as ss  # noqa: E402
from dmmt_jpeg import DmmtYccLevels  # noqa: E402
from dmmt_jpeg import YccFormat as YF  # noqa: E402
from dmmt_jpeg import YccMatrix as M  # noqa: E402
from dmmt_jpeg import YccRange as R  # noqa: E402

CONFIGS = {"4k_q75": (3840, 2160, 75), "1080p_q75": (1920, 1080, 75)}
NSLOTS = 4
SUB = 2  # the file
# name: (planes' sampling, format, bit_depth, shift, range, sample_bytes, matrix)
VARIANTS = {"i444_u8": (0, YF.PLANAR, 8, 0, R.FULL, 1, M.JFIF), "nv16_u8": (1, YF.NV, 8, 0, R.FULL, 1, M.JFIF),
            "p210_709": (1, YF.NV, 10, 6, R.LIMITED, 2, M.BT709)}


def float_ycc(t, matrix):
    """(H, W, 3) uint8 R,G,B on the device -> float full-range (y, cb, cr) in 0..255 at 4:4:4"""
    kr, kb = mx.KR_KB[int(matrix)]
    f = t.to(torch.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    return y, 128.0 + (b - y) / (2 * (1 - kb)), 128.0 + (r - y) / (2 * (1 - kr))


def down(p, rx, ry):
    """the float box average"""
    s = sum(p[yy::ry, xx::rx] for xx in range(rx) for yy in range(ry))
    return s / float(rx * ry)


def quantise(planes, depth, shift, rng, sb):
    """float full-range planes -> samples of the given levels (codes << shift)"""
    m = float(1 << (depth - 8))
    top = float((1 << depth) - 1)
    out = []
    for i, p in enumerate(planes):
        if rng == R.LIMITED:
            v = 16.0 * m + p * (219.0 * m / 255.0) if i == 0 else 128.0 * m + (p - 128.0) * (224.0 * m / 255.0)
        else:
            v = p * (top / 255.0) if i == 0 else float(1 << (depth - 1)) + (p - 128.0) * (top / 255.0)
        code = v.round().clamp(0, top).to(torch.int32) << shift
        # (uint16 samples are kept as the int16 of the same bits: torch's uint16 has few operators)
        out.append(code.to(torch.uint8).contiguous() if sb == 1 else code.to(torch.int16).contiguous())
    return out


def host(p):
    """a device plane as its numpy samples"""
    a = p.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def as_call(planar, fmt):
    y, cb, cr = planar
    return [y, cb, cr] if fmt == YF.PLANAR else [y, torch.stack([cb, cr], dim=2).contiguous()]


def repack(vname, pl):
    """what a caller does today: the planes of a variant -> 8-bit BT.601 full-range NV12 (y, uv)"""
    src, fmt, depth, shift, rng, sb, matrix = VARIANTS[vname]
    rx, ry = ss.ratios(src, SUB)
    if vname == "p210_709":
        a, b, c, d, e, f = (float(x) for x in mx.constants(mx.BT709))
        code = lambda q: ((q.to(torch.int32) & 0xFFFF) >> shift).to(torch.float32)  # noqa: E731
        y = (code(pl[0]) - 64.0) * (255.0 / 876.0) - 128.0
        ch = (code(pl[1]) - 512.0) * (255.0 / 896.0)
        cb, cr = ch[..., 0], ch[..., 1]
        y = y + a * cb.repeat_interleave(2, dim=1) + b * cr.repeat_interleave(2, dim=1) + 128.0
        uv = torch.stack([down(c * cb + d * cr, rx, ry), down(e * cb + f * cr, rx, ry)], dim=2) + 128.0
        return y.round().clamp(0, 255).to(torch.uint8), uv.round().clamp(0, 255).to(torch.uint8)
    if fmt == YF.PLANAR:
        cb, cr = pl[1].to(torch.float32), pl[2].to(torch.float32)
    else:
        cb, cr = pl[1][..., 0].to(torch.float32), pl[1][..., 1].to(torch.float32)
    uv = torch.stack([down(cb, rx, ry), down(cr, rx, ry)], dim=2)
    return pl[0], uv.round().clamp(0, 255).to(torch.uint8)


def run_config(enc, name, frames, warmup, cycles, dev):
    w, h, quality = CONFIGS[name]
    assert w % 2 == 0 and h % 2 == 0
    luma, chroma = dmmt_jpeg.quality_tables(quality)
    opt_c = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(SUB), 8, luma_table=luma,
                                                chroma_table=chroma).to_c()
    cap = (dmmt_jpeg.max_jpeg_bytes(w, h, SUB) + 255) // 256 * 256
    planes = {v: [] for v in VARIANTS}    # per variant and slot: the device planes as the call takes them
    planar = {v: [] for v in VARIANTS}    # ... and (y, cb, cr) for the yardstick
    cplanes = {v: [] for v in VARIANTS}   # the control's: averaged beforehand to 4:2:0
    cplanar = {v: [] for v in VARIANTS}
    for k in range(NSLOTS):
        torch.cuda.synchronize()  # (torch's queued kernels first: the library fills on a stream of its own)
        t = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        enc.fill_synthetic(t.data_ptr(), w, h, 1, first_frame=500 + k)
        enc.synchronize()
        for v, (src, fmt, depth, shift, rng, sb, matrix) in VARIANTS.items():
            y, cb, cr = float_ycc(t, matrix)
            shr = 1 if src == 0 else 2
            q = quantise((y, down(cb, shr, 1), down(cr, shr, 1)), depth, shift, rng, sb)
            q420 = quantise((y, down(cb, 2, 2), down(cr, 2, 2)), depth, shift, rng, sb)
            planar[v].append(q)
            planes[v].append(as_call(q, fmt))
            cplanar[v].append(q420)
            cplanes[v].append(as_call(q420, fmt))
    torch.cuda.synchronize()
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4)]
    lens = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(4)]
    tmp_uv = torch.empty((h // 2, w // 2, 2), dtype=torch.uint8, device=dev)
    tmp_y = torch.empty((h, w), dtype=torch.uint8, device=dev)
    ts = torch.cuda.Stream(dev)
    p_out, p_len = [t.data_ptr() for t in outs], [t.data_ptr() for t in lens]
    ptrs = {v: [[p.data_ptr() for p in f] for f in planes[v]] for v in VARIANTS}
    cptrs = {v: [[p.data_ptr() for p in f] for f in cplanes[v]] for v in VARIANTS}
    c_levels = {v: None if (sb == 1 and rng == R.FULL) else DmmtYccLevels(int(rng), depth, sb, shift)
                for v, (_, _, depth, shift, rng, sb, _) in VARIANTS.items()}

    def encode(kind, v, i, stream):
        """kind: "sub" the new call, "control" the existing call on 4:2:0 planes, "repack" torch then the plain call"""
        o, n = p_out[i % 4], p_len[i % 4]
        src, fmt, depth, shift, rng, sb, matrix = VARIANTS[v]
        per_pos = sb * (1 if fmt == YF.PLANAR else 2)
        if kind == "repack":  # (on the caller's stream, which is torch's current one)
            y8, uv8 = repack(v, planes[v][i % NSLOTS])
            tmp_uv.copy_(uv8)
            yp = y8.data_ptr()
            if v == "p210_709":
                tmp_y.copy_(y8)
                yp = tmp_y.data_ptr()
            enc.encode_device_ycc([yp, tmp_uv.data_ptr()], YF.NV, w, w, 1, w, h, None, o, cap, n, stream=stream,
                                  opt_c=opt_c)
        elif kind == "control":
            enc.encode_device_ycc(cptrs[v][i % NSLOTS], fmt, w * sb, (w // 2) * per_pos, 1, w, h, None, o, cap, n,
                                  stream=stream, opt_c=opt_c, levels=c_levels[v], matrix=matrix)
        else:
            cw = w if src == 0 else w // 2
            enc.encode_device_ycc(ptrs[v][i % NSLOTS], fmt, w * sb, cw * per_pos, 1, w, h, None, o, cap, n,
                                  stream=stream, opt_c=opt_c, levels=c_levels[v], matrix=matrix, chroma_sampling=src)

    last = (frames - 1) % NSLOTS
    want = {}
    for v, (src, fmt, depth, shift, rng, sb, matrix) in VARIANTS.items():
        want["sub", v] = ss.encode(*[host(p) for p in planar[v][last]], src, SUB, luma, chroma, int(matrix), depth,
                                   shift, int(rng))
        want["control", v] = mx.encode(*[host(p) for p in cplanar[v][last]], SUB, luma, chroma, int(matrix), depth,
                                       shift, int(rng))
        y8, uv8 = repack(v, planes[v][last])
        want["repack", v] = mx.encode(host(y8), host(uv8[..., 0]), host(uv8[..., 1]), SUB, luma, chroma, mx.JFIF)

    def check(kind, v, label):
        n = int(lens[(frames - 1) % 4].item())
        got = outs[(frames - 1) % 4][:n].cpu().numpy().tobytes()
        if got != want[kind, v]:
            raise SystemExit(f"{name} {kind} {v} {label}: the last frame differs from the CPU yardstick")

    def one_lane(kind, v):
        with torch.cuda.stream(ts):
            for i in range(warmup):
                encode(kind, v, i, ts.cuda_stream)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ts)
            for i in range(frames):
                encode(kind, v, i, ts.cuda_stream)
            b.record(ts)
        enc.synchronize()
        b.synchronize()
        return a.elapsed_time(b) / frames

    def four_lanes(kind, v):
        for i in range(warmup):
            encode(kind, v, i, None)
        enc.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            encode(kind, v, i, None)
        enc.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    res = {"one_lane": {}, "four_lanes": {}}

    def timed(mode, fn, kind, v, key):
        try:
            res[mode].setdefault(key, []).append(fn(kind, v))
        except dmmt_jpeg.Error as e:
            raise SystemExit(f"{name} {kind} {v} {mode}: {e}")
        check(kind, v, mode)

    for mode, lanes, fn in (("one_lane", 1, one_lane), ("four_lanes", 4, four_lanes)):
        enc.set_lanes(lanes)
        for cycle in range(cycles):
            for v in VARIANTS:
                timed(mode, fn, "control", v, v + "/control/first")
            for v in VARIANTS:
                timed(mode, fn, "sub", v, v + "/subsample")
                if lanes == 1:
                    timed(mode, fn, "repack", v, v + "/repack")
            for v in VARIANTS:
                timed(mode, fn, "control", v, v + "/control/last")
    enc.set_lanes(1)

    def stage_us(kind, v):
        """us per launch of every stage (the library's event pairs around each kernel, one lane)"""
        for i in range(warmup):
            encode(kind, v, i, ts.cuda_stream)
        enc.synchronize()
        enc.set_profiling(True)
        for i in range(frames):
            encode(kind, v, i, ts.cuda_stream)
        enc.synchronize()
        prof = enc.profile()
        enc.set_profiling(False)
        return {k: round(1e3 * ms / n, 3) for k, (ms, n) in prof.items() if n}

    stages = {}
    for v in VARIANTS:
        stages[v + "/control"] = stage_us("control", v)
        stages[v + "/subsample"] = stage_us("sub", v)
    out = {"width": w, "height": h, "file": "4:2:0", "quality": quality, "frames": frames, "warmup": warmup,
           "cycles": cycles, "jpeg_bytes_last_frame": {f"{v}/{k}": len(b) for (k, v), b in want.items()},
           "input_bytes_per_pixel": {v: (1 + (2 if src == 0 else 1)) * sb for v, (src, _, _, _, _, sb, _) in VARIANTS.items()}}
    for mode in res:
        out[mode] = {k: {"ms_per_frame_median": round(statistics.median(x), 5), "min": round(min(x), 5),
                         "max": round(max(x), 5)} for k, x in res[mode].items()}
        for v in VARIANTS:
            ctl = res[mode][v + "/control/first"] + res[mode][v + "/control/last"]
            med = statistics.median(ctl)
            e = out[mode][v + "/subsample"]
            e["ratio_to_control"] = round(statistics.median(res[mode][v + "/subsample"]) / med, 4)
            e["control_ms_median"] = round(med, 5)
            e["control_spread_ratio"] = round((max(ctl) - min(ctl)) / med, 4)
            if v + "/repack" in res[mode]:
                e["ratio_to_repack"] = round(statistics.median(res[mode][v + "/subsample"]) /
                                             statistics.median(res[mode][v + "/repack"]), 4)
    out["stage_us_per_launch"] = stages
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ycc_subsample_rate.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    enc = dmmt_jpeg.Encoder(0)
    result = {"device": torch.cuda.get_device_name(0), "build": dmmt_jpeg.lib().dmmt_build_info().decode(),
              "timing": "one lane: device events on the caller's stream; four lanes: host clock, enqueue to synchronize",
              "configs": {}}
    try:
        for name in args.configs.split(","):
            result["configs"][name] = run_config(enc, name, args.frames, args.warmup, args.cycles, dev)
            print(json.dumps({name: result["configs"][name]}), flush=True)
    finally:
        enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
