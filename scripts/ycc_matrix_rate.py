#!/usr/bin/env python3
"""Encode rate of BT.709 YCbCr device frames taken to the JFIF matrix on the way
(dmmt_encode_device_ycc_matrix: 8-bit limited-range NV12 and P010 limited range, each
with DMMT_YCC_MATRIX_BT709) against the same planes written as they are (JFIF: the
existing levels kernel), and against what a caller without the call does: a torch
repack of BT.709 limited-range NV12 to BT.601 full-range NV12 followed by
dmmt_encode_device_ycc.

Frames are resident in HBM: 4 distinct synthetic RGB frames converted once by torch,
before anything is timed, to float full-range BT.709 YCbCr with box-averaged 4:2:0
chroma and from there quantised to each variant's levels.  Per configuration (4K and
1080p, 4:2:0, q75):
  one lane    everything on one torch stream handed to the library; ms per frame
              from device events around `--frames` encodes, after a warm-up of
              the same shape
  four lanes  NULL stream, round-robin over four lanes; the lanes' streams are the
              library's own, so the window is host-timed from the first enqueue to
              dmmt_ctx_synchronize (the repack variant runs on one lane only: its
              torch kernels need the caller's stream)
The variants alternate within a cycle, each variant's control -- its own planes with
JFIF -- runs first and last in every cycle: its first-to-last spread is the noise
floor beside which the ratio variant / control is reported.  The last frame of every
variant is compared with the bytes of the CPU yardstick (tests/ycc_matrix_ref.py).

  python scripts/ycc_matrix_rate.py --out profiles/ycc_matrix_rate.json
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
import ycc_levels_ref as lv  # noqa: E402
import ycc_matrix_ref as mx  # noqa: E402
from dmmt_jpeg import DmmtYccLevels  # noqa: E402
from dmmt_jpeg import YccFormat as YF  # noqa: E402
from dmmt_jpeg import YccMatrix as M  # noqa: E402
from dmmt_jpeg import YccRange as R  # noqa: E402

CONFIGS = {"4k420q75": (3840, 2160, 2, 75), "1080p420q75": (1920, 1080, 2, 75)}
NSLOTS = 4
# name: (format, bit_depth, shift, range, sample_bytes); `name`_709 is the variant, `name`_jfif its control
PLANES = {"nv12_limited_u8": (YF.NV, 8, 0, R.LIMITED, 1), "p010_limited": (YF.NV, 10, 6, R.LIMITED, 2)}
VARIANTS = {p + "_709": p for p in PLANES}
CONTROLS = {p + "_jfif": p for p in PLANES}
REPACK = "nv12_limited_u8_torch_matrix_repack_then_ycc"


def float_ycc420(t):
    """(H, W, 3) uint8 R,G,B on the device -> float full-range BT.709 (y, cb, cr) in 0..255, chroma box-averaged 2 x 2"""
    f = t.to(torch.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.2126 * r + 0.7152 * g + 0.0722 * b
    cb = 128.0 + (b - y) / 1.8556
    cr = 128.0 + (r - y) / 1.5748

    def sub(p):
        return (p[0::2, 0::2] + p[1::2, 0::2] + p[0::2, 1::2] + p[1::2, 1::2]) / 4.0
    return y, sub(cb), sub(cr)


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


def repack_matrix(y8, uv8):
    """what a caller does today: BT.709 limited-range NV12 -> BT.601 full-range NV12, rounded to 8 bits"""
    a, b, c, d, e, f = (float(x) for x in mx.constants(mx.BT709))
    y = (y8.to(torch.float32) - 16.0) * (255.0 / 219.0) - 128.0
    ch = (uv8.to(torch.float32) - 128.0) * (255.0 / 224.0)
    cb, cr = ch[..., 0], ch[..., 1]
    up = lambda p: p.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)  # noqa: E731
    y = y + a * up(cb) + b * up(cr) + 128.0
    uv = torch.stack([c * cb + d * cr, e * cb + f * cr], dim=2) + 128.0
    return y.round().clamp(0, 255).to(torch.uint8), uv.round().clamp(0, 255).to(torch.uint8)


def run_config(enc, name, frames, warmup, cycles, dev):
    w, h, sub, quality = CONFIGS[name]
    assert sub == 2 and w % 2 == 0 and h % 2 == 0
    luma, chroma = dmmt_jpeg.quality_tables(quality)
    opt_c = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                                chroma_table=chroma).to_c()
    cap = (dmmt_jpeg.max_jpeg_bytes(w, h, sub) + 255) // 256 * 256
    levels = PLANES
    planes = {v: [] for v in levels}   # per variant and slot: the device planes as the call takes them
    planar = {v: [] for v in levels}   # ... and (y, cb, cr) for the yardstick
    for k in range(NSLOTS):
        # (torch may hand out a block that its queued kernels of the last slot still read: the
        # library fills it on a stream of its own, so torch's work is finished first)
        torch.cuda.synchronize()
        t = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        enc.fill_synthetic(t.data_ptr(), w, h, 1, first_frame=500 + k)
        enc.synchronize()
        f = float_ycc420(t)
        for v, (fmt, depth, shift, rng, sb) in levels.items():
            y, cb, cr = quantise(f, depth, shift, rng, sb)
            for q in (y, cb, cr):  # no code above the maximum, in any slot
                assert int(((q.to(torch.int32) & 0xFFFF) >> shift).max()) <= (1 << depth) - 1, (v, k)
            planar[v].append((y, cb, cr))
            planes[v].append([y, cb, cr] if fmt == YF.PLANAR else [y, torch.stack([cb, cr], dim=2).contiguous()])
    torch.cuda.synchronize()
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4)]
    lens = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(4)]
    tmp_y = torch.empty((h, w), dtype=torch.uint8, device=dev)
    tmp_uv = torch.empty((h // 2, w // 2, 2), dtype=torch.uint8, device=dev)
    ts = torch.cuda.Stream(dev)

    # device pointers, taken once: the four-lane window is host-timed and short frames are bound by the enqueue
    p_out, p_len = [t.data_ptr() for t in outs], [t.data_ptr() for t in lens]
    ptrs = {v: [[p.data_ptr() for p in f] for f in planes[v]] for v in levels}
    c_levels = {v: DmmtYccLevels(int(rng), depth, sb, shift) for v, (_, depth, shift, rng, sb) in PLANES.items()}

    def encode(vname, i, stream):
        o, n = p_out[i % 4], p_len[i % 4]
        if vname == REPACK:  # (on the caller's stream, which is torch's current one)
            y8, uv8 = repack_matrix(*planes["nv12_limited_u8"][i % NSLOTS])
            tmp_y.copy_(y8)
            tmp_uv.copy_(uv8)
            enc.encode_device_ycc([tmp_y.data_ptr(), tmp_uv.data_ptr()], YF.NV, w, w, 1, w, h, None, o, cap, n,
                                  stream=stream, opt_c=opt_c)
            return
        pl = VARIANTS.get(vname) or CONTROLS[vname]
        fmt, _, _, _, sb = levels[pl]
        cpitch = (w // 2) * sb * (1 if fmt == YF.PLANAR else 2)
        enc.encode_device_ycc(ptrs[pl][i % NSLOTS], fmt, w * sb, cpitch, 1, w, h, None, o, cap, n, stream=stream,
                              opt_c=opt_c, levels=c_levels[pl], matrix=M.BT709 if vname in VARIANTS else M.JFIF)

    last = (frames - 1) % NSLOTS
    want = {}
    for names, matrix in ((VARIANTS, mx.BT709), (CONTROLS, mx.JFIF)):
        for v, pl in names.items():
            _, depth, shift, rng, _ = levels[pl]
            want[v] = mx.encode(*[host(p) for p in planar[pl][last]], sub, luma, chroma, matrix, depth, shift, int(rng))
    y8, uv8 = repack_matrix(*planes["nv12_limited_u8"][last])
    want[REPACK] = lv.encode(y8.cpu().numpy(), uv8[..., 0].cpu().numpy(), uv8[..., 1].cpu().numpy(), sub, luma, chroma)

    def check(vname, label):
        n = int(lens[(frames - 1) % 4].item())
        got = outs[(frames - 1) % 4][:n].cpu().numpy().tobytes()
        if got != want[vname]:
            raise SystemExit(f"{name} {vname} {label}: the last frame differs from the CPU yardstick")

    def one_lane(vname):
        with torch.cuda.stream(ts):
            for i in range(warmup):
                encode(vname, i, ts.cuda_stream)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ts)
            for i in range(frames):
                encode(vname, i, ts.cuda_stream)
            b.record(ts)
        enc.synchronize()
        b.synchronize()
        return a.elapsed_time(b) / frames

    def four_lanes(vname):
        for i in range(warmup):
            encode(vname, i, None)
        enc.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            encode(vname, i, None)
        enc.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    res = {"one_lane": {}, "four_lanes": {}}

    def add(mode, key, ms):
        res[mode].setdefault(key, []).append(ms)

    def timed(mode, cycle, fn, vname):
        try:
            return fn(vname)
        except dmmt_jpeg.Error as e:
            raise SystemExit(f"{name} {vname} {mode} cycle {cycle}: {e}")

    for mode, lanes, fn in (("one_lane", 1, one_lane), ("four_lanes", 4, four_lanes)):
        enc.set_lanes(lanes)
        for cycle in range(cycles):
            for ctl in CONTROLS:
                add(mode, ctl + "/first", timed(mode, cycle, fn, ctl))
                check(ctl, mode)
            for v in list(VARIANTS) + ([REPACK] if lanes == 1 else []):
                add(mode, v, timed(mode, cycle, fn, v))
                check(v, mode)
            for ctl in CONTROLS:
                add(mode, ctl + "/last", timed(mode, cycle, fn, ctl))
    enc.set_lanes(1)

    def stage_us(vname):
        """us per launch of every stage (the library's event pairs around each kernel, one lane)"""
        for i in range(warmup):
            encode(vname, i, ts.cuda_stream)
        enc.synchronize()
        enc.set_profiling(True)
        for i in range(frames):
            encode(vname, i, ts.cuda_stream)
        enc.synchronize()
        prof = enc.profile()
        enc.set_profiling(False)
        return {k: round(1e3 * ms / n, 3) for k, (ms, n) in prof.items() if n}

    stages = {ctl + "/first": stage_us(ctl) for ctl in CONTROLS}
    for v in VARIANTS:
        stages[v] = stage_us(v)
    for ctl in CONTROLS:
        stages[ctl + "/last"] = stage_us(ctl)
    out = {"width": w, "height": h, "subsampling": "4:2:0", "quality": quality, "frames": frames, "warmup": warmup,
           "cycles": cycles, "jpeg_bytes_last_frame": {k: len(v) for k, v in want.items()},
           "input_bytes_per_frame": {v: w * h * 3 // 2 * levels[v][4] for v in levels}}
    for mode in res:
        out[mode] = {k: {"ms_per_frame_median": round(statistics.median(v), 5), "min": round(min(v), 5),
                         "max": round(max(v), 5)} for k, v in res[mode].items()}
        for v, pl in VARIANTS.items():  # the new path against its own planes written as they are
            ctl = res[mode][pl + "_jfif/first"] + res[mode][pl + "_jfif/last"]
            med = statistics.median(ctl)
            out[mode][v]["ratio_to_control"] = round(statistics.median(res[mode][v]) / med, 4)
            out[mode][v]["control_ms_median"] = round(med, 5)
            out[mode][v]["control_spread_ratio"] = round((max(ctl) - min(ctl)) / med, 4)
    out["stage_us_per_launch"] = stages
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ycc_matrix_rate.json"))
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
