#!/usr/bin/env python3
"""Encode rate of YCbCr device frames (dmmt_encode_device_ycc: NV12 and I420)
against the tight-RGB entry point at the same size, subsampling and tables.

Frames are resident in HBM: 4 distinct synthetic RGB frames (the control's input)
and the same pictures as full-range YCbCr with box-averaged 4:2:0 chroma, made
once by torch before anything is timed.  Per configuration (4K and 1080p, 4:2:0,
q75):
  one lane    everything on one torch stream handed to the library; ms per frame
              from device events around `--frames` encodes, after a warm-up of
              the same shape
  four lanes  NULL stream, round-robin over four lanes; the lanes' streams are the
              library's own, so the window is host-timed from the first enqueue to
              dmmt_ctx_synchronize
The variants alternate within a cycle, the control (dmmt_encode_device, tight
R,G,B, P420) runs first and last in every cycle -- its first-to-last spread is the
noise floor -- and the last frame of every variant is compared with the bytes of
the CPU yardstick (tests/ycc_ref.py; the control's with the oracle's).

  python scripts/ycc_rate.py --out profiles/ycc_rate.json
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
import oracle  # noqa: E402
import ycc_ref  # noqa: E402
from dmmt_jpeg import YccFormat as YF  # noqa: E402

CONFIGS = {"4k420q75": (3840, 2160, 2, 75), "1080p420q75": (1920, 1080, 2, 75)}
NSLOTS = 4


def to_ycc420(t):
    """(H, W, 3) uint8 R,G,B on the device -> full-range uint8 (y, cb, cr), chroma box-averaged 2 x 2"""
    f = t.to(torch.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = 128.0 - 0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 128.0 + 0.5 * r - 0.418688 * g - 0.081312 * b

    def sub(p):
        return (p[0::2, 0::2] + p[1::2, 0::2] + p[0::2, 1::2] + p[1::2, 1::2]) / 4.0

    def u8(p):
        return p.round().clamp(0, 255).to(torch.uint8).contiguous()
    return u8(y), u8(sub(cb)), u8(sub(cr))


def run_config(enc, name, frames, warmup, cycles, dev):
    w, h, sub, quality = CONFIGS[name]
    assert sub == 2 and w % 2 == 0 and h % 2 == 0
    luma, chroma = dmmt_jpeg.quality_tables(quality)
    opt_c = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                                chroma_table=chroma).to_c()
    cap = (dmmt_jpeg.max_jpeg_bytes(w, h, sub) + 255) // 256 * 256
    tight, i420, nv12 = [], [], []
    for k in range(NSLOTS):
        t = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        enc.fill_synthetic(t.data_ptr(), w, h, 1, first_frame=500 + k)
        enc.synchronize()
        tight.append(t)
        y, cb, cr = to_ycc420(t)
        i420.append((y, cb, cr))
        nv12.append((y, torch.stack([cb, cr], dim=2).contiguous()))
    torch.cuda.synchronize()
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4)]
    lens = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(4)]
    ts = torch.cuda.Stream(dev)

    # device pointers, taken once: the four-lane window is host-timed and short frames are bound by the enqueue
    p_out, p_len = [t.data_ptr() for t in outs], [t.data_ptr() for t in lens]
    p_tight = [t.data_ptr() for t in tight]
    p_i420 = [[p.data_ptr() for p in f] for f in i420]
    p_nv12 = [[p.data_ptr() for p in f] for f in nv12]

    def encode(vname, i, stream):
        o, n = p_out[i % 4], p_len[i % 4]
        if vname == "rgb_tight_control":
            enc.encode_device(p_tight[i % NSLOTS], 1, w, h, None, o, cap, n, frame_stride=w * h * 3, stream=stream,
                              opt_c=opt_c)
        elif vname == "i420":
            enc.encode_device_ycc(p_i420[i % NSLOTS], YF.PLANAR, w, w // 2, 1, w, h, None, o, cap, n, stream=stream,
                                  opt_c=opt_c)
        else:
            enc.encode_device_ycc(p_nv12[i % NSLOTS], YF.NV, w, w, 1, w, h, None, o, cap, n, stream=stream,
                                  opt_c=opt_c)

    last = (frames - 1) % NSLOTS
    want = {"rgb_tight_control": oracle.encode(tight[last].cpu().numpy(), 255, sub, luma, chroma, threads=8)}
    want["i420"] = want["nv12"] = ycc_ref.encode(*[p.cpu().numpy() for p in i420[last]], sub, luma, chroma)

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

    for mode, lanes, fn in (("one_lane", 1, one_lane), ("four_lanes", 4, four_lanes)):
        enc.set_lanes(lanes)
        for _ in range(cycles):
            add(mode, "rgb_tight_control/first", fn("rgb_tight_control"))
            check("rgb_tight_control", mode)
            for v in ("nv12", "i420"):
                add(mode, v, fn(v))
                check(v, mode)
            add(mode, "rgb_tight_control/last", fn("rgb_tight_control"))
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

    stages = {"rgb_tight_control/first": stage_us("rgb_tight_control"), "nv12": stage_us("nv12"),
              "i420": stage_us("i420"), "rgb_tight_control/last": stage_us("rgb_tight_control")}
    out = {"width": w, "height": h, "subsampling": "4:2:0", "quality": quality, "frames": frames, "warmup": warmup,
           "cycles": cycles, "jpeg_bytes_last_frame": {k: len(v) for k, v in want.items()},
           "input_bytes_per_frame": {"rgb_tight_control": w * h * 3, "nv12": w * h * 3 // 2, "i420": w * h * 3 // 2}}
    for mode in res:
        out[mode] = {k: {"ms_per_frame_median": round(statistics.median(v), 5), "min": round(min(v), 5),
                         "max": round(max(v), 5)} for k, v in res[mode].items()}
        ctl = res[mode]["rgb_tight_control/first"] + res[mode]["rgb_tight_control/last"]
        out[mode]["control_spread_ms"] = round(max(ctl) - min(ctl), 5)
    out["stage_us_per_launch"] = stages
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ycc_rate.json"))
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
