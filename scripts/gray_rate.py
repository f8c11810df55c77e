#!/usr/bin/env python3
"""Encode rate of grayscale device frames (dmmt_encode_device_gray, both transfers)
against the colour entry point on the same pictures replicated to R,G,B at 4:4:4.

Frames are resident in HBM: 4 distinct one-channel uint8 frames (the green channel
of the synthetic generator's pictures) and the same pictures replicated to tight
R,G,B, made once by torch before anything is timed.  One configuration: 4K, IJG
quality 90.  A gray frame has a third of the control's blocks and a third of its
input bytes.
  one lane    everything on one torch stream handed to the library; ms per frame
              from device events around `--frames` encodes, after a warm-up of
              the same shape
  four lanes  NULL stream, round-robin over four lanes; the lanes' streams are the
              library's own, so the window is host-timed from the first enqueue to
              dmmt_ctx_synchronize
The variants alternate within a cycle, the control (dmmt_encode_device, tight
R,G,B, P444) runs first and last in every cycle -- its first-to-last spread is the
noise floor -- and the last frame of every variant is compared with the bytes of
the CPU yardstick (tests/gray_ref.py; the control's with the oracle's).

  python scripts/gray_rate.py --out profiles/gray_rate.json
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
import gray_ref  # noqa: E402
import oracle  # noqa: E402
from dmmt_jpeg import GrayTransfer as GT  # noqa: E402

CONFIGS = {"4kq90": (3840, 2160, 90)}
NSLOTS = 4
VARIANTS = {"gray_as_rgb": GT.AS_RGB, "gray_y_full_range": GT.Y_FULL_RANGE}


def run_config(enc, name, frames, warmup, cycles, dev):
    w, h, quality = CONFIGS[name]
    luma, chroma = dmmt_jpeg.quality_tables(quality)
    opt_c = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(0), 8, luma_table=luma,
                                                chroma_table=chroma).to_c()
    cap = (dmmt_jpeg.max_jpeg_bytes(w, h, 0) + 255) // 256 * 256  # (covers the gray bound)
    gray, tight = [], []
    for k in range(NSLOTS):
        t = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        enc.fill_synthetic(t.data_ptr(), w, h, 1, first_frame=500 + k)
        enc.synchronize()
        g = t[:, :, 1].contiguous()
        gray.append(g)
        tight.append(g[:, :, None].expand(h, w, 3).contiguous())
    torch.cuda.synchronize()
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4)]
    lens = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(4)]
    ts = torch.cuda.Stream(dev)

    # device pointers, taken once: the four-lane window is host-timed and short frames are bound by the enqueue
    p_out, p_len = [t.data_ptr() for t in outs], [t.data_ptr() for t in lens]
    p_tight, p_gray = [t.data_ptr() for t in tight], [t.data_ptr() for t in gray]

    def encode(vname, i, stream):
        o, n = p_out[i % 4], p_len[i % 4]
        if vname == "rgb444_control":
            enc.encode_device(p_tight[i % NSLOTS], 1, w, h, None, o, cap, n, frame_stride=w * h * 3, stream=stream,
                              opt_c=opt_c)
        else:
            enc.encode_device_gray(p_gray[i % NSLOTS], w, 1, w, h, None, o, cap, n, transfer=VARIANTS[vname],
                                   stream=stream, opt_c=opt_c)

    last = (frames - 1) % NSLOTS
    g_last = gray[last].cpu().numpy()
    want = {"rgb444_control": oracle.encode(tight[last].cpu().numpy(), 255, 0, luma, chroma, threads=8)}
    for v, tr in VARIANTS.items():
        want[v] = gray_ref.encode(g_last, 255, luma, int(tr))
        print(f"# yardstick {v}: {len(want[v])} bytes", flush=True)

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
            add(mode, "rgb444_control/first", fn("rgb444_control"))
            check("rgb444_control", mode)
            for v in VARIANTS:
                add(mode, v, fn(v))
                check(v, mode)
            add(mode, "rgb444_control/last", fn("rgb444_control"))
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

    stages = {"rgb444_control/first": stage_us("rgb444_control")}
    for v in VARIANTS:
        stages[v] = stage_us(v)
    stages["rgb444_control/last"] = stage_us("rgb444_control")
    out = {"width": w, "height": h, "quality": quality, "frames": frames, "warmup": warmup, "cycles": cycles,
           "jpeg_bytes_last_frame": {k: len(v) for k, v in want.items()},
           "input_bytes_per_frame": {"rgb444_control": w * h * 3, **{v: w * h for v in VARIANTS}},
           "blocks_per_frame": {"rgb444_control": 3 * (w // 8) * (h // 8), **{v: (w // 8) * (h // 8) for v in VARIANTS}}}
    for mode in res:
        out[mode] = {k: {"ms_per_frame_median": round(statistics.median(v), 5), "min": round(min(v), 5),
                         "max": round(max(v), 5)} for k, v in res[mode].items()}
        ctl = res[mode]["rgb444_control/first"] + res[mode]["rgb444_control/last"]
        out[mode]["control_spread_ms"] = round(max(ctl) - min(ctl), 5)
        for v in VARIANTS:
            out[mode][v]["ratio_to_control_median"] = round(statistics.median(res[mode][v]) / statistics.median(ctl), 4)
    out["stage_us_per_launch"] = stages
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gray_rate.json"))
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
