#!/usr/bin/env python3
"""Encode rate of device surfaces against the tight-RGB entry point and against the
two-step baseline (a torch repack to tight R,G,B, then dmmt_encode_device) that a
caller needs without dmmt_encode_device_surfaces.

Frames are synthetic and resident in HBM (4 distinct frames per variant, used in
turn).  Per configuration (4K 4:4:4 q90, 1080p 4:2:0 q75):
  one lane    everything on one torch stream handed to the library; ms per frame
              from device events around `--frames` encodes, after a warm-up of
              the same shape
  four lanes  NULL stream, round-robin over four lanes; the lanes' streams are the
              library's own, so the window is host-timed from the first enqueue to
              dmmt_ctx_synchronize (direct variants and the control only: the
              repack of the two-step path cannot be ordered before a lane
              without a host synchronisation)
The variants alternate within a cycle, the control runs first and last in every
cycle (its spread is the noise floor), and the last frame of every variant is
compared with the oracle's bytes.

  python scripts/surface_rate.py --out profiles/surfaces_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dmmt-jpeg-encoder_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dmmt_jpeg  # noqa: E402
import oracle  # noqa: E402
from dmmt_jpeg import PixelFormat as PF  # noqa: E402

CONFIGS = {"4k444q90": (3840, 2160, 0, 90), "1080p420q75": (1920, 1080, 2, 75)}
NSLOTS = 4


def build_variants(enc, w, h, dev):
    """name -> (format, [surface tensors], repack to tight RGB or None)"""
    gen = torch.Generator(device=dev).manual_seed(1)
    tight = []
    for k in range(NSLOTS):
        t = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        enc.fill_synthetic(t.data_ptr(), w, h, 1, first_frame=500 + k)
        tight.append(t)
    enc.synchronize()

    def junk(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=gen)

    def pitched(t):
        buf = junk(h, w * 3 + 64)
        buf[:, :w * 3] = t.reshape(h, w * 3)
        return buf

    # the repacks: one torch kernel each, the cheapest form found for the layout -- a
    # strided copy into a preallocated tight frame, or flip() (B,G,R: torch has no
    # negative strides; its result is a fresh tight tensor from the caching allocator)
    v = {
        "rgb_tight_control": (None, tight, None),
        "rgb_pitch64": (PF.RGB, [pitched(t) for t in tight], lambda s, o: o.view(h, w * 3).copy_(s[:, :w * 3])),
        "bgr": (PF.BGR, [t.flip(2).contiguous() for t in tight], lambda s, o: s.flip(2)),
        "rgbx": (PF.RGBX, [torch.cat([t, junk(h, w, 1)], 2) for t in tight], lambda s, o: o.copy_(s[..., :3])),
        "bgrx": (PF.BGRX, [torch.cat([t.flip(2), junk(h, w, 1)], 2) for t in tight],
                 lambda s, o: s[..., :3].flip(2)),
        "planar": (PF.PLANAR, [t.permute(2, 0, 1).contiguous() for t in tight],
                   lambda s, o: o.copy_(s.permute(1, 2, 0))),
    }
    torch.cuda.synchronize()
    return v, tight


def surface_args(fmt, s, w, h):
    """(planes, row pitch) of a surface tensor"""
    if fmt == PF.PLANAR:
        return [s.data_ptr() + c * s.stride(0) for c in range(3)], s.stride(1)
    return s.data_ptr(), s.stride(0)


def run_config(enc, name, frames, warmup, cycles, dev):
    w, h, sub, quality = CONFIGS[name]
    luma, chroma = dmmt_jpeg.quality_tables(quality)
    opt_c = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                                chroma_table=chroma).to_c()
    cap = (dmmt_jpeg.max_jpeg_bytes(w, h, sub) + 255) // 256 * 256
    variants, tight = build_variants(enc, w, h, dev)
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4)]
    lens = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(4)]
    tmp = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(NSLOTS)]
    held = [None] * NSLOTS
    ts = torch.cuda.Stream(dev)

    def tight_encode(t, i, stream):
        enc.encode_device(t.data_ptr(), 1, w, h, None, outs[i % 4].data_ptr(), cap, lens[i % 4].data_ptr(),
                          frame_stride=w * h * 3, stream=stream, opt_c=opt_c)

    def direct(vname, i, stream):
        fmt, surf, _ = variants[vname]
        s = surf[i % NSLOTS]
        if fmt is None:
            return tight_encode(s, i, stream)
        planes, pitch = surface_args(fmt, s, w, h)
        enc.encode_device_surfaces(planes, fmt, pitch, 1, w, h, None, outs[i % 4].data_ptr(), cap,
                                   lens[i % 4].data_ptr(), stream=stream, opt_c=opt_c)

    def two_step(vname, i, stream):
        _, surf, repack = variants[vname]
        held[i % NSLOTS] = repack(surf[i % NSLOTS], tmp[i % NSLOTS])  # (kept alive until the slot's next turn)
        tight_encode(held[i % NSLOTS], i, stream)

    want = oracle.encode(tight[(frames - 1) % NSLOTS].cpu().numpy(), 255, sub, luma, chroma, threads=8)

    def check(label):
        n = int(lens[(frames - 1) % 4].item())
        got = outs[(frames - 1) % 4][:n].cpu().numpy().tobytes()
        if got != want:
            raise SystemExit(f"{name} {label}: the last frame differs from the oracle")

    def one_lane(fn, vname):
        with torch.cuda.stream(ts):
            for i in range(warmup):
                fn(vname, i, ts.cuda_stream)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ts)
            for i in range(frames):
                fn(vname, i, ts.cuda_stream)
            b.record(ts)
        enc.synchronize()
        b.synchronize()
        return a.elapsed_time(b) / frames

    def four_lanes(vname):
        for i in range(warmup):
            direct(vname, i, None)
        enc.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            direct(vname, i, None)
        enc.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    names = [n for n in variants if n != "rgb_tight_control"]
    res = {"one_lane": {}, "four_lanes": {}}

    def add(mode, key, ms):
        res[mode].setdefault(key, []).append(ms)

    enc.set_lanes(1)
    for _ in range(cycles):
        add("one_lane", "rgb_tight_control/first", one_lane(direct, "rgb_tight_control"))
        check("control")
        for n in names:
            add("one_lane", n + "/direct", one_lane(direct, n))
            check(n + " direct")
            add("one_lane", n + "/two_step", one_lane(two_step, n))
            check(n + " two-step")
        add("one_lane", "rgb_tight_control/last", one_lane(direct, "rgb_tight_control"))
    enc.set_lanes(4)
    for _ in range(cycles):
        add("four_lanes", "rgb_tight_control/first", four_lanes("rgb_tight_control"))
        for n in names:
            add("four_lanes", n + "/direct", four_lanes(n))
            check(n + " direct, four lanes")
        add("four_lanes", "rgb_tight_control/last", four_lanes("rgb_tight_control"))
    enc.set_lanes(1)
    out = {"width": w, "height": h, "subsampling": ["4:4:4", "4:2:2", "4:2:0"][sub], "quality": quality,
           "frames": frames, "warmup": warmup, "cycles": cycles, "jpeg_bytes_last_frame": len(want)}
    for mode in res:
        out[mode] = {k: {"ms_per_frame_median": round(statistics.median(v), 5), "min": round(min(v), 5),
                         "max": round(max(v), 5)} for k, v in res[mode].items()}
        ctl = res[mode]["rgb_tight_control/first"] + res[mode]["rgb_tight_control/last"]
        out[mode]["control_spread_ms"] = round(max(ctl) - min(ctl), 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfaces_rate.json"))
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
