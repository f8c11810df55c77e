"""Where the narrow block form (csrc/coef_format.hpp) stops paying: us per frame of
pipelined device encodes at any size, quality (or all-ones tables) and frame content,
for the form DMMT_COEF_FORMAT names (read when the context is created -- one process
per form).  The last frame of the run is checked against the oracle when --check.
  DMMT_COEF_FORMAT=narrow python scripts/coef_format_rate.py --size 3840x2160 --sub 0 --quality 95
  --quality 0: all-ones tables;  --noise: full-range random frames instead of the synthetic ones
Prints one JSON line: the median and every run."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dmmt-jpeg-encoder_amd")]
import torch  # noqa: E402
import dmmt_jpeg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--sub", type=int, default=0)
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--noise", action="store_true")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--lanes", type=int, default=4)
ap.add_argument("--check", action="store_true")
args = ap.parse_args()
w, h = (int(x) for x in args.size.split("x"))
luma, chroma = dmmt_jpeg.quality_tables(args.quality) if args.quality else ([1] * 64, [1] * 64)
opts = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(args.sub), 8, luma_table=list(luma),
                                           chroma_table=list(chroma))
opt_c = opts.to_c()
out_stride = (dmmt_jpeg.max_jpeg_bytes(w, h, args.sub) + 255) // 256 * 256
enc = dmmt_jpeg.Encoder(0)
enc.set_lanes(args.lanes)
d_in = [enc.malloc(w * h * 3) for _ in range(4)]
host = []
for s in range(4):
    if args.noise:
        host.append(np.random.default_rng(s).integers(0, 256, (h, w, 3), dtype=np.uint8))
        enc.h2d(d_in[s], host[-1])
    else:
        enc.fill_synthetic(d_in[s], w, h, 1, first_frame=s)
d_out = [enc.malloc(out_stride) for _ in range(args.lanes)]
d_len = [enc.malloc(4) for _ in range(args.lanes)]


def run(n):
    for i in range(n):
        enc.encode_device(d_in[i % 4], 1, w, h, None, d_out[i % args.lanes], out_stride, d_len[i % args.lanes],
                          frame_stride=w * h * 3, opt_c=opt_c)


run(20)
enc.synchronize()
us = []
for r in range(args.runs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    enc.synchronize()
    us.append((time.perf_counter() - t0) * 1e6 / args.steps)
ok = None
if args.check:
    import oracle  # (checker)
    from oracle.synth import synthetic
    i = args.steps - 1
    n = int(np.frombuffer(enc.d2h(d_len[i % args.lanes], 4), np.uint32)[0])
    frame = host[i % 4] if args.noise else synthetic(w, h, frame=i % 4)
    ok = enc.d2h(d_out[i % args.lanes], n) == oracle.encode(frame, 255, args.sub, luma, chroma, threads=16, parallel=True)
print(json.dumps({"format": os.environ.get("DMMT_COEF_FORMAT", "auto"), "size": args.size, "sub": args.sub,
                  "quality": args.quality, "noise": args.noise, "lanes": args.lanes, "steps": args.steps,
                  "us_per_frame_median": round(statistics.median(us), 2), "us_per_frame": [round(x, 2) for x in us],
                  "matches_oracle": ok}), flush=True)
enc.close()
