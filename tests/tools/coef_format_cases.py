"""Inputs of tests/test_gpu_coef_format.py and the child process that encodes them
-- TEST INFRASTRUCTURE.

The form of the quantised blocks (csrc/coef_format.hpp) is fixed when a context is
created, from DMMT_COEF_FORMAT, so the test runs this file once per setting in a
fresh process:  python coef_format_cases.py OUT.json  encodes every case on the GPU,
compares it byte for byte with the CPU reference and writes {case id: "ok" | what
differs}.  The parent proves by a census of the reference's coefficients
(census(), from oracle.forward alone) that each case holds the escapes it is named
for, before it looks at the results."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "dmmt-jpeg-encoder_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dmmt_jpeg  # noqa: E402
import oracle  # noqa: E402
from oracle.np_ref import ZIGZAG  # noqa: E402
from oracle.synth import synthetic  # noqa: E402

SIZES = [(8, 8), (9, 13), (33, 17), (136, 136)]  # (w, h); 136 x 136 4:4:4: 289 luma blocks, two chunks and more
SUBS = [0, 1, 2]
ONES = [1] * 64
# 1 at the eight lo positions, 255 elsewhere: large values below position 8 only
LO_TABLE = [1 if i in [int(ZIGZAG[k]) for k in range(8)] else 255 for i in range(64)]
MCU_W = {0: 8, 1: 16, 2: 16}
MCU_H = {0: 8, 1: 8, 2: 16}


def census(blocks):
    """blocks: (n, 64) zigzag int16.  An escape is an AC outside -127..127."""
    b = np.asarray(blocks, np.int64)
    esc = np.abs(b) > 127
    esc[:, 0] = False
    nz_hi = int((b[:, 8:] != 0).sum())
    # a block's bits are at least one code bit and the category's extra bits per non-zero AC
    cat = np.where(b[:, 1:] != 0, np.floor(np.log2(np.maximum(np.abs(b[:, 1:]), 1))).astype(np.int64) + 1, 0)
    min_bits = (cat + (b[:, 1:] != 0)).sum(axis=1)
    return {"lo": int(esc[:, 1:8].sum()), "hi": int(esc[:, 8:].sum()), "nz_hi": nz_hi,
            "hi_values": set(np.unique(b[:, 8:][esc[:, 8:]]).tolist()), "max_abs": int(np.abs(b).max()),
            "hi_blocks": int(esc[:, 8:].any(axis=1).sum()), "hi_per_block": esc[:, 8:].sum(axis=1),
            "blocks": b.shape[0], "min_bits": min_bits}


def gray_noise(w, h, seed, levels=256):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, levels, (h, w, 1)) * (255 // (levels - 1))
    return np.repeat(g, 3, axis=2).astype(np.uint8)


def colour_noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def bars(w, h, seed):
    """black and white bars 4 pixels wide with a little noise: every block's (0, 1) coefficient is large"""
    rng = np.random.default_rng(seed)
    x = np.arange(w)[None, :, None]
    img = np.where((x % 8) < 4, 235, 20) + rng.integers(-20, 21, (h, w, 1))
    return np.repeat(img, 3, axis=2).astype(np.uint8)


def exact_seed(w, h, sub):
    """the first seed whose full-range noise, divided by all-ones tables, has an escape at
    a position >= 8 (every size) and there the exact values 127, -127, 128, -128 (136 x 136)"""
    want = {128, -128} if (w, h) != (136, 136) else None
    for seed in range(200):
        b = np.asarray(oracle.forward(gray_noise(w, h, seed), 255, sub, ONES, ONES), np.int64)[:, 8:]
        vals = set(np.unique(b).tolist())
        if want is None:
            if {127, -127, 128, -128} <= vals:
                return seed
        elif (np.abs(b) > 127).any():
            return seed
    raise AssertionError("no seed found")


def u16_image(w, h, seed):
    """u16 samples up to maxval 65535: a saturated left part (the largest DC) beside binary noise"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 2, (h, w, 1)).astype(np.uint16) * 65535
    g[:, : max(w // 2, 1)] = 65535
    return np.repeat(g, 3, axis=2)


def q(quality):
    return dmmt_jpeg.quality_tables(quality)


def rgb_cases():
    """(id, rgb, maxval, sub, luma, chroma, restart interval) of the cases encoded from R,G,B frames"""
    out = []
    for (w, h) in SIZES:
        for sub in SUBS:
            tag = f"{w}x{h}-{sub}"
            out.append((f"none-{tag}", synthetic(w, h, frame=7), 255, sub, *q(50), 0))
            out.append((f"lo_only-{tag}", bars(w, h, 3), 255, sub, LO_TABLE, LO_TABLE, 0))
            out.append((f"hi_exact-{tag}", gray_noise(w, h, exact_seed(w, h, sub)), 255, sub, ONES, ONES, 0))
            out.append((f"dense_rewalk-{tag}", gray_noise(w, h, 11, levels=2), 255, sub, ONES, ONES, 0))
            out.append((f"u16-{tag}", u16_image(w, h, 5), 65535, sub, ONES, ONES, 0))
            out.append((f"restart-{tag}", colour_noise(w, h, 9), 255, sub, *q(90), 2))
    return out


def opts(sub, luma, chroma, ri=0):
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=list(luma),
                                              chroma_table=list(chroma), restart_interval=ri)


def stripe_sizes():
    return [(w, h, sub) for (w, h) in SIZES for sub in SUBS if -(-h // MCU_H[sub]) >= 2]


def run_all():
    import torch

    import ycc_ref
    from test_gpu_stripes import _joined_on_one_gpu

    res = {}
    enc = dmmt_jpeg.Encoder(0)

    def note(cid, got, want):
        res[cid] = "ok" if got == want else f"differs: {len(got)} bytes against {len(want)}"

    for cid, rgb, mv, sub, luma, chroma, ri in rgb_cases():
        got = enc.encode(dmmt_jpeg.Image.from_array(rgb, mv), opts(sub, luma, chroma, ri))
        note(cid, got, oracle.encode(rgb, mv, sub, luma, chroma, restart_interval=ri))
    for (w, h) in SIZES:
        for sub in SUBS:
            tag = f"{w}x{h}-{sub}"
            for name, (luma, chroma) in (("q90", q(90)), ("ones", (ONES, ONES))):
                y, cb, cr = ycc_ref.random_planes(w, h, sub, 21)
                got = enc.encode_ycc(y, cb=cb, cr=cr, options=opts(sub, luma, chroma))
                note(f"ycc_planar_{name}-{tag}", got, ycc_ref.encode(y, cb, cr, sub, luma, chroma))
            rgb = colour_noise(w, h, 31)
            x = np.concatenate([rgb, np.full((h, w, 1), 0xFF, np.uint8)], axis=2)
            t = torch.from_numpy(x).to("cuda:0")
            got = enc.encode_tensor(t, opts(sub, ONES, ONES), layout="HWC")[0]
            note(f"rgbx-{tag}", got, oracle.encode(rgb, 255, sub, ONES, ONES))
    # a joined two-stripe encode: the DC edges come from coef_lo in the narrow form
    for (w, h, sub) in stripe_sizes():
        rgb = colour_noise(w, h, 41)
        got, o = _joined_on_one_gpu(rgb, sub, 90, 2)
        note(f"joined-{w}x{h}-{sub}", got, oracle.encode(rgb, 255, sub, o.luma_table, o.chroma_table))
    # three lanes, frames whose tables make the rule pick narrow (q90) and wide (q100) in turn
    for (w, h) in SIZES[2:]:
        for sub in SUBS:
            frames = [colour_noise(w, h, 50 + i) if i % 3 else synthetic(w, h, frame=50 + i) for i in range(7)]
            tabs = [q(90) if i % 2 == 0 else q(100) for i in range(7)]
            stride = dmmt_jpeg.max_jpeg_bytes(w, h, sub)
            d_in = [enc.malloc(f.nbytes) for f in frames]
            d_out = [enc.malloc(stride) for _ in frames]
            d_len = [enc.malloc(4) for _ in frames]
            try:
                for d, f in zip(d_in, frames):
                    enc.h2d(d, f)
                enc.set_lanes(3)
                for i in range(7):
                    enc.encode_device(d_in[i], 1, w, h, opts(sub, *tabs[i]), d_out[i], stride, d_len[i])
                enc.synchronize()
                bad = []
                for i, f in enumerate(frames):
                    n = int(np.frombuffer(enc.d2h(d_len[i], 4), np.uint32)[0])
                    if enc.d2h(d_out[i], n) != oracle.encode(f, 255, sub, *tabs[i]):
                        bad.append(i)
                res[f"lanes_mix-{w}x{h}-{sub}"] = "ok" if not bad else f"frames {bad} differ"
            finally:
                enc.set_lanes(1)
                for d in d_in + d_out + d_len:
                    enc.free(d)
    # -32768 has no category: DMMT_E_CATEGORY_RANGE (-101), from Image<f32> dots and from host blocks
    codes = []
    dots = np.full((8, 8, 3), -1000.0, np.float32)
    dots[:, 4:, :] = 1000.0
    blocks = np.zeros((3 * 4, 64), np.int16)
    blocks[4, 9] = -32768
    for call in (lambda: enc.encode(dmmt_jpeg.Image.from_array(dots, 255), opts(0, *q(90))),
                 lambda: enc.encode_coefficients(blocks, 32, 8, opts(0, *q(90)))):
        try:
            call()
            codes.append(0)
        except dmmt_jpeg.Error as e:
            codes.append(e.code)
    ok = synthetic(16, 16)
    after = enc.encode(dmmt_jpeg.Image.from_array(ok), opts(0, *q(90))) == oracle.encode(ok, 255, 0, *q(90))
    res["cat_range"] = "ok" if codes == [-101, -101] and after else f"codes {codes}, encode after it {after}"
    enc.close()
    return res


if __name__ == "__main__":
    results = run_all()
    with open(sys.argv[1], "w") as f:
        json.dump({"format": os.environ.get("DMMT_COEF_FORMAT", "auto"), "results": results}, f)
