"""The capped grids of the looping kernels, mirrored, and the inputs of
tests/test_gpu_tile_loops.py -- TEST INFRASTRUCTURE.

front_grid_x / hist_grid_x mirror csrc/launch_grids.hpp; tests/test_launch_grids.py
holds both to GRID_TABLE and the mirror to the header on a seeded sweep.  The GPU
tests assert from the mirror, before they encode, that their launch makes every
workgroup of a front kernel walk several tiles and k_hist make several passes.
They cannot learn how many workgroups of an instantiation are resident, so they
use the bound MAX_WG_PER_CU workgroups of 256 threads per CU: the grid grows with
the resident count, so a grid of 1 at the bound is a grid of 1 on the device."""
from __future__ import annotations

import os

import numpy as np

HIST_WG_CAP = 1024          # csrc/kernels.hip DMMT_HIST_WG_CAP: k_hist workgroups per launch, one lane
HIST_WG_CAP_LANES = 512     # csrc/kernels.hpp DMMT_HIST_WG_CAP_LANES: a context of several lanes
FRONT_PER_CU_LANES = 2      # csrc/kernels.hpp DMMT_FRONT_PER_CU_LANES: front workgroups per CU, several lanes
MAX_WG_PER_CU = 8           # 256-thread workgroups a CU holds at most (32 waves in 4 SIMDs of 8)


def clampi(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def front_grid_x(resident, n_cus, per_cu_env, ntiles, n_frames, per_cu_cap):
    res = min(resident, per_cu_cap * n_cus) if per_cu_cap > 0 and not per_cu_env else resident
    return clampi(ntiles, 1, res // n_frames if res // n_frames > 0 else 1)


def hist_grid_x(bpf, n_frames, wg_cap):
    per_frame = wg_cap // n_frames if wg_cap // n_frames > 0 else 1
    return clampi((bpf + 255) // 256, 1, per_frame)


# (arguments, gridDim.x) worked out by hand; 1024 resident = 4 per CU on 256 CUs
FRONT_TABLE = [
    ((1024, 256, 0, 10000, 1, 0), 1024),        # more tiles than slots: every slot
    ((1024, 256, 0, 10, 1, 0), 10),             # ntiles below the bound
    ((1024, 256, 0, 0, 1, 0), 1),               # never an empty grid
    ((1024, 256, 0, 10000, 512, 0), 2),         # n_frames below resident
    ((1024, 256, 0, 10000, 300, 0), 3),         # (1024 / 300 rounds down)
    ((1024, 256, 0, 10000, 1024, 0), 1),        # n_frames equal to resident
    ((1024, 256, 0, 10000, 1025, 0), 1),        # above: res / n_frames == 0 gives 1
    ((1024, 256, 0, 10000, 4000, 0), 1),
    ((1024, 256, 0, 10000, 1, 2), 512),         # the per-CU cap of a context of several lanes
    ((1024, 256, 0, 10000, 256, 2), 2),
    ((1024, 256, 0, 10000, 512, 2), 1),         # 2 x CUs frames: one workgroup per frame
    ((1024, 256, 0, 10000, 513, 2), 1),         # (512 / 513 == 0 gives 1)
    ((1024, 256, 1, 10000, 1, 2), 1024),        # DMMT_FRONT_PER_CU set: the cap is ignored
    ((1024, 256, 1, 10000, 512, 2), 2),
    ((256, 256, 0, 10000, 1, 2), 256),          # fewer resident than the cap allows
    ((2048, 256, 0, 10, 512, 0), 4),            # the bound of the one-lane cases: 8 per CU
    ((2048, 256, 0, 3, 512, 0), 3),
    ((1024, 256, 0, 3000000000, 1, 0), 1024),   # a tile count beyond 32 bits
]
HIST_TABLE = [
    ((555, 1, 1024), 3),                        # one workgroup per 256 blocks
    ((256, 1, 1024), 1),
    ((257, 1, 1024), 2),
    ((0, 1, 1024), 1),                          # never an empty grid
    ((97200, 1, 1024), 380),                    # 4K 4:4:4: below the cap
    ((1000000, 1, 1024), 1024),                 # the cap of one lane
    ((1000000, 1, 512), 512),                   # the cap of several lanes
    ((1000000, 3, 1024), 341),
    ((570, 256, 1024), 3),                      # the frame's share 4, three needed
    ((555, 512, 1024), 2),                      # the one-lane cases: two per frame
    ((555, 512, 512), 1),                       # the lanes cases: one per frame
    ((1000000, 513, 512), 1),                   # wg_cap / n_frames == 0 gives 1
    ((1000000, 1025, 1024), 1),
]


# ------------------------------------------------------------------ geometry

def geometry(w, h, sub, gray=False):
    """jpeg_common.hpp make_geom and the front kernels' tiles: a tile is 256 luma
    columns (32 / hr MCUs) of one MCU row"""
    hr = 1 if gray or sub == 0 else 2
    vr = 2 if sub == 2 and not gray else 1
    bpm = hr * vr + (0 if gray else 2)
    mcux, mcuy = -(-w // (8 * hr)), -(-h // (8 * vr))
    tm = 32 // hr
    per_row = -(-mcux // tm)
    return {"hr": hr, "vr": vr, "bpm": bpm, "mcux": mcux, "mcuy": mcuy, "bpf": mcux * mcuy * bpm, "tm": tm,
            "tiles_per_row": per_row, "ntiles": per_row * mcuy, "rows": 8 * vr}


WIDTH = 290
HEIGHT = {0: 35, 1: 51, 2: 67, "gray": 107}   # by subsampling: 555, 532, 570 and 518 blocks


def shape(sub, gray=False):
    return WIDTH, HEIGHT["gray" if gray else sub]


def require_loops(w, h, sub, gray, n_frames, n_cus, lanes):
    """the preconditions of a case, from the mirror; returns (front bound, k_hist grid)"""
    assert "DMMT_FRONT_PER_CU" not in os.environ, "the per-CU cap of several lanes is ignored when DMMT_FRONT_PER_CU is set"
    g = geometry(w, h, sub, gray)
    assert g["tiles_per_row"] >= 2 and g["mcux"] % g["tm"] != 0, ("two tiles per tile row, the last partial", g)
    assert g["mcuy"] >= 5 and h % g["rows"] != 0, ("five tile rows, the last of partial height", g)
    assert g["bpf"] > 512, ("three k_hist passes at one workgroup per frame", g)
    cap = FRONT_PER_CU_LANES if lanes else 0
    bound = front_grid_x(min(MAX_WG_PER_CU, cap or MAX_WG_PER_CU) * n_cus, n_cus, False, g["ntiles"], n_frames, cap)
    hist = hist_grid_x(g["bpf"], n_frames, HIST_WG_CAP_LANES if lanes else HIST_WG_CAP)
    if lanes:
        assert bound == 1 and hist == 1, (bound, hist, n_frames, n_cus)
    else:
        assert bound <= 4 and g["ntiles"] >= 2 * bound, (bound, g, n_frames, n_cus)
        assert g["bpf"] > 256 * hist, (hist, g)  # a second pass
    return bound, hist


# ------------------------------------------------------------------ content

N_DISTINCT = 5
_noise = None


def noise(n, seed):
    """n seeded random bytes, 0xFF among them (a period that is no multiple of 16)"""
    global _noise
    if _noise is None:
        _noise = np.random.default_rng(98).integers(0, 256, (1 << 20) + 4099, dtype=np.uint8)
        _noise[::7] = 0xFF
    off = (seed * 4099) % 4096
    return np.resize(_noise[off:off + (1 << 20) + 3], n)


def frame_of(n_frames):
    """frame f holds distinct[f % N_DISTINCT]"""
    return np.arange(n_frames) % N_DISTINCT


def frame_stride(span, unit):
    """past the frame's span, a multiple of the sample size and no multiple of 16"""
    fs = span + 5 * unit
    while fs % 16 == 0:
        fs += unit
    return fs


def embed(rows, pitch, fstride, lead, seed, tail=0):
    """rows (n, h, row bytes) uint8 laid into noise: frame f's row y at
    lead + f * fstride + y * pitch"""
    n, h, rowb = rows.shape
    assert pitch >= rowb and (n == 1 or fstride >= (h - 1) * pitch + rowb)
    size = lead + (n - 1) * fstride + (h - 1) * pitch + rowb + tail
    host = noise(size, seed)
    np.lib.stride_tricks.as_strided(host[lead:], (n, h, rowb), (fstride, pitch, 1))[...] = rows
    return host


def as_rows(plane):
    """a (h, samples) array of any sample type as (h, row bytes) uint8"""
    p = np.ascontiguousarray(plane)
    return p.view(np.uint8).reshape(p.shape[0], -1)
