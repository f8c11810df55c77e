"""Mixed call sequences on one context.  The other GPU tests check one call, or calls
of one kind and size; a dmmt_ctx carries state from call to call: per-lane workspaces
grown on demand and never shrunk, histogram replicas and arrival counters that each
launch leaves zero for the next, tables shared by the lanes and swapped behind a
synchronisation, the wide or narrow coefficient form chosen per call over the other
form's stale blocks, one synchronous and one asynchronous status group per lane, the
event pair that orders a caller's stream against lane 0, the graph cache and its
eviction, and the analysed stripe between the steps of the stripe protocol.  Here
geometry, frame count, sample type, entry point and tables change between calls that
are still in flight, the synchronous entry points run while the lanes are busy, and
every output is compared byte for byte with its CPU reference (oracle,
tests/ycc_ref.py, tests/gray_ref.py, the host PPM reader).

Every test creates its own Encoder, so that the workspaces start empty and grow at
calls the test knows.  The building blocks (Job: one asynchronous call with its
reference; sync_op; striped_file; invalidated_stripe) are tests/tools/sequence_fuzz.py's,
whose seeded sweep runs here for a fixed seed."""
import os
import sys

import numpy as np
import pytest

import dmmt_jpeg
import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import sequence_fuzz as sf  # noqa: E402

gpu = pytest.mark.gpu

SHORT_STEPS, SHORT_SEED = 150, 26  # (test_sequence_schedule_covers_every_kind pins what this seed draws)


def blocks(w, h, sub, n=1):
    """the 8x8 blocks of n frames: what sizes a lane's workspace"""
    hr, vr = (1 if sub == 0 else 2), (2 if sub == 2 else 1)
    wp, hp = -(-w // (8 * hr)) * 8 * hr, -(-h // (8 * vr)) * 8 * vr
    return n * (wp * hp // 64 + 2 * (wp // hr) * (hp // vr) // 64)


def per_lane(specs, lanes):
    """the calls of a round-robin sequence that land on each lane, in order"""
    return [[s for i, s in enumerate(specs) if i % lanes == k] for k in range(lanes)]


def grows_shrinks_and_adds_frames(seq):
    """a lane's calls regrow its workspace after the first call, run a smaller call in
    the buffers a larger one left, and raise n_frames above every earlier call's"""
    need = [blocks(s["w"], s["h"], s["sub"], s["n"]) for s in seq]
    grow = any(need[j] > max(need[:j]) for j in range(1, len(seq)))
    shrink = any(need[j] < max(need[:j]) for j in range(1, len(seq)))
    frames = any(seq[j]["n"] > max(s["n"] for s in seq[:j]) for j in range(1, len(seq)))
    return grow and shrink and frames


def check_all(jobs):
    try:
        for i, job in enumerate(jobs):
            assert job.mismatch() is None, (i, job.mismatch())
    finally:
        for job in jobs:
            job.free()


# ------------------------------------------------------------------ a. geometry and frame count in flight

SIZES = [(9, 9), (328, 200), (40, 24), (264, 256), (1, 65)]  # (264 x 256 at 4:4:4: 13 chunks)


def geometry_specs(lanes):
    """3 * lanes + 1 calls.  Call i is lane k = i % lanes's call of round r = i // lanes:
    along the calls of a round, and along the rounds of a lane, the sizes cycle tiny ->
    larger -> tiny and the subsampling 0/1/2; n_frames cycles 1, 3, 2 over a lane's
    rounds (from 2 on the odd lanes, so that every lane meets a count above all its
    earlier ones) and the restart interval 0, 1, 7 over the calls"""
    specs = []
    for i in range(3 * lanes + 1):
        k, r = i % lanes, i // lanes
        w, h = SIZES[(k + r + 4) % len(SIZES)]
        q = (90, 100, 50, 100)[(k + r) % 4]  # narrow, wide, narrow, wide along a lane's rounds
        specs.append(dict(kind=("rgb_u8", "rgb_f32")[q == 100 and i % 2], w=w, h=h, sub=(k + r) % 3,
                          n=(1, 3, 2)[(r + 2 * (k % 2)) % 3], ri=(0, 1, 7)[i % 3], q=q, seed=1000 + i,
                          content=("noise", "synthetic")[i % 2]))
    assert len(specs) >= 3 * lanes + 1
    for k, seq in enumerate(per_lane(specs, lanes)):  # from the schedule, not by hoping
        assert grows_shrinks_and_adds_frames(seq) and alternates_forms(seq), (lanes, k)
    return specs


def alternates_forms(seq):
    """a lane's calls store their blocks narrow after wide and wide after narrow (q100
    and f32 dots: wide; q50 and q90: narrow)"""
    wide = [s["q"] == 100 or s["kind"].endswith("f32") for s in seq]
    steps = set(zip(wide, wide[1:]))
    return (True, False) in steps and (False, True) in steps


@gpu
@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_geometry_and_frame_count_change_in_flight(lanes):
    specs = geometry_specs(lanes)
    with dmmt_jpeg.Encoder(0) as enc:
        enc.set_lanes(lanes)
        jobs = [sf.Job(enc, s) for s in specs]
        for job in jobs:  # nothing synchronises between the calls but the library itself
            job.submit()
        enc.synchronize()
        check_all(jobs)


# ------------------------------------------------------------------ b. kinds mixed in flight

# kind -> (entry point, sample type: the dtype and what its table is filled for)
KIND_TRAITS = {
    "rgb_u8": ("device", ("u8", 255)), "rgb_u8_mv100": ("device", ("u8", 100)), "rgb_u16": ("device", ("u16", 65535)),
    "rgb_u16_mv1000": ("device", ("u16", 1000)), "rgb_f32": ("device", ("f32", None)),
    "bgrx_pitched": ("surfaces", ("u8", 255)), "planar_f32": ("surfaces", ("f32", None)),
    "nv12": ("ycc", ("u8", "YCbCr")), "i444_pitched": ("ycc", ("u8", "YCbCr")),
    "gray_u16_mv4095": ("gray", ("u16", 4095)), "gray_y": ("gray", ("u8", "Y")),
}
MIXED_ORDER = ["gray_u16_mv4095", "rgb_u8", "planar_f32", "rgb_u8_mv100", "nv12", "rgb_u16", "bgrx_pitched", "rgb_f32",
               "i444_pitched", "rgb_u16_mv1000", "gray_y",
               "rgb_u8", "gray_y", "rgb_u8_mv100", "planar_f32", "rgb_u16", "nv12", "rgb_f32", "bgrx_pitched",
               "rgb_u16_mv1000", "i444_pitched", "gray_u16_mv4095"]


def mixed_specs():
    specs = [dict(kind=kind, w=8 + (i * 53) % 190, h=5 + (i * 37) % 150, sub=i % 3, n=(1, 2, 1, 3)[i % 4],
                  ri=(0, 0, 7, 1)[i % 4], q=(50, 90, 100)[i % 3], seed=2000 + i,
                  content=("synthetic", "noise")[i % 2])
             for i, kind in enumerate(MIXED_ORDER)]
    assert set(MIXED_ORDER) == set(sf.ASYNC_KINDS) == set(KIND_TRAITS)
    for a, b in zip(specs, specs[1:]):  # every call differs from the one before it
        (ea, ta), (eb, tb) = KIND_TRAITS[a["kind"]], KIND_TRAITS[b["kind"]]
        assert ea != eb and ta != tb and a["q"] != b["q"] and (a["w"], a["h"]) != (b["w"], b["h"]), (a, b)
    return specs


@gpu
def test_kinds_mixed_in_flight():
    import torch
    specs = mixed_specs()
    with dmmt_jpeg.Encoder(0) as enc:
        streams = [torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)]
        enc.set_lanes(2)
        jobs = [sf.Job(enc, s) for s in specs]
        for i, job in enumerate(jobs):  # every second call on a caller's stream, two of them in turn
            job.submit(streams[(i // 2) % 2].cuda_stream if i % 2 else None)
        enc.synchronize()
        for s in streams:
            s.synchronize()
        check_all(jobs)


# ------------------------------------------------------------------ c. synchronous entry points among busy lanes

@gpu
def test_synchronous_entry_points_among_busy_lanes():
    queued = [dict(kind=kind, w=w, h=h, sub=sub, n=n, ri=ri, q=90, seed=3000 + i, content="synthetic")
              for i, (kind, w, h, sub, n, ri) in enumerate([
                  ("rgb_u8", 328, 200, 2, 3, 0), ("rgb_u16_mv1000", 40, 24, 0, 1, 7), ("bgrx_pitched", 264, 256, 0, 2, 0),
                  ("rgb_u8", 200, 136, 1, 3, 1), ("gray_u16_mv4095", 120, 90, 0, 2, 0), ("nv12", 330, 260, 2, 2, 0)])]
    with dmmt_jpeg.Encoder(0) as enc:
        enc.set_lanes(3)
        jobs = [sf.Job(enc, s) for s in queued]
        for job in jobs:
            job.submit()
        for i, kind in enumerate(sf.SYNC_KINDS):  # each with a geometry and tables of its own
            s = dict(kind=kind, w=23 + 31 * i, h=150 - 13 * i, sub=(i + 1) % 3, q=(50, 100, 75)[i % 3],
                     ri=(0, 5)[i % 2], seed=3100 + i, content=("noise", "synthetic")[i % 2])
            err = sf.sync_op(enc, s)
            assert err is None, (kind, err)
        enc.synchronize()
        check_all(jobs)


# ------------------------------------------------------------------ d. errors do not leak

BAD_CALL_CASES = [(1, 0), (3, 0), (3, 1), (3, 2)]  # (lanes, the lane of the bad call)


def bad_call_specs(lanes, k):
    def good(i, w, h, sub):
        return dict(kind=("rgb_u8", "rgb_u16")[i % 2], w=w, h=h, sub=sub, n=1 + i % 2, ri=0, q=(90, 100)[i % 2],
                    seed=4000 + 16 * lanes + i, content="noise")
    before = [good(i, 72, 40, 1) for i in range(lanes + k)]  # a round over every lane, then up to lane k
    bad = dict(kind="rgb_u8", w=72, h=40, sub=1, n=1, ri=0, q=90, seed=4900, bad=True)
    after = [good(20 + i, 33, 57, 2) for i in range(2 * lanes)]  # two more rounds, of another geometry
    calls = before + [bad] + after
    assert len(before) % lanes == k  # where the round-robin puts the bad call
    assert sum(1 for i in range(len(calls)) if i % lanes == k) >= 4  # good calls on lane k before and after it
    return calls


@gpu
@pytest.mark.parametrize("lanes,k", BAD_CALL_CASES)
def test_bad_call_spoils_nothing_else(lanes, k):
    with dmmt_jpeg.Encoder(0) as enc:
        enc.set_lanes(lanes)
        jobs = [sf.Job(enc, s) for s in bad_call_specs(lanes, k)]
        for job in jobs:
            job.submit()
        rgb = sf.pixels(4999, 1, 50, 61, 255)[0]
        o = sf.options(0, 75)
        assert enc.encode(dmmt_jpeg.Image.from_array(rgb), o) == oracle.encode(rgb, 255, 0, o.luma_table,
                                                                               o.chroma_table)
        with pytest.raises(dmmt_jpeg.Error) as ei:
            enc.synchronize()
        assert ei.value.name == "ValueExceedsMax"
        enc.synchronize()  # exactly once
        check_all([j for j in jobs if not j.bad])
        for j in jobs:
            j.free()


# ------------------------------------------------------------------ e. the graph cache under change

def graph_specs():
    """20 calls of pairwise different keys on a DMMT_GRAPHS=1 context (more than the 16
    the cache holds: the first are evicted), the lane's workspace regrown midway (the
    captured launches hold the old pointers), then the first four again (captured
    again) and the last four (replayed)"""
    kinds = ["rgb_u8", "bgrx_pitched", "planar_f32", "nv12", "gray_y", "rgb_u16", "i444_pitched", "rgb_f32"]
    sizes = [(40, 24), (56, 40), (24, 16), (33, 9)] * 2 + [(200, 136)] + [(64, 48), (17, 65), (80, 8)] * 2 + \
        [(328, 200)] + [(48, 48), (9, 9), (72, 56), (40, 40)]
    specs = [dict(kind=kinds[i % len(kinds)], w=w, h=h, sub=i % 3, n=(1, 2, 3)[i % 3], ri=(0, 3)[i % 2],
                  q=(90, 100, 50)[i % 3], seed=5000 + i, content=("noise", "synthetic")[i % 2])
             for i, (w, h) in enumerate(sizes)]
    assert len(specs) == 20
    need = [blocks(s["w"], s["h"], sf.effective_sub(s), s["n"]) for s in specs]
    assert sum(1 for j in range(4, 20) if need[j] > max(need[:j])) >= 2  # regrown midway, twice
    return specs


@gpu
def test_graph_cache_eviction_and_regrowth():
    specs = graph_specs()
    os.environ["DMMT_GRAPHS"] = "1"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_GRAPHS")
    jobs = []
    try:
        jobs = [sf.Job(enc, s) for s in specs]
        for i in list(range(20)) + [0, 1, 2, 3] + [16, 17, 18, 19]:
            jobs[i].submit()
            enc.synchronize()
            assert jobs[i].mismatch() is None, (i, jobs[i].mismatch())
    finally:
        for job in jobs:
            job.free()
        enc.close()


# ------------------------------------------------------------------ f. the pending stripe

STRIPE_W, STRIPE_H = 96, 64


def stripe_image(sub):
    return sf.pixels(6000 + sub, 1, STRIPE_H, STRIPE_W, 255, "synthetic")[0]


def whole_protocol_is_exact(enc, sub, joined):
    rgb = stripe_image(sub)
    data, o = sf.striped_file(enc, rgb, sub, 90, 2, joined)
    return data == oracle.encode(rgb, 255, sub, o.luma_table, o.chroma_table, restart_interval=o.restart_interval)


@gpu
@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("mode", sf.STRIPE_MODES)
@pytest.mark.parametrize("x", ["encode_small", "encode_large", "encode_coefficients", "forward_blocks", "encode_gray",
                               "encode_device_1_lane", "encode_device_lane0_of_2", "encode_device_lane1_of_2"])
def test_other_call_invalidates_pending_stripe(sub, mode, x):
    """analyze -> X -> the stripe's next step: DMMT_E_INVALID_ARGUMENT (-102), never
    bytes, whichever lane X ran on; then the whole protocol on the same context is exact"""
    with dmmt_jpeg.Encoder(0) as enc:
        jobs = []
        if x.startswith("encode_device"):
            spec = dict(kind="rgb_u8", w=136, h=104, sub=1, n=2, ri=0, q=75, seed=6100, content="noise")
            jobs = [sf.Job(enc, spec)]
            if x != "encode_device_1_lane":
                enc.set_lanes(2)
            if x == "encode_device_lane1_of_2":
                jobs.append(sf.Job(enc, dict(spec, w=24, h=16, seed=6101)))
                jobs[1].submit()  # lane 0, before the stripe: X is then the call for lane 1
            call = sf.invalidator(enc, "encode_device", 0, jobs[0])
        else:
            call = sf.invalidator(enc, x, 6200 + sub)
        try:
            assert sf.invalidated_stripe(enc, stripe_image(sub), sub, 90, mode, call) is None
            assert whole_protocol_is_exact(enc, sub, mode != "restart")
            enc.synchronize()
            for job in jobs:
                assert job.mismatch() is None
        finally:
            for job in jobs:
                job.free()


@gpu
@pytest.mark.parametrize("sub", [0, 2])
def test_fresh_analyze_replaces_pending_stripe(sub):
    a, b = stripe_image(sub), sf.pixels(6300 + sub, 1, 40, 56, 255, "noise")[0]
    with dmmt_jpeg.Encoder(0) as enc:
        oa, ob = sf.stripe_options(STRIPE_W, sub, 90, False), sf.stripe_options(56, sub, 50, False)
        sa, sb = sf.Stripes(enc, a, sub, oa, 1), sf.Stripes(enc, b, sub, ob, 1)
        try:
            enc.stripe_analyze(sa.items[0][0], oa)
            st, d_out, cap = sb.items[0]
            hist = enc.stripe_analyze(st, ob)
            got = enc.d2h(d_out, enc.stripe_encode(hist, d_out, cap))
            assert got == oracle.encode(b, 255, sub, ob.luma_table, ob.chroma_table,
                                        restart_interval=ob.restart_interval)
        finally:
            sa.free()
            sb.free()


@gpu
@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("joined", [False, True])
def test_benign_calls_leave_pending_stripe_valid(sub, joined):
    with dmmt_jpeg.Encoder(0) as enc:
        other = enc.malloc(64 * 48 * 3)

        def benign():
            d = enc.malloc(4096)
            enc.h2d(d, np.arange(1024, dtype=np.uint32))
            assert np.array_equal(np.frombuffer(enc.d2h(d, 4096), np.uint32), np.arange(1024, dtype=np.uint32))
            enc.free(d)
            enc.synchronize()
            enc.fill_synthetic(other, 64, 48, 1)
            enc.set_lanes(2)
            enc.set_lanes(1)
        try:
            rgb = stripe_image(sub)
            data, o = sf.striped_file(enc, rgb, sub, 90, 2, joined, between=benign)
            assert data == oracle.encode(rgb, 255, sub, o.luma_table, o.chroma_table,
                                         restart_interval=o.restart_interval)
        finally:
            enc.free(other)


# ------------------------------------------------------------------ the seeded sweep

def test_sequence_test_schedules_meet_their_conditions():
    """what tests a, b, d and e assert of their own schedules, checked without a GPU"""
    for lanes in (2, 3, 4):
        geometry_specs(lanes)
    mixed_specs()
    for lanes, k in BAD_CALL_CASES:
        bad_call_specs(lanes, k)
    graph_specs()


def test_sequence_schedule_covers_every_kind():
    """the schedule of the short sweep, drawn without a GPU: every kind of operation at
    least three times, and at least ten steps among two or more calls in flight"""
    sched = sf.draw_schedule(SHORT_STEPS, SHORT_SEED)
    assert sched == sf.draw_schedule(SHORT_STEPS, SHORT_SEED)
    summary = sf.schedule_summary(sched)
    assert set(summary["counts"]) == set(sf.ALL_KINDS)
    assert min(summary["counts"].values()) >= 3, summary
    assert summary["steps_with_two_in_flight"] >= 10, summary
    outstanding = 0
    for s in sched:  # never more than MAX_OUTSTANDING outputs wait for their check
        if s["kind"] in ("synchronize", "set_lanes"):
            outstanding = 0
        elif s["kind"] in sf.ASYNC_KINDS or s["kind"] == "bad_maxval" or \
                (s["kind"] == "stripe_invalidated" and s["x"] == "encode_device"):
            outstanding += 1
        assert outstanding <= sf.MAX_OUTSTANDING


@gpu
def test_seeded_sequences_short():
    res = sf.run(SHORT_STEPS, SHORT_SEED, log=lambda line: None)
    assert "mismatch" not in res, res
    assert res["steps"] == SHORT_STEPS
    print(res)
    assert min(res["counts"].values()) >= 3, res
    assert res["steps_with_two_in_flight"] >= 10, res
