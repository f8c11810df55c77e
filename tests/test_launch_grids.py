"""CPU check of the capped grids of the looping kernels (csrc/launch_grids.hpp, the
launchers' own header compiled for the host): front_grid_x and hist_grid_x against
a hand-computed table -- n_frames above, equal to and below the resident count, a
share of 0 giving 1, the per-CU cap and the cap ignored under DMMT_FRONT_PER_CU,
fewer tiles than the bound, k_hist's caps 1024 and 512 -- and the Python mirror
(tests/tools/loop_cases.py), which the GPU tests assert their preconditions from,
against the table and against the header on a seeded sweep."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "launch_grid_check.cpp")
sys.path.insert(0, os.path.join(HERE, "tools"))

import loop_cases as lc  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grids") / "launch_grid_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC], check=True)
    return exe


def ask(checker, front, hist):
    text = "".join("f %d %d %d %d %d %d\n" % a for a in front) + "".join("h %d %d %d\n" % a for a in hist)
    r = subprocess.run([checker], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [int(x) for x in r.stdout.split()]
    assert len(out) == len(front) + len(hist)
    return out[:len(front)], out[len(front):]


@needs_gxx
def test_header_matches_the_table(checker):
    f, h = ask(checker, [a for a, _ in lc.FRONT_TABLE], [a for a, _ in lc.HIST_TABLE])
    assert f == [want for _, want in lc.FRONT_TABLE]
    assert h == [want for _, want in lc.HIST_TABLE]


def test_mirror_matches_the_table():
    for a, want in lc.FRONT_TABLE:
        assert lc.front_grid_x(*a) == want, a
    for a, want in lc.HIST_TABLE:
        assert lc.hist_grid_x(*a) == want, a


@needs_gxx
def test_mirror_matches_the_header_on_a_sweep(checker):
    rng = np.random.default_rng(2024)
    front, hist = [], []
    for _ in range(4000):
        cus = int(rng.choice([1, 64, 104, 256, 304]))
        resident = cus * int(rng.integers(1, 9))
        n_frames = int(rng.choice([1, 2, 3, resident - 1 or 1, resident, resident + 1, 2 * cus, int(rng.integers(1, 5000))]))
        ntiles = int(rng.choice([0, 1, 2, 10, int(rng.integers(1, 40)), int(rng.integers(1, 1 << 20)), 3 << 31]))
        front.append((resident, cus, int(rng.integers(0, 2)), ntiles, n_frames, int(rng.integers(0, 5))))
        bpf = int(rng.choice([0, 1, 255, 256, 257, 555, int(rng.integers(1, 2000)), int(rng.integers(1, 1 << 24))]))
        hist.append((bpf, n_frames, int(rng.choice([512, 1024, 384, 1]))))
    f, h = ask(checker, front, hist)
    assert f == [lc.front_grid_x(*a) for a in front]
    assert h == [lc.hist_grid_x(*a) for a in hist]
    assert len(set(f)) > 20 and len(set(h)) > 20  # the sweep is no constant


def test_shapes_meet_the_preconditions():
    """the GPU cases' shapes on an MI355X (256 CUs, 512 frames per launch), block
    counts as the cases name them, rows and frames never 16-byte aligned"""
    for key, gray, blocks in ((0, False, 555), (1, False, 532), (2, False, 570), (0, True, 518)):
        w, h = lc.shape(key, gray)
        assert lc.geometry(w, h, key, gray)["bpf"] == blocks
        assert lc.require_loops(w, h, key, gray, 512, 256, lanes=True) == (1, 1)
        bound, hist = lc.require_loops(w, h, key, gray, 512, 256, lanes=False)
        assert (bound, hist) == (4, 2)
        for sb in (1, 2, 4):
            spp = 1 if gray else 3
            assert (w * spp * sb) % 16 and (w * h * spp * sb) % 16  # tight rows, tight frames
    with pytest.raises(AssertionError):  # one frame per launch: a workgroup per tile, no loop
        lc.require_loops(290, 35, 0, False, 1, 256, lanes=True)
    with pytest.raises(AssertionError):  # 257 x 33, the older tests' shape: 165 blocks, one k_hist pass
        lc.require_loops(257, 33, 2, False, 512, 256, lanes=True)
