"""k_front's narrow store with the folded range test (csrc/coef_format.hpp,
DMMT_NARROW_FOLD): the values at the edge of the test -- 127 and -127, the last a
byte holds, 128 and -128, the first escapes -- at a hi row of every column and at
the first hi row of columns 0..3, alone in an otherwise quiet frame, so the wave
that holds them takes the path without clamps (+-127) or has exactly one escaping
block (+-128).  Integer samples, all-ones tables, byte for byte against the CPU
reference; DMMT_COEF_FORMAT=narrow in a fresh child process (the form is fixed when
a context is created), the same frames under wide as control
(tests/tools/narrow_fold_cases.py builds the frames and encodes them).

Shapes: 8x8 and 24x16 4:4:4 (one tile, a partial one), 32x16 4:2:2, 32x32 4:2:0,
264x16 4:4:4 (a second tile with one valid MCU column; a frame with black-and-white
noise in that column only, so whatever the tile's other lanes hold is out of range
next to valid blocks), 8x8 gray (k_front_gray has a narrow twin).

Each case first proves its census on the reference's coefficients alone.

The cases hold for either setting of DMMT_NARROW_FOLD: the product builds with the
switch off (profiles/STUDIES.md section K), where the same frames go through the
clamps of every wave; a build with the switch on passed them too."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import narrow_fold_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
FORMATS = ["narrow", "wide"]
IDS = [c[0] for c in cases.CASES]
BLOCKS = {"8x8-444": 3, "24x16-444": 18, "32x16-422": 16, "32x32-420": 24, "264x16-444": 198, "8x8-gray": 1}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("narrow_fold")
    for fmt in FORMATS:
        path = str(d / f"{fmt}.json")
        env = dict(os.environ, DMMT_COEF_FORMAT=fmt)
        r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "narrow_fold_cases.py"), path], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (fmt, r.stdout[-2000:], r.stderr[-4000:])
        got = json.load(open(path))
        assert got["format"] == fmt
        out[fmt] = got["results"]
    return out


def prove_census(cid):
    c = cases.census(cid)
    print(cid, c["blocks"], c["lo_only_blocks"], c["one_escape_frames"], c["edge_no_escape"], c["escaping_blocks"])
    assert c["blocks"] == BLOCKS[cid]
    # +127, -127, +128 and -128 at a hi position in each of the eight columns
    assert c["hi_seen"] >= {(col, v) for col in range(8) for v in cases.EDGE}
    # the same at the first hi row of columns 0..3
    assert c["first_seen"] >= {(r, col, v) for (r, col) in cases.FIRST_HI for v in cases.EDGE}
    # a block whose only values beyond +-127 sit at zigzag positions 0..7
    assert c["lo_only_blocks"] >= 1
    # exactly one escaping block in a frame (alone in its wave): every +-128 frame; and
    # a +-127 at a hi position in a frame without any escape: every +-127 frame
    assert c["one_escape_frames"] >= 24 and c["edge_no_escape"] >= 24
    # most blocks of the dense frame escape (one luma block of three, four or six is
    # luma-only noise: the chroma of a gray frame is zero)
    assert max(c["escaping_blocks"]) >= max(1, BLOCKS[cid] // 6)


def test_census_needs_no_gpu_result():
    """the search itself: every designed block exists (at most 200 candidates each)"""
    assert len(cases.designed_blocks()) == 4 * (len(cases.ANY_HI) + len(cases.FIRST_HI))


@pytest.mark.parametrize("cid", IDS)
def test_edge_values_at_every_column(results, cid):
    prove_census(cid)
    for fmt in FORMATS:
        bad = [r for r in results[fmt][cid] if r != "ok"]
        assert not bad, (cid, fmt, bad)
