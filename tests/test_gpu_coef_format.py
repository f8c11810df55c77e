"""The narrow block form (csrc/coef_format.hpp: int8 ACs, 16-bit low frequencies,
escapes in the wide store) against the CPU reference, byte for byte, with
DMMT_COEF_FORMAT=narrow, wide and auto -- each in a fresh child process, since the
form is fixed when a context is created (tests/tools/coef_format_cases.py encodes
every case and reports per case).

Before a result is looked at, a census of the reference's own coefficients
(oracle.forward) proves that the case holds the escapes it is named for: an escape
is an AC outside -127..127; positions below 8 live in coef_lo, the others in
coef_hi as a byte or, escaped, in the wide store.

dense_rewalk: no frame of bounded samples can make every AC of a block an escape --
the DCT is orthonormal, so a block's 63 ACs at |v| >= 128 would need 63 * 128^2 of
the at most 64 * 128^2 its level-shifted pixels hold, with nothing left for any
other value.  The case takes the densest input the bound allows, black-and-white
noise under all-ones tables.  A full block of it has ACs of standard deviation
127.5, so 32 % of its 56 positions >= 8 are escapes, 18 +- 3.5: the census requires a
block with at least 10 and, in every chunk, a block longer than k_emit's slot
(384 bits), which sends the chunk down the window re-walk.

u16: the census requires a value of at least 500, which only the 16-bit lo words
hold (a single 4:4:4 block cannot have both the largest DC, 1020, and an AC)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import coef_format_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
FORMATS = ["narrow", "wide", "auto"]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("coef_format")
    for fmt in FORMATS:
        path = str(d / f"{fmt}.json")
        env = dict(os.environ, DMMT_COEF_FORMAT=fmt)
        r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "coef_format_cases.py"), path], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (fmt, r.stdout[-2000:], r.stderr[-4000:])
        got = json.load(open(path))
        assert got["format"] == fmt
        out[fmt] = got["results"]
    return out


@pytest.fixture(scope="module")
def rgb_cases():
    return {c[0]: c for c in cases.rgb_cases()}


def _census(case):
    cid, rgb, mv, sub, luma, chroma, ri = case
    return cases.census(oracle.forward(rgb, mv, sub, luma, chroma))


def _all_ok(results, cid):
    bad = {fmt: results[fmt][cid] for fmt in FORMATS if results[fmt][cid] != "ok"}
    assert not bad, (cid, bad)


TAGS = [f"{w}x{h}-{sub}" for (w, h) in cases.SIZES for sub in cases.SUBS]


@pytest.mark.parametrize("tag", TAGS)
def test_no_escape_anywhere(results, rgb_cases, tag):
    c = _census(rgb_cases[f"none-{tag}"])
    print(c["lo"], c["hi"], c["max_abs"])
    assert c["lo"] == 0 and c["hi"] == 0
    _all_ok(results, f"none-{tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_escapes_only_below_position_8(results, rgb_cases, tag):
    c = _census(rgb_cases[f"lo_only-{tag}"])
    print(c["lo"], c["hi"])
    assert c["lo"] > 0 and c["hi"] == 0
    _all_ok(results, f"lo_only-{tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_escapes_at_positions_from_8_with_the_edge_values(results, rgb_cases, tag):
    c = _census(rgb_cases[f"hi_exact-{tag}"])
    print(c["hi"], sorted(v for v in c["hi_values"] if abs(v) <= 129))
    assert c["hi"] > 0
    if tag.startswith("136x136"):
        # 128 and -128 are escapes; 127 and -127 are the last values a byte holds
        b = np.asarray(oracle.forward(*rgb_cases[f"hi_exact-{tag}"][1:6]), np.int64)[:, 8:]
        assert {127, -127, 128, -128} <= set(np.unique(b).tolist())
        assert {128, -128} <= c["hi_values"]
    _all_ok(results, f"hi_exact-{tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_dense_escapes_and_the_window_rewalk(results, rgb_cases, tag):
    c = _census(rgb_cases[f"dense_rewalk-{tag}"])
    print(c["hi"], c["nz_hi"], c["hi_blocks"], c["blocks"], int(c["min_bits"].max()))
    assert c["hi_per_block"].max() >= 10
    for c0 in range(0, c["blocks"], 256):  # every chunk of 256 blocks holds a block longer than a slot
        assert c["min_bits"][c0:c0 + 256].max() > 384, c0
    _all_ok(results, f"dense_rewalk-{tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_u16_maxval_65535(results, rgb_cases, tag):
    c = _census(rgb_cases[f"u16-{tag}"])
    print(c["max_abs"], c["lo"], c["hi"])
    assert c["max_abs"] >= 500 and c["hi"] > 0
    _all_ok(results, f"u16-{tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_restart_interval(results, rgb_cases, tag):
    _all_ok(results, f"restart-{tag}")


@pytest.mark.parametrize("tag", TAGS)
def test_ycc_planar_and_rgbx_surfaces(results, tag):
    for cid in (f"ycc_planar_q90-{tag}", f"ycc_planar_ones-{tag}", f"rgbx-{tag}"):
        _all_ok(results, cid)


@pytest.mark.parametrize("w,h,sub", cases.stripe_sizes())
def test_joined_two_stripe_encode(results, w, h, sub):
    _all_ok(results, f"joined-{w}x{h}-{sub}")


@pytest.mark.parametrize("tag", TAGS[6:])
def test_three_lanes_mixing_narrow_and_wide_frames(results, tag):
    _all_ok(results, f"lanes_mix-{tag}")


def test_category_range_error_in_every_form(results):
    _all_ok(results, "cat_range")
