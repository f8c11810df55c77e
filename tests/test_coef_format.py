"""CPU unit check of the narrow block form (csrc/coef_format.hpp, compiled for the
host from the header the kernels include): every int16 at every position survives
pack -> narrow form + wide store -> read; the escape byte 0x80 appears exactly for
positions >= 8 with |v| > 127 or v = -128; the lo / hi byte map is a bijection with
coef_pos; and the rule that picks the form of a call."""
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "coef_format_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coef") / "coef_format_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC], check=True)
    return exe


def test_round_trip_escape_and_byte_map(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"


def _rule(checker, luma, chroma):
    r = subprocess.run([checker, bytes(luma).hex(), bytes(chroma).hex()], capture_output=True, text=True, check=True)
    out = {}
    for line in r.stdout.splitlines():
        sb, *kv = line.split()
        out[sb] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    return out


# auto: narrow for integer samples unless a quantiser of a position >= 8 is 1
@pytest.mark.parametrize("name,tables,narrow", [
    ("ones", ([1] * 64, [1] * 64), 0),
    ("q50", None, 1),
    ("q90", None, 1),
    ("q100", None, 0),
])
def test_mode_rule(checker, name, tables, narrow):
    luma, chroma = tables if tables else dmmt_jpeg.quality_tables(int(name[1:]))
    rule = _rule(checker, list(luma), list(chroma))
    for sb in ("sb1", "sb2"):  # u8 and u16 samples
        assert rule[sb] == {"auto": narrow, "wide": 0, "narrow": 1}, (name, rule)
    # Image<f32> dots are unbounded: wide whatever is asked
    assert rule["sb4"] == {"auto": 0, "wide": 0, "narrow": 0}, (name, rule)
