"""CPU unit check of k_front_ycc's staging (csrc/ycc_load.hpp, compiled for the
host from the kernel's own header): which 16-byte chunks cover the luma and chroma
tile rows, which are loaded whole, which byte by byte and what the bytes past the
rectangle become, replayed over one byte array per plane for misalignments 0-15
(another one per plane), the three subsamplings, planar and pair planes, luma
widths around 256 and chroma widths around 128, 1-3 rows (and 17 and 48: tiles
below the first, and the interior path), tight, +1 and +16 pitches that differ
between luma and chroma.  No address outside a plane's span may be touched; a
staged luma row is the rectangle's bytes then 0, a staged chroma row the
rectangle's bytes then 0x80.  With the bound widened on purpose the check must
find the access."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ycc_load_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ycc") / "ycc_load_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC], check=True)
    return exe


def test_loader_stays_inside_the_spans_and_stages_rows_then_the_pad_sample(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:")


def test_widened_bound_is_caught(checker):
    r = subprocess.run([checker, "--no-span-check"], capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    assert "FAIL: out-of-span access at plane offset" in r.stdout, r.stdout
