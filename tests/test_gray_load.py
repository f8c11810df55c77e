"""CPU unit check of k_front_gray's staging (csrc/gray_load.hpp, compiled for the
host from the kernel's own header): which 16-byte chunks cover a tile row, which
are loaded whole, which byte by byte and what the bytes past the rectangle become,
replayed over a byte array for misalignments 0-15, samples of 1, 2 and 4 bytes,
widths around 256, 1-24 rows (tiles below the first, and the interior path), tight,
+1 and +13 sample pitches.  No address outside the plane's span may be touched; a
staged row is the rectangle's bytes then 0.  With the bound widened on purpose the
check must find the access."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "gray_load_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gray") / "gray_load_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC], check=True)
    return exe


def test_loader_stays_inside_the_span_and_stages_rows_then_zero(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:")


def test_widened_bound_is_caught(checker):
    r = subprocess.run([checker, "--no-span-check"], capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    assert "FAIL: out-of-span access at plane offset" in r.stdout, r.stdout
