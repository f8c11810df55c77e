"""CPU unit check of k_front_ycc_sub's staging (csrc/ycc_load.hpp's tile with chroma
planes finer than the file, compiled for the host from the kernel's own header): tiles
replayed over one recording byte array per plane for the three converting pairs, uint8
and uint16 samples, planar and pair planes, every misalignment (another one per
plane), luma widths around 256, 1-3 rows (and 17 and 48: tiles below the first, and the
interior path), tight and wider pitches that differ between luma and chroma.  No address
outside a plane's span may be touched, the spans being those of the planes' own
sampling; interior tiles are whole loads; a staged row is the rectangle's samples, then
the pad code of its plane.  With the bound widened on purpose the check must find the
access.  The program is also built with the address and undefined-behaviour sanitizers
(a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ycc_sub_load_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ycc_sub") / "ycc_sub_load_check")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, SRC], check=True)
    return exe


def test_loader_stays_inside_the_spans_and_stages_rows_then_the_pad_code(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:")


def test_widened_bound_is_caught(checker):
    r = subprocess.run([checker, "--no-span-check"], capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    assert "FAIL: out-of-span access at plane offset" in r.stdout, r.stdout


def sanitizers_available():
    """decided before the check is built: this g++ links a trivial program with both runtimes"""
    if shutil.which("g++") is None:
        return False
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", os.path.join(d, "probe"), src],
                           capture_output=True)
        return r.returncode == 0


@pytest.mark.skipif(not sanitizers_available(), reason="this g++ has no sanitizer runtimes")
def test_loader_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ycc_sub_load_check_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, "-o", exe,
                    SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:")
