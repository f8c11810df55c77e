"""CPU unit check of the front kernels' two shortcut quantisers (csrc/dct_quant.hpp,
compiled for the host from the kernel's own header by tests/native/quant_check.cpp):
quantize_col8_scaled (integer samples, the YCbCr front) and quantize_col8
(Image<f32> dots) against quantizer.rs:60 computed in double, for every q in 1..255
and every row scaling, +-24 ulps around the half-integer quotients (0.5 .. 2049.5;
for the f32 path 0.5 .. 4096.5, the i16 ends and the 2^22 limit of its fast path), a
few million random inputs and, for the f32 path, zeros, denormals, FLT_MAX, Inf, NaN
and random bit patterns.

Not one lane may differ.  So that this cannot pass vacuously the program also counts
the lanes the header kept on its fast path, the lanes it redid with the division, and
the lanes whose fast value is wrong -- each count must be above 0 and every lane of
the last kind must have been redone.  Built once more with the margins removed, the
check must find wrong coefficients."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "quant_check.cpp")
FLAGS = ["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"]
NO_MARGINS = ["-DDMMT_QUANT_F32_BAND=0.0f", "-DDMMT_QUANT_SCALED_BAND=0.0f", "-DDMMT_QUANT_SCALED_HALF=0.5f"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def counts(stdout, path):
    line = [ln for ln in stdout.splitlines() if ln.startswith(path + ":")]
    assert len(line) == 1, stdout
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line[0])}


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    d = tmp_path_factory.mktemp("quant")

    def make(name, extra):
        exe = str(d / name)
        subprocess.run(FLAGS + extra + ["-o", exe, SRC], check=True)
        return exe
    return make


@pytest.fixture(scope="module")
def sweep(build):
    r = subprocess.run([build("quant_check", [])], capture_output=True, text=True)
    return r


@pytest.mark.parametrize("path", ["scaled", "f32"])
def test_both_quantisers_equal_the_division_at_every_half_integer(sweep, path):
    assert sweep.returncode == 0, sweep.stdout + sweep.stderr
    assert sweep.stdout.rstrip().endswith("ok")
    c = counts(sweep.stdout, path)
    print(path, c)
    assert c["mismatches"] == 0
    assert c["exact_path_wrong"] == 0       # the header's quantize() is round(d / q) itself
    assert c["fast"] > 0 and c["redone"] > 0
    assert c["fast"] + c["redone"] == c["lanes"] > 50_000_000
    assert c["fast_differs"] > 0            # the sweep reached lanes where the margin decides
    assert c["fast_differs_not_redone"] == 0


def test_removed_margins_are_caught(build):
    # (every 8th q is enough to fail)
    r = subprocess.run([build("quant_check_no_margins", NO_MARGINS), "8"], capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    assert "FAIL: a shortcut quantiser departs from round(d / q)" in r.stdout
    for path in ("scaled", "f32"):
        c = counts(r.stdout, path)
        assert c["mismatches"] > 0 and c["fast_differs_not_redone"] > 0, (path, c)
        assert c["exact_path_wrong"] == 0
