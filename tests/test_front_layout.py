"""CPU check of the front kernels' LDS layout of the row-transformed blocks
(csrc/front_layout.hpp, the kernels' own header compiled for the host by
tests/native/front_layout_check.cpp), in both its forms: the compact one of the
uint8 4:4:4 kernels (64 floats per block, no padding; checked for every geometry)
and the padded one of the others.  The mapping (block, row, column) -> float index
is injective inside sT, the compact form fills it exactly, and every phase A row
store and phase C column read of a wave costs no more bank-conflict cycles than
under the padded formula the check keeps for comparison -- none."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "front_layout_check.cpp")

# blocks per tile of each geometry: 32 MCUs of Y, Cb, Cr; 16 of Y, Y, Cb, Cr; 16 of four Y, Cb, Cr; 32 of Y
BLOCKS = {"444": 96, "422": 64, "420": 96, "gray": 32}
BLOCKS.update({k + "c": v for k, v in list(BLOCKS.items())})  # "c": the compact layout (in use: 444c)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("layout") / "front_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        out[w[0]] = {"blocks": int(w[2]), "floats": int(w[4]), "stores": int(w[6]), "store_conflicts": int(w[8]),
                     "store_padded": int(w[10]), "reads": int(w[12]), "read_conflicts": int(w[14]),
                     "read_padded": int(w[16])}
    return out


def test_every_geometry_is_checked(report):
    assert set(report) == set(BLOCKS)
    for name, nb in BLOCKS.items():
        assert report[name]["blocks"] == nb
        assert report[name]["floats"] == (64 * nb if name.endswith("c") else 72 * nb + 4)  # compact: no padding
        # per wave: two 16-byte stores per stored row, 8 reads per column job
        assert report[name]["reads"] == 4 * 8 * (nb * 8 // 256)
        assert report[name]["stores"] > 0


def test_no_more_conflicts_than_the_padded_layout(report):
    for name, r in report.items():
        assert r["store_conflicts"] <= r["store_padded"], name
        assert r["read_conflicts"] <= r["read_padded"], name
        # both layouts are conflict-free for these lane sets
        assert r["store_conflicts"] == 0 and r["read_conflicts"] == 0, (name, r)
