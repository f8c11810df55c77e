"""Writes tests/golden/ycc_levels_7x17_*.jpg: the files tests/ycc_levels_ref.py makes
from seeded random 7 x 17 YCbCr planes with all-ones quantisation tables (the recipe
of tests/test_ycc_levels_reference.py::test_goldens, which compares byte for byte):
4:2:0 10-bit limited range (uint16, the bits at the top: shift 6), 4:4:4 8-bit limited
range (uint8), 4:2:2 12-bit full range (uint16, shift 0).

    python tests/golden/make_ycc_levels_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ycc_levels_ref as lv  # noqa: E402

W, H = 7, 17
ONES = [1] * 64
# name: (subsampling, bit_depth, shift, range)
CASES = {"P420_10L": (2, 10, 6, lv.LIMITED), "P444_8L": (0, 8, 0, lv.LIMITED), "P422_12F": (1, 12, 0, lv.FULL)}


def seed(name):
    return 2700 + sorted(CASES).index(name)


def golden_path(name):
    return os.path.join(HERE, f"ycc_levels_{W}x{H}_{name}.jpg")


def make(name):
    sub, depth, shift, rng = CASES[name]
    planes = lv.random_planes(W, H, sub, seed(name), depth, shift)
    return lv.encode(*planes, sub, ONES, ONES, depth, shift, rng)


if __name__ == "__main__":
    for n in CASES:
        with open(golden_path(n), "wb") as f:
            f.write(make(n))
        print(golden_path(n))
