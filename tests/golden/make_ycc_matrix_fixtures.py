"""Writes tests/golden/ycc_matrix_7x17_*.jpg: the files tests/ycc_matrix_ref.py makes
from seeded random 7 x 17 YCbCr planes with all-ones quantisation tables (the recipe
of tests/test_ycc_matrix_reference.py::test_goldens, which compares byte for byte):
4:2:0 BT.709 10-bit limited range (uint16, the bits at the top: shift 6), 4:4:4 BT.2020
8-bit full range (uint8), 4:2:2 BT.2020 10-bit full range (uint16, shift 0).

    python tests/golden/make_ycc_matrix_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ycc_levels_ref as lv  # noqa: E402
import ycc_matrix_ref as mx  # noqa: E402

W, H = 7, 17
ONES = [1] * 64
# name: (subsampling, matrix, bit_depth, shift, range)
CASES = {"P420_709_10L": (2, mx.BT709, 10, 6, lv.LIMITED), "P444_2020_8F": (0, mx.BT2020, 8, 0, lv.FULL),
         "P422_2020_10F": (1, mx.BT2020, 10, 0, lv.FULL)}


def seed(name):
    return 2800 + sorted(CASES).index(name)


def golden_path(name):
    return os.path.join(HERE, f"ycc_matrix_{W}x{H}_{name}.jpg")


def make(name):
    sub, matrix, depth, shift, rng = CASES[name]
    planes = lv.random_planes(W, H, sub, seed(name), depth, shift)
    return mx.encode(*planes, sub, ONES, ONES, matrix, depth, shift, rng)


if __name__ == "__main__":
    for n in CASES:
        with open(golden_path(n), "wb") as f:
            f.write(make(n))
        print(golden_path(n))
