"""Writes tests/golden/ycc_subsample_7x17_*.jpg: the files tests/ycc_subsample_ref.py
makes from seeded random 7 x 17 YCbCr planes with all-ones quantisation tables (the
recipe of tests/test_ycc_subsample_reference.py::test_goldens, which compares byte for
byte): 4:4:4 uint8 full-range planes as a 4:2:0 file, 4:2:2 P210 (10 bits at the top of a
uint16, limited range) BT.709 planes as a 4:2:0 file, 4:4:4 I010 full-range BT.2020 planes
as a 4:2:2 file.

    python tests/golden/make_ycc_subsample_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ycc_levels_ref as lv  # noqa: E402
import ycc_matrix_ref as mx  # noqa: E402
import ycc_subsample_ref as ss  # noqa: E402

W, H = 7, 17
ONES = [1] * 64
# name: (planes' sampling, file's sampling, matrix, bit_depth, shift, range)
CASES = {"444_to_420_8F": (0, 2, mx.JFIF, 8, 0, lv.FULL), "422_to_420_709_P210L": (1, 2, mx.BT709, 10, 6, lv.LIMITED),
         "444_to_422_2020_10F": (0, 1, mx.BT2020, 10, 0, lv.FULL)}


def seed(name):
    return 2900 + sorted(CASES).index(name)


def golden_path(name):
    return os.path.join(HERE, f"ycc_subsample_{W}x{H}_{name}.jpg")


def make(name):
    src, sub, matrix, depth, shift, rng = CASES[name]
    planes = lv.random_planes(W, H, src, seed(name), depth, shift)
    return ss.encode(*planes, src, sub, ONES, ONES, matrix, depth, shift, rng)


if __name__ == "__main__":
    for n in CASES:
        with open(golden_path(n), "wb") as f:
            f.write(make(n))
        print(golden_path(n))
