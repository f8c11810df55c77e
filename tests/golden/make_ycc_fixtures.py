"""Writes tests/golden/ycc_7x17_P4{44,22,20}.jpg: the files tests/ycc_ref.py makes
from seeded random 7 x 17 YCbCr planes with all-ones quantisation tables (the
recipe of tests/test_ycc_reference.py::test_goldens, which compares byte for byte).

    python tests/golden/make_ycc_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ycc_ref  # noqa: E402

W, H = 7, 17
ONES = [1] * 64
NAMES = {0: "P444", 1: "P422", 2: "P420"}


def seed(sub):
    return 1700 + sub


def golden_path(sub):
    return os.path.join(HERE, f"ycc_{W}x{H}_{NAMES[sub]}.jpg")


def make(sub):
    return ycc_ref.encode(*ycc_ref.random_planes(W, H, sub, seed(sub)), sub, ONES, ONES)


if __name__ == "__main__":
    for s in NAMES:
        with open(golden_path(s), "wb") as f:
            f.write(make(s))
        print(golden_path(s))
