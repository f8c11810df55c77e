"""Writes tests/golden/gray_7x17_{u8,u16,yfull}.jpg: the files tests/gray_ref.py makes
from seeded random 7 x 17 planes with all-ones quantisation tables -- uint8 AS_RGB,
uint16 at maxval 1023, uint8 Y_FULL_RANGE (the recipe of
tests/test_gray_reference.py::test_goldens, which compares byte for byte).

    python tests/golden/make_gray_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import gray_ref  # noqa: E402

W, H = 7, 17
ONES = [1] * 64
# name -> (dtype, maxval, transfer, seed)
KINDS = {"u8": (np.uint8, 255, gray_ref.AS_RGB, 1710), "u16": (np.uint16, 1023, gray_ref.AS_RGB, 1711),
         "yfull": (np.uint8, 255, gray_ref.Y_FULL_RANGE, 1712)}


def golden_path(kind):
    return os.path.join(HERE, f"gray_{W}x{H}_{kind}.jpg")


def plane(kind):
    dtype, maxval, _, seed = KINDS[kind]
    return np.random.default_rng(seed).integers(0, maxval + 1, (H, W)).astype(dtype)


def make(kind):
    _, maxval, transfer, _ = KINDS[kind]
    return gray_ref.encode(plane(kind), maxval, ONES, transfer)


if __name__ == "__main__":
    for k in KINDS:
        with open(golden_path(k), "wb") as f:
            f.write(make(k))
        print(golden_path(k))
