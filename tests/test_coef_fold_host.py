"""CPU unit check of the escape predicate of k_front's narrow store
(csrc/coef_format.hpp: coef_column_escapes, which runs the kernel's own fold
coef_hi_mag on the column's values as floats): for every column, row and edge value
-- alone among zeros and among +-127 -- and for a million seeded random columns it
equals "coef_pack_block wrote an escape byte 0x80 in this column"
(tests/native/coef_fold_check.cpp)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "coef_fold_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_fold_predicate_equals_the_packed_escape_bytes(tmp_path):
    exe = str(tmp_path / "coef_fold_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", exe, SRC],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
