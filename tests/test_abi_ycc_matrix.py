"""Checks of the YCbCr matrix ABI (dmmt_ycc_matrix, dmmt_encode_device_ycc_matrix,
dmmt_ycc_matrix_coefficients) without a device: the exported symbols, the enum values
and the ctypes mirrors against the header (a C program compiled from
include/dmmt_jpeg.h prints them), the coefficient helper's answers and its refusals."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg
import ycc_matrix_ref as mx
from conftest import ROOT
from dmmt_jpeg import YccMatrix as M


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    return dmmt_jpeg.lib()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_enum_and_structs_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmt_jpeg.h"\n'
                   '/* the prototypes again: a declaration that differs from the header\'s does not compile */\n'
                   'int dmmt_encode_device_ycc_matrix(dmmt_ctx*, const dmmt_device_ycc*, const dmmt_ycc_levels*,\n'
                   '                                  int32_t, const dmmt_options*, void*);\n'
                   'int dmmt_ycc_matrix_coefficients(int32_t, float*);\n'
                   'int main(void) {\n'
                   '    printf("matrices %d %d %d\\n", DMMT_YCC_MATRIX_JFIF, DMMT_YCC_MATRIX_BT709, DMMT_YCC_MATRIX_BT2020);\n'
                   '    printf("levels %zu\\n", sizeof(dmmt_ycc_levels));\n'
                   '    printf("ycc %zu\\n", sizeof(dmmt_device_ycc));\n'
                   '    printf("abi %d\\n", DMMT_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert out["matrices"].split() == [str(int(M.JFIF)), str(int(M.BT709)), str(int(M.BT2020))] == ["0", "1", "2"]
    assert (mx.JFIF, mx.BT709, mx.BT2020) == (0, 1, 2)
    assert int(out["levels"]) == ctypes.sizeof(dmmt_jpeg.DmmtYccLevels)  # both structs stay as they are
    assert int(out["ycc"]) == ctypes.sizeof(dmmt_jpeg.DmmtDeviceYcc)
    assert out["abi"] == "1"  # additive: the ABI version stays


def test_new_symbols_are_exported(L):
    for name in ("dmmt_encode_device_ycc_matrix", "dmmt_ycc_matrix_coefficients"):
        assert hasattr(L, name), name
    for name in ("YccMatrix", "ycc_matrix_coefficients"):
        assert hasattr(dmmt_jpeg, name), name
    # argument checks that need no device: a NULL context or description
    y = dmmt_jpeg.DmmtDeviceYcc()
    lv = dmmt_jpeg.DmmtYccLevels(1, 10, 2, 6)
    o = dmmt_jpeg.DmmtOptions()
    L.dmmt_default_options(ctypes.byref(o))
    for m in (M.JFIF, M.BT709, M.BT2020, 3):
        assert L.dmmt_encode_device_ycc_matrix(None, ctypes.byref(y), ctypes.byref(lv), int(m), ctypes.byref(o),
                                               None) == -102
        assert L.dmmt_encode_device_ycc_matrix(None, None, None, int(m), ctypes.byref(o), None) == -102


def test_the_python_signatures_default_to_jfif():
    import inspect
    for f in (dmmt_jpeg.Encoder.encode_device_ycc, dmmt_jpeg.Encoder.encode_ycc):
        p = inspect.signature(f).parameters["matrix"]
        assert p.default == M.JFIF == 0


def test_coefficients(L):
    for m in mx.MATRICES:
        out = (ctypes.c_float * 6)()
        assert L.dmmt_ycc_matrix_coefficients(m, out) == 0
        assert [float(x) for x in out] == [float(x) for x in mx.constants(m)]
        assert tuple(out) == dmmt_jpeg.ycc_matrix_coefficients(m)


def test_coefficients_of_an_unknown_matrix_are_refused(L):
    out = (ctypes.c_float * 6)(*[7.0] * 6)
    for bad in (0, 3, -1, 255, 1 << 30):  # (0: JFIF is no step and has no constants)
        assert L.dmmt_ycc_matrix_coefficients(bad, out) == -102, bad
        assert list(out) == [7.0] * 6  # untouched
        with pytest.raises(dmmt_jpeg.Error) as e:
            dmmt_jpeg.ycc_matrix_coefficients(bad)
        assert e.value.code == -102
    assert L.dmmt_ycc_matrix_coefficients(int(M.BT709), None) == -102
