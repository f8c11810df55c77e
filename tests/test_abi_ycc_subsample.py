"""Checks of the ABI of dmmt_encode_device_ycc_subsample (YCbCr planes finer than the
file): the exported symbol and its prototype against the header (a C program compiled
from include/dmmt_jpeg.h), the Python signatures, and -- on a device -- the argument
errors: upsampling pairs, a chroma pitch below the PLANES' row, an out_stride below the
FILE's bound, an unknown matrix or levels, and the three older calls still refusing a
sampling that differs from the file's."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg
from conftest import ROOT
from dmmt_jpeg import DmmtYccLevels as Lv
from dmmt_jpeg import YccMatrix as M
from dmmt_jpeg import YccRange as R

INVALID_ARGUMENT, CAPACITY = -102, -203
CONVERTING = [(0, 1), (0, 2), (1, 2)]   # (planes, file)
UPSAMPLING = [(1, 0), (2, 0), (2, 1)]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    return dmmt_jpeg.lib()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_prototype_matches_the_header(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text('#include <stdio.h>\n#include "dmmt_jpeg.h"\n'
                   '/* the prototype again: a declaration that differs from the header\'s does not compile */\n'
                   'int dmmt_encode_device_ycc_subsample(dmmt_ctx*, const dmmt_device_ycc*, const dmmt_ycc_levels*,\n'
                   '                                     int32_t, const dmmt_options*, void*);\n'
                   'int main(void) {\n'
                   '    printf("ycc %zu\\nabi %d\\n", sizeof(dmmt_device_ycc), DMMT_ABI_VERSION);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "proto"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert int(out["ycc"]) == ctypes.sizeof(dmmt_jpeg.DmmtDeviceYcc)  # the struct stays as it is
    assert out["abi"] == "1"  # additive: the ABI version stays


def test_the_symbol_is_exported(L):
    assert hasattr(L, "dmmt_encode_device_ycc_subsample")
    assert L.dmmt_encode_device_ycc_subsample.argtypes == L.dmmt_encode_device_ycc_matrix.argtypes
    # argument checks that need no device: a NULL context or description
    y = dmmt_jpeg.DmmtDeviceYcc()
    lv = Lv(1, 10, 2, 6)
    o = dmmt_jpeg.DmmtOptions()
    L.dmmt_default_options(ctypes.byref(o))
    for m in (M.JFIF, M.BT709, M.BT2020, 3):
        assert L.dmmt_encode_device_ycc_subsample(None, ctypes.byref(y), ctypes.byref(lv), int(m), ctypes.byref(o),
                                                  None) == INVALID_ARGUMENT
        assert L.dmmt_encode_device_ycc_subsample(None, None, None, int(m), ctypes.byref(o), None) == INVALID_ARGUMENT


def test_the_python_signatures_default_to_the_options_preset():
    for f in (dmmt_jpeg.Encoder.encode_device_ycc, dmmt_jpeg.Encoder.encode_ycc):
        assert inspect.signature(f).parameters["chroma_sampling"].default is None


@pytest.mark.gpu
def test_argument_errors(encoder):
    L = dmmt_jpeg.lib()
    w, h = 64, 16
    d = encoder.malloc(1 << 16)
    caps = [dmmt_jpeg.max_jpeg_bytes(w, h, s) for s in (0, 1, 2)]
    assert caps[0] > caps[1] > caps[2]
    d_out, d_len = encoder.malloc(caps[0]), encoder.malloc(4)
    P3 = [d, d + 8192, d + 16384]
    tables = dmmt_jpeg.quality_tables(90)

    def call(fn, src, sub, fmt=0, lp=w, cp=None, lv=None, matrix=M.JFIF, out_stride=None, sb=1):
        cw = -(-w // (1 if src == 0 else 2))
        cp = cw * (1 if fmt == 0 else 2) * sb if cp is None else cp
        y = dmmt_jpeg.Encoder.ycc(P3, fmt, lp * sb, cp, 1, w, h, src, d_out,
                                  caps[sub] if out_stride is None else out_stride, d_len)
        o = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=tables[0],
                                                chroma_table=tables[1]).to_c()
        lvp = ctypes.byref(Lv(*lv)) if lv is not None else None
        if fn == "subsample":
            return L.dmmt_encode_device_ycc_subsample(encoder.handle, ctypes.byref(y), lvp, int(matrix), ctypes.byref(o), None)
        if fn == "matrix":
            return L.dmmt_encode_device_ycc_matrix(encoder.handle, ctypes.byref(y), lvp, int(matrix), ctypes.byref(o), None)
        if fn == "levels":
            return L.dmmt_encode_device_ycc_levels(encoder.handle, ctypes.byref(y), lvp, ctypes.byref(o), None)
        return L.dmmt_encode_device_ycc(encoder.handle, ctypes.byref(y), ctypes.byref(o), None)
    p010 = (R.LIMITED, 10, 2, 6)
    try:
        for src, sub in CONVERTING + [(0, 0), (1, 1), (2, 2)]:
            for fmt in (0, 1, 2):
                assert call("subsample", src, sub, fmt) == 0, (src, sub, fmt)
            assert call("subsample", src, sub, 1, lv=p010, matrix=M.BT709, sb=2) == 0, (src, sub)
        for src, sub in UPSAMPLING:  # a file finer than the planes
            for matrix, lv, sb in ((M.JFIF, None, 1), (M.BT709, p010, 2)):
                assert call("subsample", src, sub, lv=lv, matrix=matrix, sb=sb) == INVALID_ARGUMENT, (src, sub)
        for bad in (3, -1, 7):  # a sampling that is none
            assert call("subsample", bad, 2, cp=w) == INVALID_ARGUMENT
        # the chroma pitch goes by the planes' row: 4:4:4 planes of a 4:2:0 file need w bytes, not w / 2
        assert call("subsample", 0, 2, cp=w - 1) == INVALID_ARGUMENT and call("subsample", 0, 2, cp=w // 2) == INVALID_ARGUMENT
        assert call("subsample", 0, 2, 1, cp=2 * w - 1) == INVALID_ARGUMENT and call("subsample", 0, 2, 1, cp=2 * w) == 0
        assert call("subsample", 1, 2, cp=w // 2 - 1) == INVALID_ARGUMENT and call("subsample", 1, 2, cp=w // 2) == 0
        assert call("subsample", 0, 1, 2, lv=p010, cp=4 * w - 2, sb=2) == INVALID_ARGUMENT
        # out_stride goes by the file's sampling: the 4:2:0 bound is enough for 4:4:4 planes, one byte less is not
        assert call("subsample", 0, 2, out_stride=caps[2]) == 0
        assert call("subsample", 0, 2, out_stride=caps[2] - 1) == CAPACITY
        assert call("subsample", 0, 1, out_stride=caps[1] - 1) == CAPACITY
        assert call("subsample", 1, 2, out_stride=caps[2] - 1) == CAPACITY
        for bad in (3, -1, 1 << 20):  # an unknown matrix
            assert call("subsample", 0, 2, matrix=bad) == INVALID_ARGUMENT
            assert call("subsample", 2, 2, matrix=bad) == INVALID_ARGUMENT
        for bad in ((2, 8, 1, 0), (R.FULL, 10, 1, 0), (R.FULL, 10, 2, 7), (R.LIMITED, 7, 2, 0), (R.FULL, 8, 3, 0)):
            assert call("subsample", 0, 2, lv=bad) == INVALID_ARGUMENT, bad
        assert call("subsample", 0, 2, lp=w + 1, cp=2 * w + 1, lv=p010, sb=2) == INVALID_ARGUMENT  # an odd chroma pitch
        # the three older calls refuse every mismatch as before
        for src, sub in CONVERTING + UPSAMPLING:
            assert call("plain", src, sub) == INVALID_ARGUMENT, (src, sub)
            assert call("levels", src, sub, lv=(R.LIMITED, 8, 1, 0)) == INVALID_ARGUMENT, (src, sub)
            assert call("matrix", src, sub, lv=p010, matrix=M.BT709, sb=2) == INVALID_ARGUMENT, (src, sub)
            assert call("matrix", src, sub) == INVALID_ARGUMENT, (src, sub)
        encoder.synchronize()
    finally:
        for p in (d, d_out, d_len):
            encoder.free(p)
