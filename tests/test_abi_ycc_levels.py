"""Checks of the YCbCr sample-levels ABI (dmmt_ycc_levels, dmmt_encode_device_ycc_levels,
dmmt_ycc_plane_span_levels): the ctypes mirror has the header's size and field offsets
(a C program compiled from include/dmmt_jpeg.h prints them), the span of every plane
of every format, subsampling and sample size, 0 for unsupported descriptions and
levels, the exported symbols -- all without a device -- and, on a device, the argument
errors of the encoding call."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg
from conftest import ROOT
from dmmt_jpeg import DmmtYccLevels as Lv
from dmmt_jpeg import YccRange as R

FIELDS = ["range", "bit_depth", "sample_bytes", "shift"]
# name: (bit_depth, sample_bytes, shift), the header's table
FORMATS = {"P010": (10, 2, 6), "P012": (12, 2, 4), "P016": (16, 2, 0), "I010": (10, 2, 0), "NV12 limited": (8, 1, 0)}
BAD_LEVELS = [(0, 8, 1, 1), (0, 10, 1, 0), (0, 7, 1, 0), (1, 9, 1, 0),  # uint8: 8 bits, shift 0
              (0, 7, 2, 0), (1, 17, 2, 0), (0, 0, 2, 0), (0, -1, 2, 0),  # uint16: 8..16 bits
              (0, 10, 2, 7), (1, 16, 2, 1), (0, 8, 2, 9), (0, 10, 2, -1),  # shift in 0..16-B
              (2, 8, 1, 0), (-1, 10, 2, 6),  # range
              (0, 8, 0, 0), (0, 8, 3, 0), (0, 16, 4, 0)]  # sample_bytes


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    return dmmt_jpeg.lib()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(dmmt_ycc_levels, {f}));\n' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmt_jpeg.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(dmmt_ycc_levels));\n' + prints +
                   '    printf("ycc %zu\\n", sizeof(dmmt_device_ycc));\n'
                   '    printf("ranges %d %d\\n", DMMT_YCC_RANGE_FULL, DMMT_YCC_RANGE_LIMITED);\n'
                   '    printf("abi %d\\n", DMMT_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(Lv) == 16
    assert [f for f, _ in Lv._fields_] == FIELDS
    for f in FIELDS:
        assert int(out[f]) == getattr(Lv, f).offset, f
    assert int(out["ycc"]) == ctypes.sizeof(dmmt_jpeg.DmmtDeviceYcc)  # dmmt_device_ycc stays as it is
    assert out["ranges"].split() == [str(int(R.FULL)), str(int(R.LIMITED))] == ["0", "1"]
    assert out["abi"] == "1"  # additive: the ABI version stays


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_plane_span(L, fmt, sub):
    hr, vr = (1 if sub == 0 else 2), (2 if sub == 2 else 1)
    for name, (depth, sb, shift) in FORMATS.items():
        for rng in (R.FULL, R.LIMITED):
            lv = Lv(rng, depth, sb, shift)
            for w, h in ((257, 33), (256, 32), (1, 1), (7, 17)):  # odd and even
                cw, ch = -(-w // hr), -(-h // vr)
                lrow, crow = w * sb, cw * (1 if fmt == 0 else 2) * sb
                for lp, cp in ((lrow, crow), (lrow + 2, crow + 16), (lrow + 16, crow + 2), ((1 << 20) + 6, (1 << 19) + 10)):
                    y = dmmt_jpeg.Encoder.ycc([16, 32, 48], fmt, lp, cp, 1, w, h, sub)
                    span = [dmmt_jpeg.ycc_plane_span_levels(y, lv, p) for p in (0, 1, 2, 3, -1)]
                    cspan = (ch - 1) * cp + crow
                    assert span == [(h - 1) * lp + lrow, cspan, cspan if fmt == 0 else 0, 0, 0], (name, w, h, lp, cp)


def test_null_levels_are_uint8_full_range(L):
    for fmt in (0, 1, 2):
        for sub in (0, 1, 2):
            y = dmmt_jpeg.Encoder.ycc([16, 32, 48], fmt, 300, 600, 1, 257, 33, sub)
            for p in range(4):
                want = dmmt_jpeg.ycc_plane_span(y, p)
                assert dmmt_jpeg.ycc_plane_span_levels(y, None, p) == want
                assert dmmt_jpeg.ycc_plane_span_levels(y, Lv(R.FULL, 8, 1, 0), p) == want
                assert dmmt_jpeg.ycc_plane_span_levels(y, Lv(R.LIMITED, 8, 1, 0), p) == want


def test_plane_span_of_an_unsupported_description_is_zero(L):
    lv = Lv(R.LIMITED, 10, 2, 6)
    for fmt, sub, w, h in ((3, 0, 16, 16), (-1, 0, 16, 16), (0, 3, 16, 16), (0, -1, 16, 16), (0, 0, 0, 16),
                           (0, 0, 16, 0)):
        y = dmmt_jpeg.Encoder.ycc([16, 32, 48], fmt, 4096, 4096, 1, w, h, sub)
        assert [dmmt_jpeg.ycc_plane_span_levels(y, lv, p) for p in range(3)] == [0, 0, 0], (fmt, sub, w, h)
    assert L.dmmt_ycc_plane_span_levels(None, ctypes.byref(lv), 0) == 0
    y = dmmt_jpeg.Encoder.ycc([16, 32, 48], 0, 4096, 4096, 1, 16, 16, 0)
    assert dmmt_jpeg.ycc_plane_span_levels(y, lv, 0) == 15 * 4096 + 32
    for bad in BAD_LEVELS:
        assert [dmmt_jpeg.ycc_plane_span_levels(y, Lv(*bad), p) for p in range(3)] == [0, 0, 0], bad


def test_new_symbols_are_exported(L):
    for name in ("dmmt_encode_device_ycc_levels", "dmmt_ycc_plane_span_levels"):
        assert hasattr(L, name), name
    # argument checks that need no device: a NULL context or description
    y = dmmt_jpeg.DmmtDeviceYcc()
    lv = Lv(R.LIMITED, 10, 2, 6)
    o = dmmt_jpeg.DmmtOptions()
    L.dmmt_default_options(ctypes.byref(o))
    assert L.dmmt_encode_device_ycc_levels(None, ctypes.byref(y), ctypes.byref(lv), ctypes.byref(o), None) == -102
    assert L.dmmt_encode_device_ycc_levels(None, ctypes.byref(y), None, ctypes.byref(o), None) == -102
    assert hasattr(dmmt_jpeg, "YccRange") and hasattr(dmmt_jpeg, "DmmtYccLevels")
    assert hasattr(dmmt_jpeg, "ycc_plane_span_levels")


@pytest.mark.gpu
def test_argument_errors(encoder):
    """odd pitches, strides and pointers with uint16 samples, levels out of range, and
    dmmt_encode_device_ycc's own checks with the rows' bytes doubled"""
    L = dmmt_jpeg.lib()
    w, h = 64, 16
    d = encoder.malloc(1 << 16)
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, 0)
    d_out, d_len = encoder.malloc(cap), encoder.malloc(4)
    P3 = [d, d + 8192, d + 16384]
    p010 = (R.LIMITED, 10, 2, 6)
    tables = dmmt_jpeg.quality_tables(90)

    def rc(planes, fmt, lp, cp, lv=p010, sub=0, fstride=0, out_stride=cap):
        y = dmmt_jpeg.Encoder.ycc(planes, fmt, lp, cp, 1, w, h, sub, d_out, out_stride, d_len, fstride)
        o = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=tables[0],
                                                chroma_table=tables[1]).to_c()
        lvp = ctypes.byref(Lv(*lv)) if lv is not None else None
        return L.dmmt_encode_device_ycc_levels(encoder.handle, ctypes.byref(y), lvp, ctypes.byref(o), None)
    try:
        assert rc(P3, 0, 2 * w, 2 * w) == 0 and rc(P3, 1, 2 * w, 4 * w) == 0 and rc([d, d + 8192, 0], 2, 2 * w, 4 * w) == 0
        assert rc(P3, 0, w, w, lv=None) == 0 and rc(P3, 0, w, w, lv=(R.LIMITED, 8, 1, 0)) == 0
        assert rc(P3, 0, 2 * w, 2 * w, fstride=4098) == 0
        assert rc(P3, 0, 2 * w + 1, 2 * w) == -102 and rc(P3, 0, 2 * w, 2 * w + 1) == -102   # odd pitches
        assert rc(P3, 0, 2 * w, 2 * w, fstride=4097) == -102                                  # odd frame stride
        for p in range(3):                                                                     # odd pointers
            planes = [q + (1 if i == p else 0) for i, q in enumerate(P3)]
            assert rc(planes, 0, 2 * w, 2 * w) == -102, p
        assert rc([d, d + 8193, 0], 1, 2 * w, 4 * w) == -102
        assert rc([d + 1, d + 8193, d + 16385], 0, w + 1, w + 1, lv=(R.LIMITED, 8, 1, 0)) == 0  # uint8: any alignment
        for bad in BAD_LEVELS:
            assert rc(P3, 0, 2 * w, 2 * w, lv=bad) == -102, bad
        assert rc(P3, 0, 2 * w - 2, 2 * w) == -102 and rc(P3, 0, 2 * w, 2 * w - 2) == -102    # pitches below the rows' bytes
        assert rc(P3, 1, 2 * w, 4 * w - 2) == -102 and rc(P3, 1, 2 * w, 2 * w - 2, sub=1) == -102
        assert rc(P3, 0, 2 * w, w, sub=2, out_stride=dmmt_jpeg.max_jpeg_bytes(w, h, 2)) == 0
        assert rc([0, d, d], 0, 2 * w, 2 * w) == -102 and rc([d, 0, d], 1, 2 * w, 4 * w) == -102
        assert rc(P3, 0, 2 * w, 2 * w, out_stride=cap - 1) == -203                             # DMMT_E_CAPACITY
        encoder.synchronize()
    finally:
        for p in (d, d_out, d_len):
            encoder.free(p)
