"""CPU-side checks of the YCbCr input ABI (dmmt_device_ycc, dmmt_encode_device_ycc,
dmmt_ycc_plane_span): the ctypes mirror has the header's size and field offsets (a
C program compiled from include/dmmt_jpeg.h prints them), the span of every plane
of every format and subsampling, the exported symbols."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg
from conftest import ROOT

FIELDS = ["d_plane", "luma_pitch", "chroma_pitch", "frame_stride", "n_frames", "format", "chroma_sampling", "width",
          "height", "d_out", "out_stride", "d_out_len"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    return dmmt_jpeg.lib()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(dmmt_device_ycc, {f}));\n' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmt_jpeg.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(dmmt_device_ycc));\n' + prints +
                   '    printf("formats %d %d %d\\n", DMMT_YCC_PLANAR, DMMT_YCC_NV, DMMT_YCC_NV_VU);\n'
                   '    printf("abi %d\\n", DMMT_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    S = dmmt_jpeg.DmmtDeviceYcc
    assert int(out["sizeof"]) == ctypes.sizeof(S)
    assert [f for f, _ in S._fields_] == FIELDS
    for f in FIELDS:
        assert int(out[f]) == getattr(S, f).offset, f
    F = dmmt_jpeg.YccFormat
    assert out["formats"].split() == [str(int(x)) for x in (F.PLANAR, F.NV, F.NV_VU)]
    assert out["abi"] == "1"  # additive: the ABI version stays


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_plane_span(L, fmt, sub):
    hr, vr = (1 if sub == 0 else 2), (2 if sub == 2 else 1)
    for w, h in ((257, 33), (256, 32), (1, 1), (7, 17)):  # odd and even
        cw, ch = -(-w // hr), -(-h // vr)
        crow = cw * (1 if fmt == 0 else 2)
        for lp, cp in ((w, crow), (w + 1, crow + 16), (w + 16, crow + 1), ((1 << 20) + 3, (1 << 19) + 5)):
            y = dmmt_jpeg.Encoder.ycc([16, 32, 48], fmt, lp, cp, 1, w, h, sub)
            assert dmmt_jpeg.ycc_plane_span(y, 0) == (h - 1) * lp + w
            assert dmmt_jpeg.ycc_plane_span(y, 1) == (ch - 1) * cp + crow
            assert dmmt_jpeg.ycc_plane_span(y, 2) == ((ch - 1) * cp + crow if fmt == 0 else 0)  # NV*: unused
            assert dmmt_jpeg.ycc_plane_span(y, 3) == 0 and dmmt_jpeg.ycc_plane_span(y, -1) == 0


def test_plane_span_of_an_unsupported_description_is_zero(L):
    for fmt, sub, w, h in ((3, 0, 16, 16), (-1, 0, 16, 16), (0, 3, 16, 16), (0, -1, 16, 16), (0, 0, 0, 16),
                           (0, 0, 16, 0)):
        y = dmmt_jpeg.Encoder.ycc([16, 32, 48], fmt, 4096, 4096, 1, w, h, sub)
        assert [dmmt_jpeg.ycc_plane_span(y, p) for p in range(3)] == [0, 0, 0], (fmt, sub, w, h)
    assert L.dmmt_ycc_plane_span(None, 0) == 0


def test_new_symbols_are_exported(L):
    for name in ("dmmt_encode_device_ycc", "dmmt_ycc_plane_span"):
        assert hasattr(L, name), name
    # argument checks that need no device: a NULL context or description
    y = dmmt_jpeg.DmmtDeviceYcc()
    o = dmmt_jpeg.DmmtOptions()
    L.dmmt_default_options(ctypes.byref(o))
    assert L.dmmt_encode_device_ycc(None, ctypes.byref(y), ctypes.byref(o), None) == -102
