"""CPU-side checks of the device-surface ABI (dmmt_device_surfaces,
dmmt_encode_device_surfaces, dmmt_surface_span): the ctypes mirror has the
header's size and field offsets (a C program compiled from include/dmmt_jpeg.h
prints them), the span of every format, the exported symbols."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg
from conftest import ROOT

FIELDS = ["d_plane", "row_pitch", "frame_stride", "n_frames", "format", "width", "height", "maxval", "sample_bytes",
          "d_out", "out_stride", "d_out_len"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    return dmmt_jpeg.lib()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(dmmt_device_surfaces, {f}));\n' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmt_jpeg.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(dmmt_device_surfaces));\n' + prints +
                   '    printf("formats %d %d %d %d %d\\n", DMMT_PF_RGB, DMMT_PF_BGR, DMMT_PF_RGBX, DMMT_PF_BGRX, '
                   'DMMT_PF_PLANAR);\n    printf("abi %d\\n", DMMT_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    S = dmmt_jpeg.DmmtDeviceSurfaces
    assert int(out["sizeof"]) == ctypes.sizeof(S)
    assert [f for f, _ in S._fields_] == FIELDS
    for f in FIELDS:
        assert int(out[f]) == getattr(S, f).offset, f
    P = dmmt_jpeg.PixelFormat
    assert out["formats"].split() == [str(int(x)) for x in (P.RGB, P.BGR, P.RGBX, P.BGRX, P.PLANAR)]
    assert out["abi"] == "1"  # additive: the ABI version stays


@pytest.mark.parametrize("fmt,sb,spp", [(0, 1, 3), (1, 1, 3), (0, 2, 3), (1, 4, 3), (2, 1, 4), (3, 1, 4), (4, 1, 1),
                                        (4, 4, 1)])
def test_surface_span(L, fmt, sb, spp):
    w, h = 257, 33
    tight = w * spp * sb
    for pitch in (tight, tight + sb, tight + 16, (1 << 20) + 3 * sb):
        s = dmmt_jpeg.Encoder.surfaces(16, fmt, pitch, 1, w, h, sample_bytes=sb)
        assert dmmt_jpeg.surface_span(s) == (h - 1) * pitch + tight
    s = dmmt_jpeg.Encoder.surfaces(16, fmt, tight, 1, w, 1, sample_bytes=sb)
    assert dmmt_jpeg.surface_span(s) == tight


def test_surface_span_of_an_unsupported_surface_is_zero(L):
    for fmt, sb in ((2, 2), (3, 4), (4, 2), (5, 1), (-1, 1), (0, 3)):
        assert dmmt_jpeg.surface_span(dmmt_jpeg.Encoder.surfaces(16, fmt, 4096, 1, 16, 16, sample_bytes=sb)) == 0
    assert L.dmmt_surface_span(None) == 0


def test_new_symbols_are_exported(L):
    for name in ("dmmt_encode_device_surfaces", "dmmt_surface_span"):
        assert hasattr(L, name), name
    # argument checks that need no device: a NULL context or surface
    s = dmmt_jpeg.DmmtDeviceSurfaces()
    o = dmmt_jpeg.DmmtOptions()
    L.dmmt_default_options(ctypes.byref(o))
    assert L.dmmt_encode_device_surfaces(None, ctypes.byref(s), ctypes.byref(o), None) == -102
