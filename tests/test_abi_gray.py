"""CPU-side checks of the grayscale input ABI (dmmt_device_gray, dmmt_gray_image,
dmmt_encode_device_gray, dmmt_jpeg_encode_gray, dmmt_gray_span,
dmmt_max_gray_jpeg_bytes): the ctypes mirrors have the header's size and field
offsets (a C program compiled from include/dmmt_jpeg.h prints them), the span and
the size bound have their values, the exported symbols refuse what is decided
before a device is needed.  That is the NULL cases only: like dmmt_encode_device_ycc
(tests/test_abi_ycc.py) the entry points resolve their context first, and without a
GPU there is none, so every other invalid description is refused in
tests/test_gpu_gray.py::test_invalid_arguments."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dmmt_jpeg
from conftest import ROOT

FIELDS = ["d_plane", "row_pitch", "frame_stride", "n_frames", "transfer", "width", "height", "maxval", "sample_bytes",
          "d_out", "out_stride", "d_out_len"]
IMAGE_FIELDS = ["width", "height", "maxval", "sample_bytes", "gray", "transfer"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    return dmmt_jpeg.lib()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(dmmt_device_gray, {f}));\n' for f in FIELDS)
    prints += "".join(f'    printf("image_{f} %zu\\n", offsetof(dmmt_gray_image, {f}));\n' for f in IMAGE_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmt_jpeg.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(dmmt_device_gray));\n'
                   '    printf("image_sizeof %zu\\n", sizeof(dmmt_gray_image));\n' + prints +
                   '    printf("transfers %d %d\\n", DMMT_GRAY_AS_RGB, DMMT_GRAY_Y_FULL_RANGE);\n'
                   '    printf("abi %d\\n", DMMT_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    S, I = dmmt_jpeg.DmmtDeviceGray, dmmt_jpeg.DmmtGrayImage
    assert int(out["sizeof"]) == ctypes.sizeof(S) and int(out["image_sizeof"]) == ctypes.sizeof(I)
    assert [f for f, _ in S._fields_] == FIELDS and [f for f, _ in I._fields_] == IMAGE_FIELDS
    for f in FIELDS:
        assert int(out[f]) == getattr(S, f).offset, f
    for f in IMAGE_FIELDS:
        assert int(out["image_" + f]) == getattr(I, f).offset, f
    T = dmmt_jpeg.GrayTransfer
    assert out["transfers"].split() == [str(int(T.AS_RGB)), str(int(T.Y_FULL_RANGE))]
    assert out["abi"] == "1"  # additive: the ABI version stays


@pytest.mark.parametrize("sb", [1, 2, 4])
def test_span(L, sb):
    for w, h in ((257, 33), (256, 32), (1, 1), (7, 17), (65535, 3)):
        for pitch in (w * sb, (w + 1) * sb, (w + 13) * sb, (1 << 30)):
            g = dmmt_jpeg.Encoder.gray(16, pitch, 1, w, h, sample_bytes=sb)
            assert dmmt_jpeg.gray_span(g) == (h - 1) * pitch + w * sb, (w, h, pitch)


def test_span_of_an_unsupported_description_is_zero(L):
    for sb, w, h in ((0, 16, 16), (3, 16, 16), (8, 16, 16), (1, 0, 16), (1, 16, 0)):
        assert dmmt_jpeg.gray_span(dmmt_jpeg.Encoder.gray(16, 4096, 1, w, h, sample_bytes=sb)) == 0, (sb, w, h)
    assert L.dmmt_gray_span(None) == 0


def test_max_gray_jpeg_bytes(L):
    # header bound + two bytes per worst-case scan byte (31 * 64 bits per block) + per
    # block a stuffed pad byte and an RST marker + EOI and slack: jpeg_common.hpp's
    # max_jpeg_bytes for one block per MCU
    header = 2 + 18 + 2 * 69 + 19 + 4 * (4 + 17 + 256) + 6 + 14
    for w, h in ((1, 1), (7, 17), (8, 8), (257, 33), (3840, 2160), (65535, 65535)):
        nb = -(-w // 8) * -(-h // 8)
        want = header + 2 * ((nb * 31 * 64 + 7) // 8) + 4 * nb + 2 + 64
        assert dmmt_jpeg.max_gray_jpeg_bytes(w, h) == want, (w, h)
        assert 0 < dmmt_jpeg.max_gray_jpeg_bytes(w, h) <= dmmt_jpeg.max_jpeg_bytes(w, h, 0), (w, h)
    assert dmmt_jpeg.max_gray_jpeg_bytes(0, 16) == 0 and dmmt_jpeg.max_gray_jpeg_bytes(16, 0) == 0


def test_new_symbols_are_exported_and_refuse_null(L):
    for name in ("dmmt_encode_device_gray", "dmmt_gray_span", "dmmt_max_gray_jpeg_bytes", "dmmt_jpeg_encode_gray"):
        assert hasattr(L, name), name
    for name in ("GrayTransfer", "DmmtDeviceGray", "gray_span", "max_gray_jpeg_bytes"):
        assert hasattr(dmmt_jpeg, name), name
    for name in ("gray", "encode_device_gray", "encode_gray"):
        assert hasattr(dmmt_jpeg.Encoder, name), name
    # argument checks that need no device: a NULL context, description or result
    g = dmmt_jpeg.DmmtDeviceGray()
    im = dmmt_jpeg.DmmtGrayImage()
    o = dmmt_jpeg.DmmtOptions()
    L.dmmt_default_options(ctypes.byref(o))
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.dmmt_encode_device_gray(None, ctypes.byref(g), ctypes.byref(o), None) == -102
    assert L.dmmt_jpeg_encode_gray(None, ctypes.byref(im), ctypes.byref(o), ctypes.byref(out), ctypes.byref(n)) == -102
