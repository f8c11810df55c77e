"""What fits on a CU beside k_front, read from the built library's gfx950 code
object (no GPU needed).  A context of several lanes keeps two k_front workgroups on
nearly every CU nearly all the time ("what fits beside k_front"), and
the other lanes' kernels share what those leave: with the bench's instantiations,
two workgroups of k_front_n<1, 1, uint8_t> plus five of k_emit_n<8> must fit a
SIMD's 512 VGPRs and the CU's LDS, and none of them may use scratch."""
import importlib.util
import os
import re
import struct
import subprocess
import tempfile

import pytest

import dmmt_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VGPRS_PER_SIMD = 512       # one file per SIMD, arch + acc; a 256-thread workgroup puts one wave on each SIMD
VGPR_GRANULE = 8           # registers per lane a wave's allocation is rounded up to
LDS_PER_CU = 160 * 1024
# Bytes a workgroup's LDS allocation is rounded up to.  The code object's descriptor
# counts LDS in blocks of 128 dwords (512 bytes) on gfx9; with the 160 KiB of gfx950 the
# same field counts blocks of 320 dwords.  The larger one is used here: a set of
# workgroups that fits under 1,280 also fits under 512.
LDS_GRANULE = 1280

FRONT = r"\d+k_front_nILi1ELi1EhLi\d+EE"  # k_front_n<1, 1, uint8_t, WPE>
EMIT8 = r"\d+k_emit_nILi8EE"
EMIT7 = r"\d+k_emit_nILi7EE"
HIST = r"\d+k_hist_nILb0ELb1EE"           # k_hist_n<false, true>


@pytest.fixture(scope="module")
def kernels():
    """mangled name -> its resource counts, for every kernel of the library"""
    spec = importlib.util.spec_from_file_location("last_vgpr_check", os.path.join(ROOT, "tools", "last_vgpr_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    out = {}
    for co in tool.code_objects(dmmt_jpeg.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(tool.LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True,
                                   text=True, check=True).stdout
            allocated = descriptor_vgprs(tool, f.name, co)
        for block in re.split(r"\n\s+- \.", notes):  # one block per kernel, its keys in any order
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and re.search(r"\.vgpr_count:", block):
                out[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                                      for k in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
                out[name.group(1)]["allocated_vgprs"] = allocated[name.group(1)]
    return out


def descriptor_vgprs(tool, path, co):
    """kernel -> the registers per lane the hardware allocates to a wave: the kernel
    descriptor's granulated count (compute_pgm_rsrc1 bits 0-5, at byte 48 of the 64-byte
    descriptor NAME.kd), in granules of VGPR_GRANULE.  The metadata's .vgpr_count is what
    the code uses; the compiler may ask for more, to hold the occupancy at what the LDS
    allows, and then that is what a wave takes from the SIMD's file."""
    readelf = os.path.join(tool.LLVM, "llvm-readelf")
    sections = {}  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", subprocess.run(
            [readelf, "-S", "-W", path], capture_output=True, text=True, check=True).stdout, re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for line in subprocess.run([readelf, "-s", "-W", path], capture_output=True, text=True, check=True).stdout.splitlines():
        w = line.split()
        if len(w) == 8 and w[7].endswith(".kd") and w[6].isdigit():
            addr, off = sections[int(w[6])]
            rsrc1 = struct.unpack_from("<I", co, off + int(w[1], 16) - addr + 48)[0]
            out[w[7][:-3]] = ((rsrc1 & 0x3F) + 1) * VGPR_GRANULE
    return out


def one(kernels, pattern):
    found = [v for k, v in kernels.items() if re.search(pattern, k)]
    assert len(found) == 1, (pattern, found)
    return found[0]


def regs(k):
    assert k["allocated_vgprs"] >= k["vgpr_count"]
    return k["allocated_vgprs"]


def lds(k):
    return -(-k["group_segment_fixed_size"] // LDS_GRANULE) * LDS_GRANULE


def beside_two_fronts(front, other):
    """workgroups of `other` that fit a CU beside two of `front`"""
    return min((VGPRS_PER_SIMD - 2 * regs(front)) // regs(other), (LDS_PER_CU - 2 * lds(front)) // max(lds(other), 1))


def test_five_k_emit_workgroups_fit_beside_two_k_front(kernels):
    front, emit = one(kernels, FRONT), one(kernels, EMIT8)
    print("k_front_n<1,1,u8>", front, "k_emit_n<8>", emit)
    assert 2 * regs(front) + 5 * regs(emit) <= VGPRS_PER_SIMD
    assert 2 * lds(front) + 5 * lds(emit) <= LDS_PER_CU
    assert beside_two_fronts(front, emit) >= 5


def test_the_front_kernel_meets_its_targets(kernels):
    front = one(kernels, FRONT)
    assert front["vgpr_count"] <= 96 and front["allocated_vgprs"] <= 96
    assert front["group_segment_fixed_size"] <= 33280


# every uint8 4:4:4 front kernel: tight (k_front), surfaces (k_front_surf: layouts 1 RGB / BGR and
# 3 planar), YCbCr (k_front_ycc: plain; levels and matrix kinds with one-byte samples), wide and narrow
U8_444 = [r"\d+k_front(_n)?ILi1ELi1EhLi\d+EE", r"\d+k_front_surf(_n)?ILi1ELi1EhLi[13]ELi\d+EE",
          r"\d+k_front_ycc(_n)?ILi1ELi1ELi\dELi\d+EE", r"\d+k_front_ycc_lv(_n)?INS_\w+ELi1ELi1ELi\dELi1ELi\d+EE"]
# RGBX / BGRX (layout 2) stages rows a third longer: 34,432 bytes, four workgroups per CU, and the
# compiler pads its allocation to 104 registers; it stays outside the target
RGBX_444 = r"\d+k_front_surf(_n)?ILi1ELi1EhLi2ELi\d+EE"


def test_every_u8_444_front_kernel_meets_the_targets(kernels):
    seen = 0
    for pattern, least in zip(U8_444, (2, 4, 6, 12)):
        found = {k: v for k, v in kernels.items() if re.search(pattern, k)}
        assert len(found) >= least, (pattern, sorted(found))
        for name, k in found.items():
            assert k["allocated_vgprs"] <= 96 and k["group_segment_fixed_size"] <= 33280, (name, k)
            assert k["private_segment_fixed_size"] == 0, name
            seen += 1
    print(seen, "kernels")
    for name, k in kernels.items():
        if re.search(RGBX_444, name):
            assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] <= 34432, (name, k)


def test_no_front_kernel_uses_scratch(kernels):
    front = {k: v for k, v in kernels.items() if "k_front" in k}
    assert len(front) >= 200
    assert [k for k, v in front.items() if v["private_segment_fixed_size"]] == []


def test_no_scratch(kernels):
    for pattern in (FRONT, EMIT8, EMIT7, HIST):
        assert one(kernels, pattern)["private_segment_fixed_size"] == 0, pattern


def test_the_table_of_design_3(kernels):
    """the counts DESIGN.md 3 records beside two k_front_n<1, 1, uint8_t> workgroups"""
    front = one(kernels, FRONT)
    got = {name: beside_two_fronts(front, one(kernels, pattern))
           for name, pattern in (("k_emit_n<8>", EMIT8), ("k_emit_n<7>", EMIT7), ("k_hist_n", HIST))}
    print(got)
    assert got == {"k_emit_n<8>": 5, "k_emit_n<7>": 4, "k_hist_n": 6}
