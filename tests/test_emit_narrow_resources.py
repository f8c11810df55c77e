"""The narrow-form kernels' residency, read from the built library's gfx950 code
object (no GPU needed).  k_emit_n<8> must fit eight workgroups of 256 threads per CU
like k_emit<8>: at most 64 VGPRs, 20,480 bytes of LDS, no scratch.  k_hist_n runs
at eight waves per SIMD (at most 64 VGPRs) and must not spill either."""
import importlib.util
import os
import re
import subprocess
import tempfile

import dmmt_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _kernels(pattern):
    spec = importlib.util.spec_from_file_location("last_vgpr_check", os.path.join(ROOT, "tools", "last_vgpr_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    found = {}
    for co in tool.code_objects(dmmt_jpeg.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(tool.LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True,
                                   text=True, check=True).stdout
        for block in re.split(r"\n\s+- \.", notes):  # one block per kernel, its keys in any order
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and re.search(pattern, name.group(1)):
                found[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in KEYS}
    return found


def test_k_emit_n_fits_eight_workgroups_per_cu():
    found = _kernels(r"\d+k_emit_nILi8EE")
    print(found)
    assert len(found) == 1, found
    md = next(iter(found.values()))
    assert md["vgpr_count"] <= 64
    assert md["group_segment_fixed_size"] <= 20480
    assert md["private_segment_fixed_size"] == 0


def test_k_hist_n_eight_waves_no_scratch():
    found = _kernels(r"\d+k_hist_nILb")
    print(found)
    assert len(found) == 2, found  # with and without the fused tables
    for md in found.values():
        assert md["vgpr_count"] <= 64
        assert md["private_segment_fixed_size"] == 0
