"""k_emit's residency on a CU, read from the built library's gfx950 code object
(no GPU needed): eight workgroups of 256 threads per CU need at most 512 / 8 = 64
VGPRs per wave and 160 KB / 8 = 20,480 bytes of LDS per workgroup, and a kernel
that spills to scratch is slower than one at seven per CU (DESIGN.md 3;
profiles/STUDIES.md I)."""
import importlib.util
import os
import re
import subprocess
import tempfile

import dmmt_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k_emit_metadata():
    spec = importlib.util.spec_from_file_location("last_vgpr_check", os.path.join(ROOT, "tools", "last_vgpr_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    if not os.path.exists(dmmt_jpeg.LIB_PATH):
        dmmt_jpeg.build()
    found = []
    for co in tool.code_objects(dmmt_jpeg.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(tool.LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True,
                                   text=True, check=True).stdout
        for block in re.split(r"\n\s+- \.", notes):  # one block per kernel, its keys in any order
            name = re.search(r"\.name:\s+(\S+)", block)
            # (k_emit<8>: the instantiation for eight per CU; k_emit<7> serves batched
            # launches from a context of several lanes, launch_emit)
            if name and re.search(r"\d+k_emitILi8EE", name.group(1)):
                found.append({k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                              for k in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert len(found) == 1, found
    return found[0]


def test_k_emit_fits_eight_workgroups_per_cu():
    md = _k_emit_metadata()
    print(md)
    assert md["vgpr_count"] <= 64
    assert md["group_segment_fixed_size"] <= 20480
    assert md["private_segment_fixed_size"] == 0
