#!/usr/bin/env python3
"""Resource table of the front kernels from two `make asm` outputs, parent beside new.

usage: front_resources.py PARENT_BUILD_DIR NEW_BUILD_DIR [CXXFILT]

For every kernel whose name contains k_front in kernels.s, front_ycc.s and
front_gray.s: VGPRs (.amdhsa_next_free_vgpr), LDS bytes, scratch bytes, instruction
lines and the resident workgroups per CU they allow -- a workgroup is four waves,
one per SIMD: min(160 KiB / LDS, 512 / roundup8(VGPR), 8).  Exit status 1 when a
kernel of the new build falls a class: fewer workgroups per CU, any scratch, other
LDS bytes, or -- compiled with a register budget (__launch_bounds__'s second
argument, the name's last template argument, above 1) -- more VGPRs.
"""
import re
import subprocess
import sys

FILES = ("kernels.s", "front_ycc.s", "front_gray.s")


def kernels(path):
    out, name, cur, count = {}, None, None, 0
    for line in open(path):
        m = re.match(r"^(_Z\w*k_front\w*):", line)
        if m:
            name, count = m.group(1), 0
            out[name] = {}
        elif name and re.match(r"^\s+[a-z]\w+(\s|$)", line) and not line.lstrip().startswith("."):
            count += 1
            if line.split()[0] == "s_endpgm":
                out[name]["insts"] = count
                name = None
        m = re.match(r"^\s+\.amdhsa_kernel (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"^\s+\.amdhsa_(next_free_vgpr|group_segment_fixed_size|private_segment_fixed_size) (\d+)", line)
        if m and cur in out:
            out[cur][m.group(1)] = int(m.group(2))
    return out


def per_cu(k):
    lds, vgpr = k["group_segment_fixed_size"], k["next_free_vgpr"]
    return min(163840 // lds if lds else 8, 512 // ((vgpr + 7) // 8 * 8), 8)


def main():
    parent_dir, new_dir = sys.argv[1:3]
    cxxfilt = sys.argv[3] if len(sys.argv) > 3 else "c++filt"
    bad, grown, n = [], [], 0
    print("# kernel | parent: vgpr lds scratch insts wg/cu | new: vgpr lds scratch insts wg/cu")
    for f in FILES:
        old, new = kernels(f"{parent_dir}/{f}"), kernels(f"{new_dir}/{f}")
        if sorted(old) != sorted(new):
            bad.append(f"{f}: the two builds hold different kernels")
        names = sorted(set(old) & set(new))
        plain = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        for mangled, name in sorted(zip(names, plain), key=lambda t: t[1]):
            name = re.sub(r"^void dmmt::|\(.*$", "", name)
            a, b = old[mangled], new[mangled]
            cols = lambda k: f"{k['next_free_vgpr']:3d} {k['group_segment_fixed_size']:6d} {k['private_segment_fixed_size']} {k['insts']:5d} {per_cu(k)}"
            print(f"{f[:-2]:10s} {name:55s} | {cols(a)} | {cols(b)}")
            n += 1
            bounded = int(re.search(r"(\d+)>$", name).group(1)) > 1
            if per_cu(b) < per_cu(a):
                bad.append(f"{name}: {per_cu(a)} -> {per_cu(b)} workgroups per CU")
            if b["private_segment_fixed_size"]:
                bad.append(f"{name}: scratch")
            if b["group_segment_fixed_size"] != a["group_segment_fixed_size"]:
                bad.append(f"{name}: LDS bytes differ")
            if bounded and b["next_free_vgpr"] > a["next_free_vgpr"]:
                bad.append(f"{name}: more VGPRs under a register budget")
            if b["insts"] > a["insts"] * 1.01:
                grown.append(f"{name}: {a['insts']} -> {b['insts']} instruction lines")
    print(f"# {n} kernels; fell a class: {len(bad)}; instruction lines up by more than 1 %: {len(grown)}")
    for line in bad + grown:
        print("# " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
