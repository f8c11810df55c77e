#!/usr/bin/env python3
"""Resource table of the front kernels from two `make asm` outputs, parent beside new.

usage: front_resources.py PARENT_BUILD_DIR NEW_BUILD_DIR [CXXFILT]

For every kernel whose name contains k_front in any .s file of a build: VGPRs
(.amdhsa_next_free_vgpr), LDS bytes, scratch bytes, instruction lines and the
resident workgroups per CU they allow -- a workgroup is four waves, one per SIMD:
min(160 KiB / LDS, 512 / roundup8(VGPR), 8) -- and whether the two builds'
instruction streams are the same text once local labels are renumbered (same /
DIFFERS).  A kernel of one build is paired with the other's by what it is (key),
whatever file holds it and whatever it is called there.  Exit status 1 when a kernel
of the new build falls a class: fewer workgroups per CU, any scratch, more LDS bytes,
or -- compiled with a register budget (__launch_bounds__'s second argument, the
name's last template argument, above 1; the table's wpe column, and no part of the
key, so a kernel is paired across a change of its budget) -- more VGPRs.
"""
import glob
import re
import subprocess
import sys


def kernels(path):
    out, name, cur, labels = {}, None, None, {}
    for line in open(path):
        m = re.match(r"^(_Z\w*k_front\w*):", line)
        if m:
            name, labels = m.group(1), {}
            out[name] = {"text": []}
        elif name and re.match(r"^\s+[a-z]\w+(\s|$)", line) and not line.lstrip().startswith("."):
            inst = " ".join(line.split(";")[0].split())
            out[name]["text"].append(re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), f"L{len(labels)}"), inst))
            if inst == "s_endpgm":
                out[name]["insts"] = len(out[name]["text"])
                name = None
        m = re.match(r"^\s+\.amdhsa_kernel (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"^\s+\.amdhsa_(next_free_vgpr|group_segment_fixed_size|private_segment_fixed_size) (\d+)", line)
        if m and cur in out:
            out[cur][m.group(1)] = int(m.group(2))
    return out


def key(name):
    """The YCbCr kernels are k_front_ycc<HR, VR, FMT, WPE> (plain, uint8) and
    k_front_ycc_lv<YccLvArgs or YccMxArgs, HR, VR, FMT, SB, WPE>, and were that and
    k_front_ycc_lv, k_front_ycc_mx<HR, VR, FMT, SB, WPE>: all become
    k_front_ycc[_n] KIND<HR, VR, FMT, SB, WPE>.  Any other kernel: its name."""
    m = re.match(r"k_front_ycc(_lv|_mx)?(_n)?<(?:dmmt::Ycc(Lv|Mx)?Args, )?(.*)>$", name)
    if not m:
        return re.sub(r", \d+>$", ", *>", name)
    kind = {None: "plain", "_lv": "levels", "Lv": "levels", "_mx": "matrix", "Mx": "matrix"}[m.group(3) or m.group(1)]
    args = m.group(4).split(", ")
    if len(args) == 4:
        args.insert(3, "1")
    return f"k_front_ycc{m.group(2) or ''} {kind}<{', '.join(args[:-1])}, *>"


def build(directory, cxxfilt):
    """key -> (file, kernel) over every .s file of a build"""
    out = {}
    for path in sorted(glob.glob(f"{directory}/*.s")):
        ks = kernels(path)
        plain = subprocess.run([cxxfilt], input="\n".join(ks), capture_output=True, text=True, check=True).stdout.split("\n")
        for mangled, name in zip(ks, plain):
            name = re.sub(r"^void dmmt::|\(.*$", "", name)
            ks[mangled]["wpe"] = int(re.search(r"(\d+)>$", name).group(1))
            out[key(name)] = (path.rsplit("/", 1)[-1][:-2], ks[mangled])
    return out


def per_cu(k):
    lds, vgpr = k["group_segment_fixed_size"], k["next_free_vgpr"]
    return min(163840 // lds if lds else 8, 512 // ((vgpr + 7) // 8 * 8), 8)


def main():
    parent_dir, new_dir = sys.argv[1:3]
    cxxfilt = sys.argv[3] if len(sys.argv) > 3 else "c++filt"
    old, new = build(parent_dir, cxxfilt), build(new_dir, cxxfilt)
    bad, grown, differ = [], [], []
    for name in sorted(set(old) ^ set(new)):
        bad.append(f"{name}: only in the {'parent' if name in old else 'new'} build")
    print("# file kernel | parent: wpe vgpr lds scratch insts wg/cu | new: wpe vgpr lds scratch insts wg/cu | instruction stream")
    names = sorted(set(old) & set(new))
    for name in names:
        a, (f, b) = old[name][1], new[name]
        cols = lambda k: f"{k['wpe']} {k['next_free_vgpr']:3d} {k['group_segment_fixed_size']:6d} {k['private_segment_fixed_size']} {k['insts']:5d} {per_cu(k)}"
        same = a["text"] == b["text"]
        print(f"{f:10s} {name:55s} | {cols(a)} | {cols(b)} | {'same' if same else 'DIFFERS'}")
        bounded = b["wpe"] > 1
        if per_cu(b) < per_cu(a):
            bad.append(f"{name}: {per_cu(a)} -> {per_cu(b)} workgroups per CU")
        if b["private_segment_fixed_size"]:
            bad.append(f"{name}: scratch")
        if b["group_segment_fixed_size"] > a["group_segment_fixed_size"]:
            bad.append(f"{name}: more LDS bytes")
        if bounded and b["next_free_vgpr"] > a["next_free_vgpr"]:
            bad.append(f"{name}: more VGPRs under a register budget")
        if b["insts"] > a["insts"] * 1.01:
            grown.append(f"{name}: {a['insts']} -> {b['insts']} instruction lines")
        if not same:
            differ.append(name)
    print(f"# {len(names)} kernels ({sum('k_front_ycc' in n for n in names)} k_front_ycc); fell a class: {len(bad)}; "
          f"instruction lines up by more than 1 %: {len(grown)}; instruction stream identical: {len(names) - len(differ)}")
    for line in bad + grown:  # (a differing instruction stream: the table's last column)
        print("# " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
