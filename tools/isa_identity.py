#!/usr/bin/env python3
"""Are the kernels of two source trees the same instructions?  The check of a refactor that must not change device code: every
translation unit of the library (ecgpu_inst_<group>.hip x curve, ecgpu_misc.hip) is compiled to gfx950 assembly in both trees
(-S --offload-device-only with the Makefile's flags, no GPU needed) and compared kernel by kernel: the instruction text and the
kernel descriptor without the compiler's comments and with local labels (.LBB<n>_<m>, .Lpost_getpc<n>, ... — numbered per
translation unit) renamed by order of appearance, and the resource lines the compiler prints behind a kernel (registers, scratch,
LDS, occupancy).

    python tools/isa_identity.py <other tree> [this tree] [-j JOBS] [--keep DIR] [--only group_Curve ...]

Prints one line per unit, the kernels that exist in one tree only, the first differing line of every kernel that differs, and a
summary; exit status 1 if a kernel differs or exists in the second tree only.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "elliptic-curves_amd"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--offload-device-only"]
RESOURCES = ("NumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy", "LDSByteSize", "codeLenInByte")


def units(tree):
    mk = open(os.path.join(tree, PKG, "Makefile")).read()
    curves = re.search(r"^CURVES := (.*)$", mk, re.M).group(1).split()
    groups = re.search(r"^GROUPS := (.*)$", mk, re.M).group(1).split()
    return [(g, c) for g in groups for c in curves] + [("misc", "")]


def assembly(tree, unit, out):
    group, curve = unit
    if not os.path.exists(out):
        src = os.path.join(tree, PKG, "csrc", "ecgpu_%s.hip" % (group if not curve else "inst_" + group))
        cmd = ["hipcc"] + FLAGS + (["-DECGPU_CURVE=" + curve] if curve else []) + ["-o", out + ".tmp", src]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        os.rename(out + ".tmp", out)
    return open(out).read()


def kernels(txt):
    """{name: (normalised text, {resource: value})} of every function of an assembly file"""
    res = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^\t\.(?:text|section|type|globl|protected|weak)\b)", txt, re.S | re.M):
        names = {}
        body = re.sub(r"[ \t]*;[^\n]*", "", m.group(2))             # the compiler's comments quote block numbers of the unit
        body = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda l: names.setdefault(l.group(0), ".L%d" % len(names)), body)
        info = dict(re.findall(r"^; (\w+)[:=]? *=? *(\S+)", m.group(3), re.M))
        res[m.group(1)] = (body, {k: info[k] for k in RESOURCES if k in info})
    return res


def compare(unit, trees, keep):
    tag = "_".join(x for x in unit if x)
    a, b = (kernels(assembly(t, unit, os.path.join(keep, "%s_%s.s" % (side, tag)))) for side, t in zip("ab", trees))
    diff = []
    for name in sorted(set(a) & set(b)):
        if a[name][0] != b[name][0]:
            la, lb = a[name][0].split("\n"), b[name][0].split("\n")
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            diff.append("%s: line %d of %d / %d: %r / %r" % (name, i, len(la), len(lb), "".join(la[i:i + 1]).strip(), "".join(lb[i:i + 1]).strip()))
        elif a[name][1] != b[name][1]:
            diff.append("%s: resources %r / %r" % (name, a[name][1], b[name][1]))
    return tag, len(a), len(b), sorted(set(a) - set(b)), sorted(set(b) - set(a)), diff


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other")
    ap.add_argument("this", nargs="?", default=ROOT)
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 2))
    ap.add_argument("--keep", help="directory for the assembly files (kept, and reused by the next run)")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    trees = (os.path.abspath(args.other), os.path.abspath(args.this))
    todo = [u for u in units(trees[1]) if not args.only or "_".join(x for x in u if x) in args.only]
    with tempfile.TemporaryDirectory() as td:
        keep = args.keep or td
        os.makedirs(keep, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(max(1, args.j // 2)) as pool:        # (two compilations per unit)
            results = list(pool.map(lambda u: compare(u, trees, keep), todo))
    same = gone = new = differ = 0
    for tag, na, nb, only_a, only_b, diff in results:
        print("%-22s %3d -> %3d functions, %3d identical (text, descriptor, resources)" % (tag, na, nb, nb - len(only_b) - len(diff)))
        for name in only_a:
            print("    only in the first:  %s" % name)
        for name in only_b:
            print("    only in the second: %s" % name)
        for line in diff:
            print("    DIFFERS  %s" % line)
        same += nb - len(only_b) - len(diff)
        gone += len(only_a)
        new += len(only_b)
        differ += len(diff)
    print("total: %d units; %d functions identical, %d differ, %d only in the first tree, %d only in the second" % (len(results), same, differ, gone, new))
    return 1 if differ or new else 0


if __name__ == "__main__":
    sys.exit(main())
