"""tools/ct_isa_check.py --unit x448 on the gfx950 code of the X448 kernels (csrc/ecgpu_x448.h): the three instantiations of
k_x448_ladder — checked, unchecked, base — report OK (there is no finish kernel: the inversion and the canonical store are the
ladder kernel's tail), and the kernel-resource remarks of the same translation unit show no scratch.  Compiles with hipcc (no GPU
needed)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "ct_isa_check.py")
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")

_run = {}


def run(*args):
    if args not in _run:                                       # one compilation per argument list, shared among the tests
        _run[args] = subprocess.run([sys.executable, TOOL, "--unit", "x448", "--curve", "K256Params", *args], capture_output=True, text=True)
    return _run[args]


def test_the_three_ladder_kernels_pass():
    r = run()
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if "instructions" in l]
    assert len(lines) == 3
    for mode in (0, 1, 2):
        mine = [l for l in lines if "::k_x448_ladder<%d>" % mode in l]
        assert len(mine) == 1 and mine[0].rstrip().endswith("-> OK"), (mode, r.stdout)
    assert "VIOLATIONS" not in r.stdout and "NOT FOUND" not in r.stdout


def test_unknown_kernel_is_an_error():
    r = run("--kernels", "k_no_such_kernel")
    assert r.returncode != 0 and "NOT FOUND" in r.stdout


def test_every_field_op_is_free_of_data_dependent_branches():
    """k_selftest_fe448 holds every op of ecgpu_fe448.h, canon and the byte conversions included; it switches on its op — a kernel
    argument — and its loaded limbs feed nothing but arithmetic"""
    r = run("--kernels", "k_selftest_fe448")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("-> OK"), r.stdout


def test_no_scratch(tmp_path):
    """the kernel-resource remarks of the translation unit, compiled as the Makefile compiles it: 0 bytes of scratch, no spills, for
    every kernel of the unit"""
    obj = tmp_path / "x448.o"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "ecgpu_x448.hip"), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("k_x448_ladder" in n for n in names) == 3 and sum("k_selftest_fe448" in n for n in names) == 1
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    assert len(scratch) == len(names) == len(spills) == 4
    assert scratch == [0] * 4 and spills == [0] * 4, r.stderr
    assert "Dynamic Stack: True" not in r.stderr
