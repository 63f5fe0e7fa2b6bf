"""tools/ct_isa_check.py --unit pke on the gfx950 code of the SM2 public-key encryption kernels: every listed kernel reports OK, and a
kernel name that matches nothing is an error.  Compiles to assembly with hipcc (no GPU needed)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "ct_isa_check.py")
KERNELS = ("k_pke_load", "k_pke_seal", "k_pke_open")


def run(*args):
    return subprocess.run([sys.executable, TOOL, "--unit", "pke", "--curve", "Sm2Params", *args], capture_output=True, text=True)


def test_every_listed_kernel_reports_ok():
    r = run()
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if "instructions" in l]
    for k in KERNELS:
        mine = [l for l in lines if "::%s<" % k in l]
        assert len(mine) == 1 and mine[0].rstrip().endswith("-> OK"), (k, r.stdout)
    assert len(lines) == len(KERNELS)
    assert "VIOLATIONS" not in r.stdout and "NOT FOUND" not in r.stdout


def test_the_point_kernel_is_not_on_the_list_and_is_seen():
    """k_pke_point branches on the public point on purpose: it is a kernel of its own, outside the default selection, and the analysis
    sees it when asked"""
    r = run("--kernels", "k_pke_point")
    assert "::k_pke_point<" in r.stdout and "NOT FOUND" not in r.stdout, r.stdout


def test_unknown_kernel_is_an_error():
    r = run("--kernels", "k_no_such_kernel")
    assert r.returncode != 0 and "NOT FOUND" in r.stdout
