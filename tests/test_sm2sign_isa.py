"""tools/ct_isa_check.py --unit sm2sign on the gfx950 code of the SM2DSA signing kernels (csrc/ecgpu_sm2sign.h): every listed kernel
reports OK, a kernel name that matches nothing is an error, and the default lists of --unit sign and --unit pke — which look at the
same translation unit — are what they were.  Compiles to assembly with hipcc (no GPU needed)."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "ct_isa_check.py")
KERNELS = ("k_sm2_sign_e", "k_sm2_rfc6979", "k_sm2dsa_sign_finish")


def run(*args):
    return subprocess.run([sys.executable, TOOL, "--unit", "sm2sign", "--curve", "Sm2Params", *args], capture_output=True, text=True)


def test_every_listed_kernel_reports_ok():
    r = run()
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if "instructions" in l]
    for k in KERNELS:
        mine = [l for l in lines if "::%s<" % k in l]
        assert len(mine) == 1 and mine[0].rstrip().endswith("-> OK"), (k, r.stdout)
    assert len(lines) == len(KERNELS)
    assert "VIOLATIONS" not in r.stdout and "NOT FOUND" not in r.stdout


def test_unknown_kernel_is_an_error():
    r = run("--kernels", "k_no_such_kernel")
    assert r.returncode != 0 and "NOT FOUND" in r.stdout


def test_the_other_units_of_the_translation_unit_are_untouched():
    spec = importlib.util.spec_from_file_location("ct_isa_check", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.UNITS["sm2sign"] == ("ecgpu_inst_sign.hip", ",".join(KERNELS))
    assert tool.UNITS["sign"] == ("ecgpu_inst_sign.hip",
                                  "k_rfc6979_first,k_schnorr_nonce,k_ecdsa_sign_finish,k_schnorr_sign_finish,k_sign_nonce_load")
    assert tool.UNITS["pke"] == ("ecgpu_inst_sign.hip", "k_pke_load,k_pke_seal,k_pke_open")
    # no name of one list selects a kernel of another (the tool matches by substring)
    for unit in ("sign", "pke"):
        for theirs in tool.UNITS[unit][1].split(","):
            assert not any(theirs in k or k in theirs for k in KERNELS), (unit, theirs)
