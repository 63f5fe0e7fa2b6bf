"""tools/ct_isa_check.py --unit bignsign on the gfx950 code of the bign signing kernels (csrc/ecgpu_bignsign.h): the generator, the
finish and the load kernel report OK — the generator's S-box lookups are computed, not fetched —, and the two kernels that are left
off the list on purpose ARE reported: k_bign_genk_retry for its loop on the rejected candidates, k_bign_sign_s0 for its S-box table
in LDS, which shows that the analysis sees data-indexed lookups in this unit.  Compiles to assembly with hipcc (no GPU needed)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "ct_isa_check.py")
KERNELS = ("k_bign_genk", "k_bign_sign_finish", "k_sign_nonce_load")
MUST_FLAG = ("k_bign_genk_retry", "k_bign_sign_s0")

_run = {}


def run(*args):
    if args not in _run:                                       # one compilation per argument list, shared among the tests
        _run[args] = subprocess.run([sys.executable, TOOL, "--unit", "bignsign", "--curve", "Bign256Params", *args], capture_output=True,
                                    text=True)
    return _run[args]


def test_the_default_kernels_pass_and_the_two_others_are_reported():
    r = run("--must-flag", ",".join(MUST_FLAG))
    assert r.returncode == 0, r.stdout + r.stderr
    head, tail = r.stdout.split("-- %s (violations expected)" % MUST_FLAG[0])
    lines = [l for l in head.splitlines() if "instructions" in l]
    for k in KERNELS:
        mine = [l for l in lines if "::%s<" % k in l]
        assert len(mine) == 1 and mine[0].rstrip().endswith("-> OK"), (k, r.stdout)
    assert len(lines) == len(KERNELS)                          # k_bign_genk_retry is not selected by the name k_bign_genk
    assert "VIOLATIONS" not in head and "NOT FOUND" not in r.stdout and "MUST-FLAG FAILED" not in r.stdout
    retry, s0 = tail.split("-- %s (violations expected)" % MUST_FLAG[1])
    assert "k_bign_genk_retry<" in retry and "VIOLATIONS" in retry and "branch on tainted" in retry
    assert "k_bign_sign_s0<" in s0 and "VIOLATIONS" in s0 and "LDS address from tainted register" in s0


def test_the_retry_kernel_alone_fails_the_check():
    r = run("--kernels", "k_bign_genk_retry")
    assert r.returncode != 0 and "VIOLATIONS" in r.stdout


def test_unknown_kernel_is_an_error():
    r = run("--kernels", "k_no_such_kernel")
    assert r.returncode != 0 and "NOT FOUND" in r.stdout
