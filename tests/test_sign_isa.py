"""The signing kernels (csrc/ecgpu_sign.h) on their gfx950 ISA: tools/ct_isa_check.py --unit sign compiles ecgpu_inst_sign.hip to
assembly (no GPU needed) and runs its taint analysis from every loaded record — keys, nonces, digests, the HMAC state, the affine
R — to every branch condition and every memory address.  k_rfc6979_retry, whose trip count follows the rejected candidates on
purpose, must be REPORTED: that the analysis objects to it shows that it looks at these kernels."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "ct_isa_check.py")
DATA_INDEPENDENT = ("k_rfc6979_first", "k_ecdsa_sign_finish", "k_schnorr_nonce", "k_schnorr_sign_finish")


def _run(*args):
    return subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=1500)


# k256 (the only set with the two Schnorr kernels), p256, p384 (SHA-384: the 64-bit compression function), a brainpool set, and
# p521: the 128-step reduction of ScalarN::reduce_wire, whose select the compiler once turned into an exec-masked block, and the
# two-output candidate of Rfc6979::first (66 bytes from a 64-byte HMAC)
@pytest.mark.parametrize("curve", ["K256Params", "P256Params", "P384Params", "Bp256Params", "P521Params"])
def test_no_branch_or_address_depends_on_a_key_nonce_or_digest(curve):
    r = _run("--unit", "sign", "--curve", curve, "--must-flag", "k_rfc6979_retry")
    assert r.returncode == 0, r.stdout + r.stderr
    ok = [line for line in r.stdout.splitlines() if line.rstrip().endswith("-> OK")]
    want = [k for k in DATA_INDEPENDENT if curve == "K256Params" or not k.startswith("k_schnorr")] + ["k_sign_nonce_load"]
    for k in want:
        assert sum(1 for line in ok if k + "<" in line) == 1, (k, r.stdout)
    assert len(ok) == len(want), r.stdout
    # the retry kernel is analysed and objected to: a branch, and the exec mask, follow the loaded accepted flag / the candidates
    tail = r.stdout[r.stdout.index("-- k_rfc6979_retry"):]
    assert "k_rfc6979_retry<" in tail and "VIOLATIONS" in tail and "MUST-FLAG FAILED" not in r.stdout, r.stdout
    assert "branch on tainted" in tail, tail


def test_a_kernel_that_does_not_exist_is_an_error():
    r = _run("--unit", "sign", "--curve", "P256Params", "--kernels", "k_rfc6979_first,k_no_such_kernel")
    assert r.returncode != 0 and "NOT FOUND" in r.stdout, r.stdout


def test_the_retry_kernel_fails_the_plain_check():
    r = _run("--unit", "sign", "--curve", "P256Params", "--kernels", "k_rfc6979_retry")
    assert r.returncode != 0 and "VIOLATIONS" in r.stdout, r.stdout
