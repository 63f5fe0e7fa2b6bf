"""Adversarial limb-level vectors (tests/field_vectors.py) through the g++ twin of the device arithmetic, for all twelve
parameter sets and against BOTH builds of the twin: the plain one and the -DECGPU_BOUNDS_CHECK one, where every lazily reduced
element is checked at run time against the magnitude its type declares (a violated bound traps).

Family C (canonical domain, existing ops), family R (raw domain, ops 30 - 39 of csrc/ecgpu_selftest_raw.h: structured limbs and
the second representative [p, 2p) at the magnitude limits, the fused mul_sub / sqr_sub of every parameter set among them) and
family N (ScalarN: ops 0 - 4 of the twin's scalar_op, the device's 40 - 44).  Expected values are Python integers; equality is
exact.  tests/test_gpu_field_adversarial.py runs the same vectors on gfx950.

What these vectors cannot reach: the slack between 2^B - 1 and LB - 1 of a limb.  Operands that enter through unpack have strict
limbs; only a reduction's own output carries more.  tools/field_model.py covers that corner on the Python restatement, and on
the device k256's op 15 (tests/test_gpu_selftest.py) keeps covering it for the assembly blocks."""
import ctypes
import fcntl
import os
import subprocess

import pytest

import field_vectors as fv
import hostcheck_lib as hc
import pyec

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS_LIB = os.path.join(HERE, "hostcheck", "libhostcheck_bounds.so")


def _bounds_lib():
    src = os.path.join(HERE, "hostcheck", "hostcheck.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "elliptic-curves_amd", "csrc")
    # (as in test_hostcheck_bounds.py: one pytest-xdist worker builds, into a temporary name, the others wait)
    with open(BOUNDS_LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        if not os.path.exists(BOUNDS_LIB) or os.path.getmtime(BOUNDS_LIB) < max(os.path.getmtime(d) for d in deps):
            tmp = "%s.%d.tmp" % (BOUNDS_LIB, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DECGPU_BOUNDS_CHECK", "-Wno-unknown-pragmas",
                                   "-o", tmp, src])
            os.replace(tmp, BOUNDS_LIB)
    return ctypes.CDLL(BOUNDS_LIB)


@pytest.fixture(scope="module", params=["plain", "bounds"])
def twin(request):
    """hostcheck_lib on the plain build, then on the bounds-checking build (swapped in the way test_hostcheck_bounds.py does)."""
    hc.lib()
    old = hc._lib
    if request.param == "bounds":
        hc._lib = _bounds_lib()
    yield request.param
    hc._lib = old


def _run(c, fam, call):
    for op in sorted(fam):
        a, b, want = fam[op]
        got = fv.dec(c, call(op, fv.enc(c, a), fv.enc(c, b) if b is not None else None))
        msg = fv.first_mismatch(c, op, fam[op], got)
        assert msg is None, msg


@pytest.mark.parametrize("curve", fv.CURVES)
def test_canonical_domain_structured_and_steered(twin, oracle, curve):
    """Family C: structured canonical values and structured INTERNAL limbs (s R^-1), result-steered pairs, the inversion shapes;
    ops 0 - 2 also against the oracle on every 37th case."""
    c = pyec.CURVES[curve]
    fam = fv.family_c(curve)
    fv.check_coverage(curve, fam_c=fam)
    _run(c, fam, lambda op, a, b: hc.field_op_batch(c.cid, op, a, b))
    for op in (0, 1, 2):
        a, b, want = fam[op]
        for i in range(0, len(a), 37):
            A, B = a[i].to_bytes(c.L, c.order), b[i].to_bytes(c.L, c.order)
            assert int.from_bytes(oracle.field_op(c.cid, op, A, B), c.order) == want[i], (curve, op, hex(a[i]), hex(b[i]))


@pytest.mark.parametrize("curve", fv.CURVES)
def test_raw_domain_at_the_magnitude_limits(twin, curve):
    """Family R: ops 30 - 39 on limbs as written (all ones, one limb, [p, 2p)), scaled to MAXPROD / MAXMAG / SQLIM."""
    c = pyec.CURVES[curve]
    fam = fv.family_r(curve)
    fv.check_coverage(curve, fam_r=fam)
    _run(c, fam, lambda op, a, b: hc.field_op_batch(c.cid, op, a, b))


@pytest.mark.parametrize("curve", fv.CURVES)
def test_scalars_mod_n(twin, curve):
    """Family N: ScalarN's Montgomery multiplication, safegcd inversion, reduce_wire (p521: all 128 subtractions), is_high and
    the to_mont / from_mont round trip."""
    c = pyec.CURVES[curve]
    fam = fv.family_n(curve)
    fv.check_coverage(curve, fam_n=fam)
    _run(c, fam, lambda op, a, b: hc.scalar_op_batch(c.cid, fv.N_OP_TO_HOSTCHECK[op], a, b))


def test_raw_ops_reject_what_they_do_not_know():
    c = pyec.CURVES["p256"]
    one = fv.enc(c, [1])
    for op in (22, 29, 40, 45):
        assert hc.lib().hc_field_op(c.cid, op, hc._p(hc._a(one)), hc._p(hc._a(one)), hc._p(hc._a(one))) == -1
    assert hc.lib().hc_scalar_op(c.cid, 5, hc._p(hc._a(one)), None, hc._p(hc._a(one))) == -1
