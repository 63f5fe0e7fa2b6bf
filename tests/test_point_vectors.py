"""The adversarial coordinates of tests/point_vectors.py through the g++ twin of the point formulas (selftest_point_raw,
csrc/ecgpu_selftest_point_raw.h: Group<C> and ct_dbl4 on raw limbs), all twelve parameter sets, against BOTH builds of the twin:
the plain one and the -DECGPU_BOUNDS_CHECK one, where every wrap / add / neg checks at run time the magnitude its type declares —
the formulas wrap their operands as m (Proj, Affine) and mj (Jac, Xyzz), so the limbs written here are checked against exactly
those claims, and a trap is a failure of the bound analysis.  Per vector: the result's class equals the model's, and the
returned limbs keep what the return type promises ((1, 1) for Proj, (1, JTV) for what jstore stored).  The generator's coverage
assertions run once per set.  tests/test_gpu_point_vectors.py runs the same vectors on gfx950 and compares limb for limb.

One stand-alone program (tests/hostcheck/point_raw_san.cpp, AddressSanitizer + UBSan, run as a child process on a file of
records) repeats a slice of every op on every set over buffers of exactly one record."""
import ctypes
import os
import struct
import subprocess
import fcntl

import numpy as np
import pytest

import hostcheck_lib as hc
import point_vectors as pv
from test_field_adversarial import _bounds_lib

HC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
SAN_SRC, SAN_PROG = os.path.join(HC, "point_raw_san.cpp"), os.path.join(HC, "point_raw_san")


@pytest.fixture(scope="module", params=["plain", "bounds"])
def twin(request):
    hc.lib()
    old = hc._lib
    if request.param == "bounds":
        hc._lib = _bounds_lib()
    yield request.param
    hc._lib = old


@pytest.mark.parametrize("curve", pv.CURVES)
def test_generator_coverage(curve):
    """every limb position at its bound and at zero in every operand slot, [p, 2p) everywhere, every D relation under every
    identity spelling, V = JV on the Montgomery sets — from the accepted vectors"""
    ev = pv.check_coverage(curve)
    assert ev["B acc"] >= 200


@pytest.mark.parametrize("curve", pv.CURVES)
def test_point_formulas_on_adversarial_limbs(twin, curve):
    S = pv.get_set(curve)
    vecs, _ = pv.vectors(curve)
    for op in sorted(vecs):
        P, Q = pv.arrays(S, vecs[op])
        out = hc.point_raw(S.c.cid, op, P, Q)
        msg = pv.first_failure(S, op, vecs[op], out)
        assert msg is None, "%s twin: %s" % (twin, msg)
        # what the gfx950 test holds the device to, limb for limb (`python tests/point_vectors.py --golden` rewrites it)
        assert pv.digest(out) == pv.golden()[curve][str(op)], "%s twin: %s op %d differs from tests/golden/point_vectors_twin.json" % (twin, curve, op)


def test_raw_point_ops_reject_what_they_do_not_know():
    rec = np.zeros(4 * hc.NL[1], np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    for op in (18, 99, 255, 4 | 1 << 8, 15 | 65 << 8):
        assert hc.lib().hc_point_raw(1, op, rec.ctypes.data_as(u32p), None, ctypes.c_size_t(1), rec.copy().ctypes.data_as(u32p)) == -1, op


def build_san():
    csrc = os.path.join(os.path.dirname(os.path.dirname(HC)), "elliptic-curves_amd", "csrc")
    deps = [SAN_SRC, os.path.join(HC, "batchinv_host.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    with open(SAN_PROG + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(SAN_PROG) or os.path.getmtime(SAN_PROG) < max(os.path.getmtime(d) for d in deps):
            tmp = "%s.%d.tmp" % (SAN_PROG, os.getpid())
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=undefined,address",
                                   "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", tmp, SAN_SRC])
            os.replace(tmp, SAN_PROG)


def test_sanitized_standalone_program(tmp_path):
    """AddressSanitizer + UBSan on every op of every set: the loose patterns lead each list, so a slice from its head and one
    from its tail see limbs at LB and the structured ones; results compared inside the program with the plain twin's."""
    build_san()
    cases = []
    for curve in pv.CURVES:
        S = pv.get_set(curve)
        vecs, _ = pv.vectors(curve)
        for op in sorted(vecs):
            vs = vecs[op][:24] + vecs[op][-8:]
            P, Q = pv.arrays(S, vs)
            want = hc.point_raw(S.c.cid, op, P, Q)
            assert pv.first_failure(S, op, vs, want) is None
            cases.append(struct.pack("<4I", S.c.cid, op, len(vs), int(Q is not None)) + P.tobytes() + (Q.tobytes() if Q is not None else b"") +
                         np.ascontiguousarray(want).tobytes())
    path = tmp_path / "records.bin"
    path.write_bytes(b"".join(cases))
    r = subprocess.run([SAN_PROG, str(path)], capture_output=True)
    assert r.returncode == 0 and r.stdout.decode().strip() == "%d cases equal" % len(cases), (r.returncode, r.stdout[-300:], r.stderr[-3000:])
