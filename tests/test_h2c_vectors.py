"""The vectors of tests/h2c_vectors.py through the g++ twin of the hash-to-curve lanes (tests/hostcheck_h2c), every row compared
exactly: family R through hh_reduce against the big-integer residue, U through hh_map and hh_sswu against tests/h2c_model.py,
P through hh_map with two u per point, I through hh_iso_k256.  CPU only.

Every test runs twice: on the plain build and on a second build of the same twin with -DECGPU_BOUNDS_CHECK, in which every lazily
reduced element is checked at run time against the magnitude its type declares — a structured u that pushed `add(sqr(tv1), tv1)`
or a `mul2` operand past its declared magnitude aborts there."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import h2c_model as hm
import h2c_vectors as hv
import pyec
import test_hostcheck_h2c as T

BOUNDS_LIB = os.path.join(T.HERE, "libhostcheck_h2c_bounds.so")
_u8p = ctypes.POINTER(ctypes.c_uint8)
_map_memo = {}


def bounds_lib():
    deps = [T.SRC] + [os.path.join(T.CSRC, f) for f in os.listdir(T.CSRC) if f.endswith(".h")]
    with open(BOUNDS_LIB + ".lock", "w") as lock:            # pytest-xdist workers arrive together: one builds, the others wait
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(BOUNDS_LIB) or os.path.getmtime(BOUNDS_LIB) < max(os.path.getmtime(d) for d in deps):
            tmp = BOUNDS_LIB + ".tmp.%d" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DECGPU_BOUNDS_CHECK", "-Wno-unknown-pragmas",
                                   "-o", tmp, T.SRC])
            os.replace(tmp, BOUNDS_LIB)
    return ctypes.CDLL(BOUNDS_LIB)


@pytest.fixture(scope="module", params=["plain", "bounds"])
def twin(request):
    return T.lib() if request.param == "plain" else bounds_lib()


def _a(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _p(a):
    return a.ctypes.data_as(_u8p)


def model_map(s, u):
    key = (s.curve.name, u)
    if key not in _map_memo:
        _map_memo[key] = hm.map_to_curve(s, u)
    return _map_memo[key]


def twin_reduce(lib, s, which, okms):
    c = s.curve
    n = len(okms)
    I, out = _a(b"".join(okms)), np.zeros(n * c.L, np.uint8)
    assert lib.hh_reduce(c.cid, int(which == "n"), _p(I), ctypes.c_size_t(n), _p(out)) == 0
    return [int.from_bytes(bytes(out[i * c.L:(i + 1) * c.L]), "big") for i in range(n)]


def twin_map(lib, s, us, per_point):
    """the points as X || Y || Z records, and the flags"""
    c = s.curve
    n = len(us) // per_point
    U = _a(b"".join(u.to_bytes(c.L, "big") for u in us))
    out, flags = np.zeros(n * 3 * c.L, np.uint8), np.zeros(n, np.uint8)
    assert lib.hh_map(c.cid, _p(U), per_point, ctypes.c_size_t(n), _p(out), _p(flags)) == 0
    return [bytes(out[i * 3 * c.L:(i + 1) * 3 * c.L]) for i in range(n)], list(flags)


def first_bad(rows, got, want):
    """None, or the first differing row with both values"""
    assert len(got) == len(want) == len(rows)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    return None if not bad else "%d of %d differ, first at %d: %r, got %r, want %r" % (len(bad), len(want), bad[0], rows[bad[0]], got[bad[0]],
                                                                                      want[bad[0]])


@pytest.mark.parametrize("curve", hv.CURVES)
def test_coverage(curve):
    hv.check_coverage(curve)


@pytest.mark.parametrize("which", ["p", "n"])
@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_r_reductions(twin, curve, which):
    s = hm.SUITES[curve]
    rows = hv.family_r(curve, which)
    got = twin_reduce(twin, s, which, [okm for _, okm, _ in rows])
    m = hv.modulus(curve, which)
    want = [int.from_bytes(okm, "big") % m for _, okm, _ in rows]
    assert want == [w for _, _, w in rows]
    bad = first_bad([(cls, okm.hex()) for cls, okm, _ in rows], got, want)
    assert bad is None, (curve, which, bad)


@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_u_map_and_sswu(twin, curve):
    s = hm.SUITES[curve]
    c = s.curve
    rows = hv.family_u(curve)
    us = [u for _, u in rows]
    recs, flags = twin_map(twin, s, us, 1)
    assert not any(flags)
    got = [T.affine(c, r) for r in recs]
    want = [model_map(s, u) for u in us]
    assert all(P is not pyec.INF and pyec.on_curve(c, P) for P in want)
    bad = first_bad(rows, got, want)
    assert bad is None, (curve, bad)
    # the map before the isogeny and before the projective hand-over: xn / xd and y on the curve SSWU runs on
    U, out = _a(b"".join(u.to_bytes(c.L, "big") for u in us)), np.zeros(len(us) * 3 * c.L, np.uint8)
    assert twin.hh_sswu(c.cid, _p(U), ctypes.c_size_t(len(us)), _p(out)) == 0
    got = []
    for i in range(len(us)):
        xn, xd, y = (int.from_bytes(bytes(out[(3 * i + j) * c.L:(3 * i + j + 1) * c.L]), "big") for j in range(3))
        assert 0 < xd < c.p and xn < c.p and y < c.p, (curve, rows[i])
        got.append((xn * pow(xd, -1, c.p) % c.p, y))
    bad = first_bad(rows, got, [hm.sswu(s, u) for u in us])
    assert bad is None, (curve, "sswu", bad)


@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_p_colliding_pairs(twin, curve):
    s = hm.SUITES[curve]
    c = s.curve
    rows = hv.family_p(curve, model_map)
    us = [u for r in rows for u in r[:2]]
    recs, flags = twin_map(twin, s, us, 2)
    assert not any(flags)
    bad = first_bad(rows, [T.affine(c, r) for r in recs], [r[2] for r in rows])
    assert bad is None, (curve, bad)
    for r, rec in zip(rows, recs):
        Z = int.from_bytes(rec[2 * c.L:], "big")
        if r[2] is pyec.INF:                                 # a Z the formulas computed from unequal Z1, Z2: zero exactly
            assert Z == 0 and any(rec[:2 * c.L]), (curve, r)
        else:
            assert Z != 0 and pyec.on_curve(c, T.affine(c, rec)), (curve, r)


def test_family_i_isogeny(twin):
    s = hm.SUITES["k256"]
    c = s.curve
    rows = hv.family_i("k256")
    enc = lambda k: _a(b"".join(r[k].to_bytes(32, "big") for r in rows))
    XN, XD, Y, out = enc(1), enc(2), enc(3), np.zeros(len(rows) * 96, np.uint8)
    assert twin.hh_iso_k256(_p(XN), _p(XD), _p(Y), ctypes.c_size_t(len(rows)), _p(out)) == 0
    recs = [bytes(out[i * 96:(i + 1) * 96]) for i in range(len(rows))]
    bad = first_bad([r[:4] for r in rows], [T.affine(c, r) for r in recs], [r[4] for r in rows])
    assert bad is None, bad
    identity = (0).to_bytes(32, "big") + (1).to_bytes(32, "big") + (0).to_bytes(32, "big")
    for r, rec in zip(rows, recs):
        assert (rec == identity) == (r[4] is pyec.INF), r[:4]                # exactly (0 : 1 : 0), nothing else with Z = 0
