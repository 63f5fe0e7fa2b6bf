"""csrc/ecgpu_fe448.h and the lane body of k_x448_ladder (csrc/ecgpu_x448.h) compiled for the CPU (tests/hostcheck_x448): the fe448
vectors of tests/fe448_vectors.py through the plain build and the -DECGPU_BOUNDS_CHECK build, limb for limb against Python integers
(a trap in the bounds build is a failure of the bound analysis), and the ladder against tests/x448_model.py on the golden vectors,
the 1,000-iteration chain of RFC 7748, 200 random pairs and every special u.  The same source with its own main is built with
AddressSanitizer + UBSan as a stand-alone program and run once over such rows.  CPU only."""
import ctypes
import fcntl
import json
import os
import random
import subprocess

import numpy as np
import pytest

import fe448_vectors as fv
import x448_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostcheck_x448")
SRC = os.path.join(HERE, "hostcheck_x448.cpp")
LIB = os.path.join(HERE, "libhostcheck_x448.so")
BOUNDS_LIB = os.path.join(HERE, "libhostcheck_x448_bounds.so")
PROG = os.path.join(HERE, "hostcheck_x448_san")
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("ecgpu_x448.h", "ecgpu_fe448.h", "ecgpu_params.h")]
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "x448.json")))
CHECKED, UNCHECKED, BASE = 0, 1, 2
_vp = ctypes.c_void_p
_libs = {}


def _build(target, flags):
    def fresh():
        return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in DEPS)
    with open(target + ".lock", "w") as lock:               # pytest-xdist workers arrive together: one builds, the others wait
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            tmp = target + ".tmp.%d" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + flags + ["-o", tmp, SRC])
            os.replace(tmp, target)


def lib(bounds=False):
    if bounds not in _libs:
        target = BOUNDS_LIB if bounds else LIB
        _build(target, ["-O2", "-fPIC", "-shared"] + (["-DECGPU_BOUNDS_CHECK"] if bounds else []))
        _libs[bounds] = ctypes.CDLL(target)
    return _libs[bounds]


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def twin_fe448(op, rows, bounds=False):
    """-> uint32[n, 16]: the op on the rows of fe448_vectors (also what tests/test_gpu_fe448.py holds the device against)"""
    n = len(rows)
    A = np.array(fv.flat(rows, 1), np.uint32)
    fb = fv.flat(rows, 2)
    B = None if fb is None else np.array(fb, np.uint32)
    out = np.zeros(n * 16, np.uint32)
    assert lib(bounds).hx_fe448(int(op), _p(A), _p(B), ctypes.c_size_t(n), _p(out)) == 0
    return out.reshape(n, 16)


def twin_x448(mode, scalars, points, bounds=False):
    """-> [(record, ok)]"""
    n = len(scalars)
    K = np.frombuffer(b"".join(scalars), np.uint8).copy()
    U = None if points is None else np.frombuffer(b"".join(points), np.uint8).copy()
    out, ok = np.full(n * 56, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    assert lib(bounds).hx_x448(mode, _p(K), _p(U), ctypes.c_size_t(n), _p(out), _p(ok)) == 0
    return [(bytes(out[56 * i:56 * i + 56]), int(ok[i])) for i in range(n)]


# ---- the field ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", (False, True), ids=("plain", "bounds"))
@pytest.mark.parametrize("op", range(9), ids=fv.OP_NAMES)
def test_fe448_vectors_limb_for_limb(op, bounds):
    rows = fv.rows(op)
    got = twin_fe448(op, rows, bounds)
    for i, (label, a, b) in enumerate(rows):
        g = [int(x) for x in got[i]]
        assert g == fv.model(op, a, b), (fv.OP_NAMES[op], label)
        want = fv.expected_value(op, a, b)
        if want is not None:
            assert (fv.value(g) - want) % fv.P == 0, (fv.OP_NAMES[op], label)
        if op not in (fv.ADD, fv.BYTES):
            assert max(g) <= fv.T, (fv.OP_NAMES[op], label)                  # tight out, whatever came in
        if op == fv.CANON:
            assert fv.value(g) < fv.P and max(g) <= fv.MASK, label


def test_the_vectors_cover_what_they_claim():
    labels = {op: [r[0] for r in fv.rows(op)] for op in range(9)}
    for k in (0, 7, 8, 15, 22):
        assert "column %d maximal" % k in labels[fv.MUL] and "column %d maximal" % k in labels[fv.SQR]
    for t in ("product 0 (0)", "product 1 (1)", "product p - 1 (0)", "all limbs at the bound", "top limb at the bound",
              "second representative of p-1"):
        assert t in labels[fv.MUL], t
    for name in ("p-1", "p", "p+1", "2^224-1", "2^224", "2^224+1", "2^448-1"):
        for op in (fv.MUL, fv.SQR, fv.ADD, fv.SUB, fv.MUL_SMALL, fv.CARRY, fv.CANON):
            assert name + " x " + name in labels[op], (op, name)
        assert name in labels[fv.BYTES]
    assert sum(l.startswith("in [p, 2^448)") for l in labels[fv.CANON]) == 20
    for name in ("0", "1", "p-1", "2^224"):
        assert "invert " + name in labels[fv.INVERT]
    a, b = fv.rows(fv.MUL)[0][1:]
    assert max(fv.product_columns(a, b)) == 38 * 4 * fv.T ** 2 < 2 ** 64 - 2 ** 36     # the bound of the header, reached


# ---- the ladder ----------------------------------------------------------------------------------------------------------------------
def test_golden_vectors_through_the_lane_body():
    for v in VEC["fixed"]:
        k, u, want = (bytes.fromhex(v[x]) for x in ("scalar", "point", "expected"))
        assert twin_x448(CHECKED, [k], [u]) == [(want, 1)] and twin_x448(UNCHECKED, [k], [u]) == [(want, 1)]
    ab = {k: bytes.fromhex(v) for k, v in VEC["alice_bob"].items()}
    assert twin_x448(BASE, [ab["alice_private"], ab["bob_private"]], None) == [(ab["alice_public"], 1), (ab["bob_public"], 1)]
    assert twin_x448(CHECKED, [ab["alice_private"], ab["bob_private"]], [ab["bob_public"], ab["alice_public"]]) == [(ab["shared"], 1)] * 2
    for rec in VEC["low_order"]:
        assert twin_x448(CHECKED, [ab["alice_private"]], [bytes.fromhex(rec)]) == [(m.ZERO, 0)]
        assert twin_x448(UNCHECKED, [ab["alice_private"]], [bytes.fromhex(rec)]) == [(m.ZERO, 1)]


@pytest.mark.parametrize("bounds", (False, True), ids=("plain", "bounds"))
def test_the_iterated_chain(bounds):
    start = np.frombuffer(bytes.fromhex(VEC["iterated"]["start"]), np.uint8).copy()
    out = np.zeros(56, np.uint8)
    for iters, key in ((1, "after_1"), (1000, "after_1000")):
        assert lib(bounds).hx_x448_iterate(_p(start), iters, _p(out)) == 0
        assert bytes(out).hex() == VEC["iterated"][key]


@pytest.mark.parametrize("bounds", (False, True), ids=("plain", "bounds"))
def test_random_pairs_and_every_special_u(bounds):
    rng = random.Random("hostcheck-x448")
    ks = [bytes(rng.getrandbits(8) for _ in range(56)) for _ in range(200)]
    us = [bytes(rng.getrandbits(8) for _ in range(56)) for _ in range(200)]
    specials = list(m.SPECIAL_U.values()) + [m.twist_u(rng) for _ in range(4)]
    ks += [bytes(rng.getrandbits(8) for _ in range(56)) for _ in specials]
    us += specials
    assert twin_x448(CHECKED, ks, us, bounds) == [m.x448(k, u) for k, u in zip(ks, us)]
    assert twin_x448(UNCHECKED, ks, us, bounds) == [(m.x448_unchecked(k, u), 1) for k, u in zip(ks, us)]
    assert twin_x448(BASE, ks[:40], None, bounds) == [(m.public_key(k), 1) for k in ks[:40]]


def test_the_clamp_is_applied_in_the_lane_body():
    u = m.le(5)
    for k in (bytes(56), b"\xff" * 56, b"\x03" + bytes(55), bytes(55) + b"\x7f"):
        assert twin_x448(UNCHECKED, [k], [u]) == [(m.x448_unchecked(k, u), 1)]
    assert twin_x448(UNCHECKED, [bytes(56)], [u]) == twin_x448(UNCHECKED, [b"\x03" + bytes(55)], [u])


def test_sanitized_standalone_program(tmp_path):
    """AddressSanitizer + UBSan on the lane body, every buffer exactly its record's size"""
    # (the runtimes linked into the program itself: it needs no preload and does not mind what else the process environment loads)
    _build(PROG, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                  "-DHOSTCHECK_X448_MAIN"])
    rng = random.Random("x448-san")
    rows = [(CHECKED, bytes.fromhex(v["scalar"]), bytes.fromhex(v["point"])) for v in VEC["fixed"]]
    rows += [(CHECKED, bytes(rng.getrandbits(8) for _ in range(56)), u) for u in m.SPECIAL_U.values()]
    rows += [(UNCHECKED, bytes(rng.getrandbits(8) for _ in range(56)), u) for u in m.SPECIAL_U.values()]
    rows += [(BASE, bytes(rng.getrandbits(8) for _ in range(56)), m.ZERO) for _ in range(3)]
    rows += [(CHECKED, b"\xff" * 56, b"\xff" * 56), (UNCHECKED, bytes(56), m.twist_u(rng))]
    want = []
    for mode, k, u in rows:
        rec, ok = m.x448(k, u) if mode == CHECKED else (m.x448_unchecked(k, u), 1) if mode == UNCHECKED else (m.public_key(k), 1)
        want.append("%s %d" % (rec.hex(), ok))
    path = tmp_path / "rows.txt"
    path.write_text("".join("%d %s %s\n" % (mode, k.hex(), u.hex()) for mode, k, u in rows))
    r = subprocess.run([PROG, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == want
