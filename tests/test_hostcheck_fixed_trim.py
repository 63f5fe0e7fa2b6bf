"""fixed_base_mul (csrc/ecgpu_fixedmul.h) on the CPU over the scalars of tests/fixed_trim_vectors.py, against the big-integer model
(tests/pyec.py).  On the host a lane is its own wave: a scalar leaves the fast path of the comb walk at its first zero digit, so one
scalar per zero position (window 0, window 1, both, every other window) takes every hand-over from the fast path to the state
machine, and the special scalars (0, 1, n - 1, one-window scalars, the comb's corner scalars, the carry patterns) take the rest.
bp256 is the COMB_NEEDS_CHECK set and p384 a set of another width: both keep the single loop; w = 5 puts bp256's top window at bit 255.

The widths are 5 and 8, not the 15 / 17 / widths in use of the GPU test: the CPU table of width w holds 2^(w-1) entries per window,
each normalised by an inversion of its own (minutes from w = 15 on; tests/hostcheck/fixed_trim_san.cpp refuses w > 12), and the
model's affine multiplication costs milliseconds per scalar, so the list is the GPU test's with one scalar per zero position instead
of a wave per position and the one-window scalars at digit 2^(w-1) only (`fixed_trim_vectors.host_scalars`).  Every hand-over from
the fast path — a zero digit at each window, at window 0, window 1 and both — and every special scalar is in it.

The same scalars go through a stand-alone program under AddressSanitizer + UBSan (tests/hostcheck/fixed_trim_san.cpp)."""
import fcntl
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import comb_vectors as cv
import fixed_trim_vectors as ftv
import hostcheck_lib as hc
import pyec

HC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
SAN_SRC, SAN_PROG = os.path.join(HC, "fixed_trim_san.cpp"), os.path.join(HC, "fixed_trim_san")
CASES = [("k256", 5), ("k256", 8), ("p256", 8), ("p384", 8), ("bp256", 5), ("bp256", 8)]


@functools.lru_cache(None)
def vectors(curve, w):
    """(scalars, wire scalars, expected x || y records, expected identity flags) by the model, once per case"""
    c = pyec.CURVES[curve]
    ks = ftv.host_scalars(c, w, 0xF17E0000 + 64 * c.cid + w)
    pts = [pyec.enc_point(c, pyec.mul(c, k, pyec.G(c))) for k in ks]
    return ks, cv.enc(c, ks), b"".join(p[0] for p in pts), bytes(p[1] for p in pts)


def test_vectors_cover_what_they_claim():
    for curve, w in CASES:
        c = pyec.CURVES[curve]
        nwin = cv.window_count(c, w)
        ks = vectors(curve, w)[0]
        first_zero, folded_first_zero, carries = set(), set(), 0
        for k in ks:
            if k == 0:
                continue
            flip, d = cv.recode(c, w, k)
            top = max(j for j in range(nwin) if d[j])
            z = [j for j in range(top) if d[j] == 0]
            if z:
                (folded_first_zero if flip else first_zero).add(z[0])
            if d[0] == 0 and d[1] == 0:
                first_zero.add("0 and 1")
            live = [x for x in d if x]
            carries += len(live) >= nwin - 1 and all(x < 0 for x in live[:-1])
        # a zero digit below the top non-zero one at every window but the last; the top window zero is every small scalar
        assert set(range(nwin - 1)) <= first_zero and "0 and 1" in first_zero, (curve, w)
        # n - k is folded back to k whenever n is close to 2^bits; for bp256 (n = 0.66 * 2^256) only where k is small enough
        assert (set(range(nwin - 1)) <= folded_first_zero) if c.n >> (8 * c.L - 4) == 15 else folded_first_zero, (curve, w)
        assert carries >= 1 and 0 in ks and 1 in ks and c.n - 1 in ks, (curve, w)


@pytest.mark.parametrize("curve,w", CASES)
def test_twin_against_the_model(curve, w):
    c = pyec.CURVES[curve]
    ks, scal, want, winf = vectors(curve, w)
    for nthreads in (1, 7):
        rc, out, inf = hc.batch_mul_base(c.cid, w, scal, nthreads)
        assert rc == 0
        got = np.asarray(out).reshape(len(ks), 2 * c.L)
        exp = np.frombuffer(want, np.uint8).reshape(len(ks), 2 * c.L)
        bad = np.flatnonzero((got != exp).any(axis=1) | (np.asarray(inf) != np.frombuffer(winf, np.uint8)))
        assert bad.size == 0, "%s w = %d: %d of %d differ, first k = %#x, digits %s" % (
            curve, w, bad.size, len(ks), ks[bad[0]], cv.recode(c, w, ks[bad[0]]))


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
    build_san()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for curve, w in CASES:
            c = pyec.CURVES[curve]
            ks, scal, want, winf = vectors(curve, w)
            f.write(struct.pack("<3I", c.cid, w, len(ks)) + bytes(scal) + want + winf)
    r = subprocess.run([SAN_PROG, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d cases equal" % len(CASES) in r.stdout
