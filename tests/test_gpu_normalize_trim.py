"""-m gpu: k_normalize behind ecgpu_batch_mul_base_dev (the quad-major hand-over from k_fixed_base) and behind
ecgpu_batch_normalize_dev (record-major, wire records in), byte for byte against the oracle.

Point counts 1, 65,535, 65,536, 65,537 (the first count at which a lane owns two records) and 2 x 65,536 + 1 (three).  The lanes of a
call are tests/comb_vectors.py `normalize_lanes`: lane t owns records t, t + T, t + 2 T, ...  Identities (k = 0, resp. Z = 0) sit
first, last and in the middle of a lane's chain, on every record of a chain, on the one record of the lane that owns a single one, on
the first records of all 64 lanes of a wave and on the last records of another wave.

Coordinates of the wire records: 0, 1 and p - 1 in every combination of X, Y, Z (Z = 0 is the identity whatever X and Y are), the
values of the limb patterns of tests/point_vectors.py (limbs at the magnitude limits; a wire record carries their canonical values,
the limbs themselves reach the formulas in tests/test_gpu_point_vectors.py), and random ones.  The records need not be on the curve:
to_affine is X / Z, Y / Z.  The oracle's result for the largest count is computed once and cut for the smaller ones.  A call on ONE
record is made with the identity (the cases above) and with a regular record.

The identity test of the forward pass itself — Field::is_zero_short, k256: the strict limbs after one fold against 0 and p — on
Z as LIMBS, which neither entry point can carry: raw point op 19 (csrc/ecgpu_selftest_point_raw.h) over
normalize_trim_vectors.zero_test_limbs (the point vectors' limbs by import, the spellings of 0 and p, every multiple of p that fits,
a top limb at and above 2^24), against the integers and against Field::is_zero in the same record."""
import ctypes

import numpy as np
import pytest

import comb_vectors as cv
import oracle_lib
import pyec
from gpu_common import ecgpu_module, rand_scalars
from normalize_trim_vectors import identity_records, wire_records, zero_test_limbs

pytestmark = pytest.mark.gpu

COUNTS = (1, 65535, 65536, 65537, 2 * 65536 + 1)
NMAX = max(COUNTS)
CURVES = ("k256", "p256")


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)          # raises without the HIP extension / a gfx950 device: no fallback
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def test_lane_geometry_is_what_the_cases_assume():
    assert [cv.normalize_lanes(n) for n in COUNTS] == [(1, 1), (1, 65535), (1, 65536), (2, 32769), (3, 43691)]
    assert len(range(32768, 65537, 32769)) == 1 and len(range(0, 65537, 32769)) == 2       # one lane with a single record


def dev_call(eng, name, cid, inputs, n, out_bytes):
    lib = eng._lib
    dp = lambda b: ctypes.c_void_p(b.ptr)
    bufs = [eng.to_device(x) for x in inputs]
    d_o, d_f = eng.dev_alloc(max(out_bytes, 16)), eng.dev_alloc(max(n, 16))
    try:
        eng._chk(getattr(lib, name)(eng._ctx, cid, *[dp(b) for b in bufs], ctypes.c_size_t(n), dp(d_o), dp(d_f)))
        return eng.to_host(d_o, out_bytes), eng.to_host(d_f, n)
    finally:
        for b in bufs + [d_o, d_f]:
            b.free()


@pytest.fixture(scope="module")
def base_points():
    """per curve: NMAX random scalars and the oracle's k G for them, once"""
    out = {}
    for name in CURVES:
        c = pyec.CURVES[name]
        scal = rand_scalars(c.cid, NMAX, 0x4E0A0000 + c.cid).reshape(NMAX, c.L)
        want, winf = oracle_lib.batch_mul_base_mt(c.cid, scal.reshape(-1))
        assert not winf.any()
        out[name] = (scal, np.asarray(want, np.uint8).reshape(NMAX, 2 * c.L))
    return out


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("curve", CURVES)
def test_mul_base_hand_over(eng, base_points, curve, n):
    c = pyec.CURVES[curve]
    scal, want = base_points[curve]
    scal, want = scal[:n].copy(), want[:n].copy()
    ident = identity_records(n)
    scal[ident] = 0
    want[ident] = 0
    winf = np.zeros(n, np.uint8)
    winf[ident] = 1
    got, ginf = dev_call(eng, "ecgpu_batch_mul_base_dev", c.cid, [scal.reshape(-1)], n, n * 2 * c.L)
    bad = np.flatnonzero((got.reshape(n, 2 * c.L) != want).any(axis=1) | (ginf != winf))
    assert bad.size == 0, (curve, n, bad[:8], cv.normalize_lanes(n))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("curve", CURVES)
def test_normalize_wire_records(eng, curve, n):
    c = pyec.CURVES[curve]
    rec = wire_records(c, n, 0x4E0B0000 + 8 * c.cid + COUNTS.index(n))
    want, winf = oracle_lib.batch_normalize(c.cid, rec.reshape(-1))
    winf = np.asarray(winf, np.uint8)
    assert winf[identity_records(n)].all() and winf.sum() < len(identity_records(n)) + 40
    got, ginf = dev_call(eng, "ecgpu_batch_normalize_dev", c.cid, [rec.reshape(-1)], n, n * 2 * c.L)
    bad = np.flatnonzero((got.reshape(n, 2 * c.L) != np.asarray(want, np.uint8).reshape(n, 2 * c.L)).any(axis=1) | (ginf != winf))
    assert bad.size == 0, (curve, n, bad[:8], rec[bad[0]].tobytes().hex() if bad.size else None)


@pytest.mark.parametrize("curve", CURVES)
def test_one_regular_record(eng, base_points, curve):
    c = pyec.CURVES[curve]
    scal, want = base_points[curve]
    got, ginf = dev_call(eng, "ecgpu_batch_mul_base_dev", c.cid, [scal[7].copy()], 1, 2 * c.L)
    assert bytes(got) == bytes(want[7]) and bytes(ginf) == b"\0", curve
    for seed in range(4):
        rec = wire_records(c, 1, 0x4E0E0000 + seed, identities=False)
        rec[0, 2 * c.L:] = np.random.default_rng(seed).integers(1, 255, c.L, dtype=np.uint8)     # a random Z: not 0, below p
        rec[0, 2 * c.L] &= 0x7F
        want1, winf1 = oracle_lib.batch_normalize(c.cid, rec.reshape(-1))
        assert not np.asarray(winf1).any()
        got, ginf = dev_call(eng, "ecgpu_batch_normalize_dev", c.cid, [rec.reshape(-1)], 1, 2 * c.L)
        assert bytes(got) == bytes(want1) and bytes(ginf) == b"\0", (curve, seed, rec.tobytes().hex())


@pytest.mark.parametrize("curve", ["k256", "p256", "p384"])
def test_forward_pass_zero_test_on_limbs(eng, curve):
    rec, want = zero_test_limbs(curve)
    out = eng.selftest_point_raw(pyec.CURVES[curve].cid, 19, rec)
    short, full = out[:, 0] == 1, out[:, 1] == 1
    assert (out[:, :2] <= 1).all() and not out[:, 2:].any()
    bad = np.flatnonzero((short != want) | (full != want))
    assert bad.size == 0, (curve, bad[:8], [hex(int(x)) for x in rec[bad[0]]][-20:] if bad.size else None)
