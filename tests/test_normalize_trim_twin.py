"""The lane body of k_normalize on the CPU (NormRec under batch_inv_lane, tests/hostcheck) after the forward pass's zero test moved to
Field::is_zero_short: wire records X || Y || Z with Z = 0 first, last, in the middle and on every record of a lane's chain, on the
lane that owns a single record, and coordinates 0, 1, p - 1 and the values of the point vectors' limb patterns, against the oracle;
a call on one regular record.  k256 takes the short test (k_is_zero); p256 and p384 keep is_zero.

The test itself on Z as LIMBS (a wire record carries canonical values only): raw point op 19 of csrc/ecgpu_selftest_point_raw.h
returns Field::is_zero_short beside Field::is_zero, here on the g++ twin in its plain and its -DECGPU_BOUNDS_CHECK build, over
normalize_trim_vectors.zero_test_limbs — the limbs of tests/point_vectors.py by import (magnitude limits, the identity spelt 0 and
p), every multiple of p that magnitude-1 limbs hold in canonical and shifted splits, a top limb at and above 2^24 (the fold).
tests/test_gpu_normalize_trim.py runs the same records on gfx950.  The integer restatement is tools/field_model.py k256_is_zero_m1."""
import numpy as np
import pytest

import oracle_lib
import hostcheck_lib as hc
import pyec
from normalize_trim_vectors import wire_records, zero_test_limbs
from test_field_adversarial import _bounds_lib

N, LANES = 3 * 211 + 1, 211          # chains of three records, lane 0 owns four


@pytest.mark.parametrize("curve", ["k256", "p256", "p384"])
def test_twin_normalize_with_degenerate_records(curve):
    oracle_lib.build()
    c = pyec.CURVES[curve]
    rec = wire_records(c, N, 0x4E0C0000 + c.cid).copy()
    chain = lambda t: list(range(t, N, LANES))
    ident = [chain(3)[0], chain(4)[-1], chain(5)[1]] + chain(6) + chain(0)[-1:] + [chain(t)[0] for t in range(64, 128)]
    rec.reshape(N, 3, c.L)[ident, 2] = 0
    want, winf = oracle_lib.batch_normalize(c.cid, rec.reshape(-1))
    assert np.asarray(winf)[ident].all()
    for lanes in (LANES, 1, N):
        got, ginf = hc.normalize(c.cid, 0, rec.reshape(-1), lanes)
        assert bytes(got) == bytes(want) and bytes(ginf) == bytes(winf), (curve, lanes)
    one = wire_records(c, 1, 0x4E0C1000 + c.cid, identities=False)
    one[0, 2 * c.L:] = 0
    one[0, -1] = 3                                                # Z = 3
    want, winf = oracle_lib.batch_normalize(c.cid, one.reshape(-1))
    got, ginf = hc.normalize(c.cid, 0, one.reshape(-1), 1)
    assert not np.asarray(winf).any() and bytes(got) == bytes(want) and bytes(ginf) == bytes(winf), curve


@pytest.mark.parametrize("build", ["plain", "bounds"])
@pytest.mark.parametrize("curve", ["k256", "p256", "p384"])
def test_twin_forward_pass_zero_test_on_limbs(curve, build):
    hc.lib()
    old = hc._lib
    if build == "bounds":
        hc._lib = _bounds_lib()
    try:
        rec, want = zero_test_limbs(curve)
        out = hc.point_raw(pyec.CURVES[curve].cid, 19, rec)
    finally:
        hc._lib = old
    assert (out[:, :2] <= 1).all() and not out[:, 2:].any()
    bad = np.flatnonzero(((out[:, 0] == 1) != want) | ((out[:, 1] == 1) != want))
    assert bad.size == 0, (curve, build, bad[:8], [hex(int(x)) for x in rec[bad[0]]][-20:] if bad.size else None)
