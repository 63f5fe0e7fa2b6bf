"""-m gpu: the vectors of tests/h2c_vectors.py on gfx950, every row compared exactly.  The reductions, the map before the isogeny
and the isogeny itself are reached through ecgpu_selftest_h2c (a kernel of its own that calls the functions k_h2c_expand and k_h2c_map
call: h2c_reduce_field, h2c_reduce_scalar, H2cMap::sswu, H2cMap::iso_k256); the map and the sum Q0 + Q1 through
ecgpu_map_to_curve_batch, the product's own entry point.  The expected values are the big-integer residue and tests/h2c_model.py: the
ones tests/test_h2c_vectors.py holds the g++ twin to, so device, twin and model agree or one of these two modules fails.

The model costs about a millisecond per mapped element: it runs once per distinct u and is shared by the tests."""
import ctypes
import random

import numpy as np
import pytest

import h2c_model as hm
import h2c_vectors as hv
import pyec
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
ERR_CURVE, ERR_ARG = -1, -7
OP_P, OP_N, OP_SSWU, OP_ISO = 0, 1, 2, 3

_memo = {}


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


def u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def enc_ints(c, values):
    return u8(b"".join(int(v).to_bytes(c.L, "big") for v in values))


def dec_ints(c, data):
    data = bytes(data)
    return [int.from_bytes(data[i:i + c.L], "big") for i in range(0, len(data), c.L)]


def model_map(s, u):
    key = (s.curve.name, u)
    if key not in _memo:
        _memo[key] = hm.map_to_curve(s, u)
    return _memo[key]


def enc_points(c, points):
    xy, inf = bytearray(), bytearray()
    for P in points:
        if P is pyec.INF:
            xy += bytes(2 * c.L); inf.append(1)
        else:
            xy += P[0].to_bytes(c.L, "big") + P[1].to_bytes(c.L, "big"); inf.append(0)
    return bytes(xy), bytes(inf)


def first_bad(rows, got, want):
    assert len(got) == len(want) == len(rows), (len(got), len(want), len(rows))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    return None if not bad else "%d of %d differ, first at %d: %r, got %r, want %r" % (len(bad), len(want), bad[0], rows[bad[0]], got[bad[0]],
                                                                                      want[bad[0]])


def ordinary_u(s, n):
    rng = random.Random("h2c-vectors-ordinary-" + s.curve.name)
    key = ("ordinary", s.curve.name)
    if key not in _memo:
        _memo[key] = [rng.randrange(1, s.curve.p) for _ in range(130)]
    return _memo[key][:n]


# ---- R: the two reductions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["p", "n"])
@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_r_reductions(eng, curve, which):
    """every row in ONE batch per (curve, modulus), in the generator's order with the classes interleaved by a fixed stride, so that
    each wave holds mixed classes; then 257 rows and 1 row (the block edge)"""
    s = hm.SUITES[curve]
    c = s.curve
    rows = hv.family_r(curve, which)
    order = sorted(range(len(rows)), key=lambda i: ((i * 37) % len(rows), i))
    rows = [rows[i] for i in order]
    assert len({cls for cls, _, _ in rows[:64]}) >= 4
    op = OP_N if which == "n" else OP_P
    for part in (rows, rows[:257], rows[-1:]):
        got = dec_ints(c, eng.selftest_h2c(c.cid, op, u8(b"".join(okm for _, okm, _ in part))))
        bad = first_bad([(cls, okm.hex()) for cls, okm, _ in part], got, [w for _, _, w in part])
        assert bad is None, (curve, which, len(part), bad)


# ---- U: the map, and the map before the isogeny ----------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_u_map_and_sswu(eng, curve):
    s = hm.SUITES[curve]
    c = s.curve
    rows = hv.family_u(curve)
    us = [u for _, u in rows]
    xy, inf = eng.map_to_curve(c.cid, enc_ints(c, us), 1)
    want = [model_map(s, u) for u in us]
    assert all(P is not pyec.INF and pyec.on_curve(c, P) for P in want)
    wxy, winf = enc_points(c, want)
    assert bytes(inf) == winf, curve
    got = [bytes(xy[i * 2 * c.L:(i + 1) * 2 * c.L]) for i in range(len(us))]
    bad = first_bad(rows, got, [wxy[i * 2 * c.L:(i + 1) * 2 * c.L] for i in range(len(us))])
    assert bad is None, (curve, bad)
    out = dec_ints(c, eng.selftest_h2c(c.cid, OP_SSWU, enc_ints(c, us)))
    got = []
    for i in range(len(us)):
        xn, xd, y = out[3 * i:3 * i + 3]
        assert 0 < xd < c.p and xn < c.p and y < c.p, (curve, rows[i])            # canonical, and xd is never zero
        got.append((xn * pow(xd, -1, c.p) % c.p, y))
    bad = first_bad(rows, got, [hm.sswu(s, u) for u in us])
    assert bad is None, (curve, "sswu", bad)


# ---- P: colliding pairs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_p_pair_at_first_middle_and_last_index(eng, curve):
    """each colliding pair at index 0, 32 and 64 of a batch of 65 ordinary pairs: 2 map(u) (on the curve) or the identity as
    out_inf = 1 with an all-zero record there, the neighbours untouched"""
    s = hm.SUITES[curve]
    c = s.curve
    n = 65
    base = ordinary_u(s, 2 * n)
    base_want = [pyec.add(c, model_map(s, base[2 * i]), model_map(s, base[2 * i + 1])) for i in range(n)]
    assert all(P is not pyec.INF for P in base_want)
    rows = hv.family_p(curve, model_map)
    assert len(rows) == 160
    for k, (u0, u1, want_sum, _) in enumerate(rows):
        at = (0, n // 2, n - 1)[k % 3]
        pairs, want = list(base), list(base_want)
        pairs[2 * at], pairs[2 * at + 1] = u0, u1
        want[at] = want_sum
        xy, inf = eng.map_to_curve(c.cid, enc_ints(c, pairs), 2)
        wxy, winf = enc_points(c, want)
        assert bytes(inf) == winf and bytes(xy) == wxy, (curve, k, at, u0, u1)
        rec = bytes(xy[at * 2 * c.L:(at + 1) * 2 * c.L])
        if want_sum is pyec.INF:
            assert inf[at] == 1 and rec == bytes(2 * c.L)
        else:
            assert inf[at] == 0 and pyec.on_curve(c, pyec.dec_point(c, rec, 0))


@pytest.mark.parametrize("curve", hv.CURVES)
def test_family_p_whole_waves_of_colliding_pairs(eng, curve):
    """batches made of colliding pairs only, 64 + 1 rows: a whole wave takes the doubling case, or the identity, together; then
    the two kinds interleaved"""
    s = hm.SUITES[curve]
    c = s.curve
    rows = hv.family_p(curve, model_map)
    dbl = [r for r in rows if r[2] is not pyec.INF]
    opp = [r for r in rows if r[2] is pyec.INF]
    assert len(dbl) == len(opp) == 80
    for what, part in (("doubling", dbl[:65]), ("identity", opp[:65]), ("mixed", rows[:65]), ("mixed", rows[-65:])):
        assert len(part) == 65
        xy, inf = eng.map_to_curve(c.cid, enc_ints(c, [u for r in part for u in r[:2]]), 2)
        wxy, winf = enc_points(c, [r[2] for r in part])
        assert bytes(inf) == winf and bytes(xy) == wxy, (curve, what)


# ---- I: the isogeny on fractions the map never produces ----------------------------------------------------------------------------
def test_family_i_isogeny(eng):
    s = hm.SUITES["k256"]
    c = s.curve
    rows = hv.family_i("k256")
    out = bytes(eng.selftest_h2c(c.cid, OP_ISO, enc_ints(c, [v for r in rows for v in r[1:4]])))
    recs = [out[i * 96:(i + 1) * 96] for i in range(len(rows))]
    got = []
    for rec in recs:
        X, Y, Z = dec_ints(c, rec)
        assert max(X, Y, Z) < c.p
        got.append(pyec.INF if Z == 0 else (X * pow(Z, -1, c.p) % c.p, Y * pow(Z, -1, c.p) % c.p))
    bad = first_bad([r[:4] for r in rows], got, [r[4] for r in rows])
    assert bad is None, bad
    identity = (0).to_bytes(32, "big") + (1).to_bytes(32, "big") + (0).to_bytes(32, "big")
    for r, rec in zip(rows, recs):
        assert (rec == identity) == (r[4] is pyec.INF), r[:4]                      # exactly (0 : 1 : 0), as on the twin
    assert sum(1 for r in rows if r[0] == "forged") >= 26


# ---- the entry point's own errors -------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    mod = ecgpu_module()
    lib, p8 = eng._lib, ctypes.POINTER(ctypes.c_uint8)
    buf, out = np.zeros(3 * 72, np.uint8), np.full(3 * 72, 0xA5, np.uint8)
    pi, po = buf.ctypes.data_as(p8), out.ctypes.data_as(p8)
    one = ctypes.c_size_t(1)
    for cid in (mod.K256, mod.P256, mod.P384):
        for op in (-1, 4, 99):
            assert lib.ecgpu_selftest_h2c(eng._ctx, cid, op, pi, one, po) == ERR_ARG                 # unknown op
        for op in (OP_P, OP_N, OP_SSWU):
            assert lib.ecgpu_selftest_h2c(eng._ctx, cid, op, None, one, po) == ERR_ARG               # a NULL array with n > 0
            assert lib.ecgpu_selftest_h2c(eng._ctx, cid, op, pi, one, None) == ERR_ARG
            assert lib.ecgpu_selftest_h2c(eng._ctx, cid, op, None, ctypes.c_size_t(0), None) == 0    # n = 0 touches nothing
    assert (out == 0xA5).all()
    assert lib.ecgpu_selftest_h2c(eng._ctx, mod.K256, OP_ISO, None, ctypes.c_size_t(0), None) == 0
    for cid in (mod.P256, mod.P384):                                                                 # the isogeny belongs to secp256k1
        assert lib.ecgpu_selftest_h2c(eng._ctx, cid, OP_ISO, pi, one, po) == ERR_CURVE
    for cid in (mod.P521, mod.SM2, mod.P224, mod.BP256, mod.BIGN256, 99):                            # no suite, or no such curve
        for op in (OP_P, OP_N, OP_SSWU, OP_ISO):
            assert lib.ecgpu_selftest_h2c(eng._ctx, cid, op, pi, one, po) == ERR_CURVE
    assert (out == 0xA5).all()
    with pytest.raises(mod.EcgpuError) as e:
        eng.selftest_h2c(mod.P256, OP_ISO, bytes(96))
    assert e.value.code == ERR_CURVE
    with pytest.raises(mod.EcgpuError) as e:
        eng.selftest_h2c(mod.P384, OP_P, bytes(71))                                                  # not a whole record of L = 72
    assert e.value.code == ERR_ARG
    assert eng.selftest_h2c(mod.P384, OP_N, b"").size == 0
    got = eng.selftest_h2c(mod.P256, OP_P, (pyec.P256.p + 5).to_bytes(48, "big"))                    # and a well-formed call
    assert bytes(got) == (5).to_bytes(32, "big")
