"""-m gpu: the adversarial inversion inputs of tests/modinv_vectors.py on gfx950, all twelve parameter sets.  What only the device has
in csrc/ecgpu_modinv.h: the division steps as v_mad_u64_u32 on register pairs whose upper halves hold garbage, the matrix updates as
v_mad_i64_i32 written by hand, and invert_var's wave ballot.  tests/test_modinv_vectors.py runs the same vectors through the model
and the g++ twin, so a failure here alone is one of those three.

  * the self-test ops: field 4 (F::inv) and 17 (F::inv<true>) on the canonical operand that hands each vector to the division
    steps, the raw-domain 46 and 47 on the vector itself and on vector + p, scalar 41 on the vectors mod n.  Exact; a mismatch
    names the first differing vector.
  * op 17 / 47 with every wave of 64 holding the inputs that finish earliest (1, 0, p) beside those that finish latest (batch counts
    by the model): a lane that is done goes on taking batches until the ballot of its wave is empty.
  * in situ at the smallest sizes that reach each kernel: batch_normalize and mul_xyz (scalar 1) on records (x z, y z, z) with z
    running over the vectors — one record per lane, and chains of two through the tool build — and ecdsa_verify with s running
    over the vectors mod n, signatures valid by construction (z = s k - r d), one inversion per lane and, tiled past 65,536, through
    k_scalar_batch_inv's one inversion of a lane's product."""
import time

import numpy as np
import pytest

import modinv_vectors as mv
import pyec
from gpu_common import ALL_CURVES, ecgpu_module

pytestmark = pytest.mark.gpu

mm = mv.mm
ECDSA_SETS = [c for c in ALL_CURVES if c != "sm2"]           # every parameter set with ECDSA (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keng():
    """the tool build: ECGPU_NORM_K read from the environment (tests/test_gpu_lane_chains.py)"""
    e = ecgpu_module().Engine(0, variant="knobs")
    yield e
    e.close()


_durations = []


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    _durations.append((time.perf_counter() - t0, request.node.name))


@pytest.fixture(scope="module", autouse=True)
def _print_slowest():
    """The slowest cases of this module, printed when it is done (shown with -s or -rA): a case is meant to stay below about 5 s."""
    yield
    print("\nslowest cases of test_gpu_modinv_vectors:")
    for dt, name in sorted(_durations, reverse=True)[:12]:
        print("  %6.2f s  %s" % (dt, name))


def _arr(c, vals):
    return np.frombuffer(mv.enc(c, vals), np.uint8)


def _op(eng, c, op, vals):
    return mv.dec(c, eng.selftest_field(c.cid, op, _arr(c, vals)))


def raw_operands(name):
    c = pyec.CURVES[name]
    xs = mv.all_vectors(name, "p")
    lim = mv.raw_lim(name)
    return xs + [0, c.p] + [v + c.p for v in xs if v + c.p < lim]


@pytest.mark.parametrize("name", mv.CURVES)
def test_device_field_inversions_on_every_vector(eng, name):
    c = pyec.CURVES[name]
    xs = mv.all_vectors(name, "p")
    a = [mv.canonical_operand(name, v) for v in xs]
    want = [mv.want_field_inv(name, v) for v in xs]
    for op in (4, 17):
        msg = mv.first_mismatch(name, "op %d" % op, xs, _op(eng, c, op, a), want)
        assert msg is None, msg
    ws = raw_operands(name)
    want = [mv.want_raw_inv(name, w) for w in ws]
    for op in (46, 47):
        msg = mv.first_mismatch(name, "op %d" % op, ws, _op(eng, c, op, ws), want)
        assert msg is None, msg


@pytest.mark.parametrize("name", mv.CURVES)
def test_device_scalar_inversion_on_every_vector(eng, name):
    c = pyec.CURVES[name]
    xs = mv.all_vectors(name, "n")
    msg = mv.first_mismatch(name, "op 41", xs, _op(eng, c, 41, xs), [pow(x, -1, c.n) if x else 0 for x in xs])
    assert msg is None, msg


def mixed_waves(name):
    """The raw operands laid out so that every wave of 64 holds the earliest-finishing inputs (0, p, 1 and the fewest batches
    of the variable form, by the model) beside the latest-finishing ones; padded to whole waves with 1."""
    c = pyec.CURVES[name]
    ws = [w for w in raw_operands(name) if w not in (0, 1, c.p)]
    red = lambda vals: [w % c.p for w in vals]                 # (F::inv's pack reduces in front of the division steps)
    _, tr = mm.invert_var(red(ws), c.p, mv.nw(name), wave=1, check=False, check_result=False)
    order = [ws[j] for j in np.argsort(tr.batches, kind="stable")]
    longest = int(tr.batches.max())
    late = order[::-1]
    waves = []
    for k in range(0, (len(order) + 1) // 2, 30):
        w = [1, 0, c.p, late[0]] + order[k: k + 30] + late[k: k + 30]
        waves.append(w + [1] * (64 - len(w)))
    lanes = [x for w in waves for x in w]
    assert len(lanes) % 64 == 0 and set(ws) <= set(lanes)
    # the model on this very layout: every wave runs as long as the longest input, and its early lanes wait for it
    _, trw = mm.invert_var(red(lanes), c.p, mv.nw(name), wave=64, check=False)
    assert longest == trw.batches.max() and (trw.took == longest).all() and (trw.batches.reshape(-1, 64).min(axis=1) == 0).all()
    return lanes


@pytest.mark.parametrize("name", mv.CURVES)
def test_device_variable_form_waves_mix_early_and_late(eng, name):
    """ops 47 and 17 (the ballot path the host twin cannot take): the lanes of a wave leave invert_var's loop together, so 1, 0 and
    p run every batch of the family S maximum beside them, and must come out as if they had stopped."""
    c = pyec.CURVES[name]
    lanes = mixed_waves(name)
    msg = mv.first_mismatch(name, "op 47, mixed waves", lanes, _op(eng, c, 47, lanes), [mv.want_raw_inv(name, w) for w in lanes])
    assert msg is None, msg
    canon = [mv.canonical_operand(name, w % c.p) for w in lanes]
    msg = mv.first_mismatch(name, "op 17, mixed waves", lanes, _op(eng, c, 17, canon), [mv.want_field_inv(name, w % c.p) for w in lanes])
    assert msg is None, msg


# ---- in situ ----------------------------------------------------------------------------------------------------------------------

def xyz_records(name):
    """(records X || Y || Z = (x z, y z, z) with (x, y) = G and z the canonical operand of every non-zero vector, the affine G)"""
    c = pyec.CURVES[name]
    p = c.p
    zs = [mv.canonical_operand(name, v) for v in mv.all_vectors(name, "p") if v % p]
    assert 64 < len(zs) <= 4096
    rec = b"".join(mv.enc(c, [c.gx * z % p, c.gy * z % p, z]) for z in zs)
    return zs, np.frombuffer(rec, np.uint8), mv.enc(c, [c.gx, c.gy])


def _check_affine(name, what, zs, out, inf, g):
    c = pyec.CURVES[name]
    assert not np.asarray(inf).any(), (name, what, "a finite record came back as the identity")
    out = np.asarray(out).reshape(len(zs), 2 * c.L)
    bad = [i for i in range(len(zs)) if bytes(out[i]) != g]
    assert not bad, "%s %s: %d of %d records differ, first at %d: z = %#x (the inversion receives %#x), got %s" % (
        name, what, len(bad), len(zs), bad[0], zs[bad[0]], zs[bad[0]] * mv.mont_r(name) % c.p, bytes(out[bad[0]]).hex())


@pytest.mark.parametrize("name", mv.CURVES)
def test_device_normalize_and_xyz_ladder_on_every_vector(eng, keng, name, monkeypatch):
    """k_normalize with one record per lane (n <= 4,096) and with chains of two (ECGPU_NORM_K = 2 on the tool build: the lane
    inverts the product of two vectors), and k_xyz_affine in front of the constant-time ladder (scalar 1)."""
    c = pyec.CURVES[name]
    zs, rec, g = xyz_records(name)
    _check_affine(name, "batch_normalize", zs, *eng.batch_normalize(c.cid, rec), g)
    monkeypatch.setenv("ECGPU_NORM_K", "2")
    try:
        _check_affine(name, "batch_normalize, K = 2", zs, *keng.batch_normalize(c.cid, rec), g)
    finally:
        monkeypatch.delenv("ECGPU_NORM_K")
    one = _arr(c, [1] * len(zs))
    _check_affine(name, "mul_xyz", zs, *eng.mul_xyz(c.cid, one, rec, constant_time=True), g)


def _next_prime(n):
    while any(n % q == 0 for q in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


@pytest.mark.parametrize("name", ECDSA_SETS)
def test_device_ecdsa_verify_with_s_on_every_vector(eng, name):
    """s runs over the vectors mod n; with r = x(k G) mod n and z = s k - r d every signature is valid, and none is with s + 1
    (but for s = (n - 1) / 2, where s + 1 = -s).
    Once with one inversion per lane (n <= 65,536), once tiled to a prime count above 65,537 (k_scalar_batch_inv: several signatures
    per lane, one inversion of their product)."""
    c = pyec.CURVES[name]
    n = c.n
    d, k = 0x1D5 + 977 * c.cid, 0xC0DE + 31 * c.cid
    G = pyec.G(c)
    Q, R = pyec.mul(c, d, G), pyec.mul(c, k, G)
    r = R[0] % n
    assert r
    ss = [s for s in mv.all_vectors(name, "n") if s]
    zz = [(s * k - r * d) % n for s in ss]
    m = len(ss)
    be = lambda vals: b"".join(v.to_bytes(c.L, "big") for v in vals)
    q = be([Q[0], Q[1]])
    Z, Rr, S, Qq = be(zz), be([r] * m), be(ss), q * m
    ok = eng.ecdsa_verify(c.cid, Z, Rr, S, Qq)
    bad = np.nonzero(np.asarray(ok) != 1)[0]
    assert not len(bad), "%s: %d of %d valid signatures rejected, first s = %#x" % (name, len(bad), m, ss[bad[0]])
    ok = eng.ecdsa_verify(c.cid, Z, Rr, be([s + 1 for s in ss]), Qq)
    # (r, s + 1) is valid exactly where s + 1 = -s mod n, the other s of the same signature: s = (n - 1) / 2, which family L holds
    twin = np.array([(2 * s + 1) % n == 0 for s in ss], np.uint8)
    assert twin.sum() == 1
    bad = np.nonzero(np.asarray(ok) != twin)[0]
    assert not len(bad), "%s: %d wrong verdicts with s + 1, first s = %#x" % (name, len(bad), ss[bad[0]])
    big = _next_prime(65537 + 1000)
    reps = big // m + 1
    ok = eng.ecdsa_verify(c.cid, (Z * reps)[: big * c.L], (Rr * reps)[: big * c.L], (S * reps)[: big * c.L], (Qq * reps)[: big * 2 * c.L])
    bad = np.nonzero(np.asarray(ok) != 1)[0]
    assert not len(bad), "%s, %d signatures: %d valid ones rejected, first at %d, s = %#x" % (name, big, len(bad), bad[0], ss[bad[0] % m])
