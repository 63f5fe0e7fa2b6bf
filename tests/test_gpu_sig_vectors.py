"""-m gpu: the vectors of tests/sig_vectors.py (R chosen, the key derived) through every verification entry point on gfx950.

tests/test_sig_vectors.py holds the same vectors against the big-integer model, the oracle and the CPU build of csrc/ecgpu_verify.h;
here the kernels of csrc/ecgpu_ecdsa.h get them — wire loads, the shared scalar inversions, the a G + b P kernels, the finish —
and must give the verdict of the construction and of the oracle, element for element.  Each scheme and curve runs as one batch of a
few hundred elements (the vectors tiled, no multiple of 64) and again in reversed order: a failed element is replaced by
0 G + 0 G and its neighbours must not notice.  The ECDSA and recovery vectors of k256, p224 and p521 also run tiled over the
smallest prime batch at which every lane of k_scalar_batch_inv owns at least two elements, so that elements which drop out of the
lane's product (s = 0, s = n, s + n, r = 0) and the extremes s = 1, s = n - 1 sit first, in the middle and last in a lane's chain."""
import os
import re
import time

import numpy as np
import pytest

import oracle_lib
import pyec
import sig_vectors as sv
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


_durations = []


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    _durations.append((time.perf_counter() - t0, request.node.name))


@pytest.fixture(scope="module", autouse=True)
def _print_times():
    """Shown with -s or -rA: the slowest cases (generation of a curve's vectors is host time inside the first case that asks) and
    the host seconds sig_vectors took per scheme and curve."""
    yield
    print("\nslowest cases of test_gpu_sig_vectors:")
    for dt, name in sorted(_durations, reverse=True)[:12]:
        print("  %6.2f s  %s" % (dt, name))
    print("host seconds generating the vectors:")
    for (scheme, curve), dt in sorted(sv.GEN_SECONDS.items()):
        print("  %-11s %-8s %5.2f s" % (scheme, curve, dt))


def orders(vec):
    """The vectors tiled to a few hundred elements, no multiple of 64, forwards and reversed"""
    m = len(vec)
    n = 4 * m + 3
    if n % 64 == 0:
        n += 1
    fwd = [vec[i % m] for i in range(n)]
    return fwd, fwd[::-1]


def same(got, want, batch, what):
    got, want = bytes(got), bytes(want)
    assert len(got) == len(want) == len(batch)
    for i, v in enumerate(batch):
        assert got[i] == want[i], (what, i, v.family, v.label, "device %d, expected %d" % (got[i], want[i]))


@pytest.mark.parametrize("curve", sv.ECDSA_CURVES)
def test_ecdsa_verify(eng, curve):
    c = pyec.CURVES[curve]
    for batch in orders(sv.ecdsa_vectors(curve)):
        z, r, s, q, exp, exp_hs = sv.pack_ecdsa(c, batch)
        for high, want in ((False, exp), (True, exp_hs)):
            got = eng.ecdsa_verify(c.cid, z, r, s, q, reject_high_s=high)
            same(got, want, batch, (curve, high))
            same(got, oracle_lib.ecdsa_verify(c.cid, z, r, s, q, high), batch, (curve, high, "oracle"))


@pytest.mark.parametrize("curve", sv.MSG_CURVES)
def test_ecdsa_verify_msg(eng, curve):
    c = pyec.CURVES[curve]
    for ln, part in sv.by_len(sv.ecdsa_msg_vectors(curve)).items():
        for batch in orders(part):
            q, m, sg, exp, exp_hs = sv.pack_ecdsa_msg(c, batch)
            for high, want in ((False, exp), (True, exp_hs)):
                got = eng.ecdsa_verify_msg(c.cid, q, m, ln, sg, reject_high_s=high)
                same(got, want, batch, (curve, ln, high))
                same(got, oracle_lib.ecdsa_verify_msg(c.cid, q, m, ln, sg, high), batch, (curve, ln, high, "oracle"))


def same_keys(c, got_xy, got_ok, want, batch, what):
    want_xy, want_ok = want
    same(got_ok, want_ok, batch, what)
    got_xy, w = bytes(got_xy), 2 * c.L
    for i, v in enumerate(batch):
        assert got_xy[i * w:(i + 1) * w] == bytes(want_xy[i * w:(i + 1) * w]), (what, i, v.family, v.label)


@pytest.mark.parametrize("curve", sv.ECDSA_CURVES)
def test_ecdsa_recover(eng, curve):
    c = pyec.CURVES[curve]
    for batch in orders(sv.recover_vectors(curve)):
        z, r, s, recid, plain, high_s = sv.pack_recover(c, batch)
        for high, want in ((False, plain), (True, high_s)):
            out, ok = eng.ecdsa_recover(c.cid, z, r, s, recid, reject_high_s=high)
            same_keys(c, out, ok, want, batch, (curve, high))
            same_keys(c, out, ok, oracle_lib.ecdsa_recover(c.cid, z, r, s, recid, high), batch, (curve, high, "oracle"))


def test_schnorr_verify(eng):
    for batch in orders(sv.schnorr_vectors("k256")):
        e, r, s, pxy, exp = sv.pack_schnorr(batch)
        got = eng.schnorr_verify(e, r, s, pxy)
        want_o = bytes(oracle_lib.schnorr_verify(e, r, s, pxy))
        same(got, want_o, batch, "oracle")
        same(got, bytes(want_o[i] if x == 2 else x for i, x in enumerate(exp)), batch, "construction")   # 2: odd-y key, the oracle decides


def test_schnorr_verify_raw(eng):
    for ln, part in sv.by_len(sv.schnorr_raw_vectors("k256")).items():
        for batch in orders(part):
            pk, m, sg, exp = sv.pack_schnorr_raw(batch)
            got = eng.schnorr_verify_raw(pk, m, ln, sg)
            same(got, exp, batch, ln)
            same(got, oracle_lib.schnorr_verify_raw(pk, m, ln, sg), batch, (ln, "oracle"))


def test_sm2dsa_verify(eng):
    for batch in orders(sv.sm2dsa_vectors("sm2")):
        e, r, s, q, exp = sv.pack_sm2dsa(batch)
        got = eng.sm2dsa_verify(e, r, s, q)
        same(got, exp, batch, "sm2dsa")
        same(got, oracle_lib.sm2dsa_verify(e, r, s, q), batch, "oracle")


def test_bign_verify(eng):
    for batch in orders(sv.bign_vectors("bign256")):
        h, sg, q, exp = sv.pack_bign(batch)
        got = eng.bign_verify(h, sg, q)
        same(got, exp, batch, "bign")
        same(got, oracle_lib.bign_verify(h, sg, q), batch, "oracle")


def test_bign_verify_msg(eng):
    for ln, part in sv.by_len(sv.bign_msg_vectors("bign256")).items():
        for batch in orders(part):
            q, m, sg, exp = sv.pack_bign_msg(batch)
            got = eng.bign_verify_msg(q, m, ln, sg)
            same(got, exp, batch, ln)
            same(got, oracle_lib.bign_verify_msg(q, m, ln, sg), batch, (ln, "oracle"))


# ---- the shared scalar inversions: chains of several elements per lane ------------------------------------------------------
def is_prime(v):
    return v > 1 and all(v % d for d in range(2, int(v ** 0.5) + 1))


def next_prime(v):
    while not is_prime(v):
        v += 1
    return v


def chain_plan():
    """(n, lanes, per lane): the smallest prime batch at which every lane of k_scalar_batch_inv owns at least two elements, by the
    rule of launch_scalar_batch_inv as the source states it (k = ceil(n / 65536) elements per lane, lanes = ceil(n / k), lane t owns
    t, t + lanes, ...).  With k = 2 a batch of odd length leaves the last lane one element, so a prime batch needs k = 3."""
    with open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_inst_base.hip")) as f:
        body = f.read().split("static void launch_scalar_batch_inv", 1)[1].split("\n}", 1)[0]
    m = re.search(r"size_t k = \(n \+ (\d+)\) / (\d+);\s*if \(k > (\d+)\) k = \d+;\s*const size_t nthreads = \(n \+ k - 1\) / k;", body)
    assert m and int(m.group(1)) + 1 == int(m.group(2)), "launch_scalar_batch_inv no longer states its lane rule this way"
    per = int(m.group(2))
    n = per + 1
    while True:
        n = next_prime(n)
        k = min(-(-n // per), int(m.group(3)))
        lanes = -(-n // k)
        if k >= 2 and n - 1 - (lanes - 1) >= lanes:               # the last lane's second element exists
            return n, lanes, k
        n += 1


def chain_positions(n, lanes, m, case):
    """the positions (0 = first, k - 1 = last in the forward pass) that copies of tile element `case` take in their lanes' chains"""
    return {j // lanes for j in range(case, n, m)}


@pytest.mark.parametrize("curve", ["k256", "p224", "p521"])
def test_inversion_chains(eng, curve):
    c = pyec.CURVES[curve]
    L = c.L
    n, lanes, k = chain_plan()
    assert k == 3 and 2 * 65536 < n < 2 * 65536 + 200
    vec = list(sv.ecdsa_vectors(curve))
    vec += vec[: next_prime(len(vec)) - len(vec)]                  # a tile of prime length: a lane's elements are different cases
    m = len(vec)
    assert lanes % m
    dropped = [i for i, v in enumerate(vec) if v.s % c.n == 0 or v.s >= c.n]
    assert {vec[i].label for i in dropped} >= {"s = 0", "s = n", "s + n"}
    for i in dropped + [i for i, v in enumerate(vec) if v.s in (1, c.n - 1)]:
        assert chain_positions(n, lanes, m, i) == set(range(k))   # first, middle and last of a chain
    z, r, s, q, exp, _ = sv.pack_ecdsa(c, vec)
    same(eng.ecdsa_verify(c.cid, z, r, s, q), exp, vec, (curve, "small"))
    reps = n // m + 1
    big = eng.ecdsa_verify(c.cid, (z * reps)[: n * L], (r * reps)[: n * L], (s * reps)[: n * L], (q * reps)[: n * 2 * L])
    bad = np.nonzero(np.asarray(big) != np.tile(np.frombuffer(exp, np.uint8), reps)[:n])[0]
    assert bad.size == 0, (curve, [(int(j), vec[j % m].label) for j in bad[:8]])

    rvec = list(sv.recover_vectors(curve))
    rvec += rvec[: next_prime(len(rvec)) - len(rvec)]
    m = len(rvec)
    assert lanes % m
    dropped = [i for i, v in enumerate(rvec) if v.r % c.n == 0 or v.r >= c.n]       # recovery inverts r
    assert {rvec[i].label for i in dropped} >= {"r = 0", "r = n"}
    for i in dropped:
        assert chain_positions(n, lanes, m, i) == set(range(k))
    z, r, s, recid, (want_xy, want_ok), _ = sv.pack_recover(c, rvec)
    out, ok = eng.ecdsa_recover(c.cid, z, r, s, recid)
    same_keys(c, out, ok, (want_xy, want_ok), rvec, (curve, "small"))
    reps = n // m + 1
    out, ok = eng.ecdsa_recover(c.cid, (z * reps)[: n * L], (r * reps)[: n * L], (s * reps)[: n * L], (recid * reps)[:n])
    assert bytes(ok) == (want_ok * reps)[:n]
    assert bytes(out) == (want_xy * reps)[: n * 2 * L]
