"""-m gpu: the part of the MSM behind the buckets on gfx950, on the vectors of tests/msm_tail_vectors.py.

Ops 20 - 22 of ecgpu_selftest_point (csrc/ecgpu_selftest_msm.h) give RowsK256::mul, RowsK256::norm64 and RowsDblK256's enter / step /
leave raw limbs and return raw limbs: the device's limbs must be the limbs of tools/rows_field_model.py, limb for limb, below the
bound the header states, and the integers mod p.  Ops 23 - 26 run msm_hom_add_quad, msm_block_sum and msm_jac_dbl_lanes on chosen
points: against tests/pyec.py, against the per-lane Group::add / Group::dbl / jac_dbl of the older ops on the same inputs, and every
copy in a quad / wave equal.  The Horner chain of k_msm_combine: term lists whose accumulator cancels, meets an equal point, changes
sign or idles through empty windows at a chosen window (one `lincomb` each with the window width forced), two ranks whose parts
cancel, adjacent buckets — against the dot product (sum k_i s_i) G, which knows nothing of windows.  k256 on its GLV halves through
the product library and on the plain scalar through the tool build with ECGPU_MSM_GLV=0, as tests/test_gpu_scalar_vectors.py does."""
import time

import numpy as np
import pytest

import msm_tail_vectors as mt
import pyec
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu

K = pyec.K256
# the sets whose k_msm_combine takes msm_jac_dbl_lanes: a = -3 and no A_GENERIC in csrc/ecgpu_params.h (the Brainpool twists and
# bign256 carry it: they run the one-lane chain, as bp256 does)
MINUS3_SETS = ["p256", "p384", "sm2", "p224", "p192", "p521"]
CHAIN_SETS = [("k256", True), ("k256", False), ("p256", False), ("p384", False), ("p521", False), ("bp256", False)]


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keng():
    """The tool build of the library (tuning knobs read from the environment): k256 on the plain folded scalar."""
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
    print("\nslowest cases of test_gpu_msm_tail:")
    for dt, name in sorted(_durations, reverse=True)[:12]:
        print("  %6.2f s  %s" % (dt, name))


def raw(eng, op, pwords, qwords):
    """ecgpu_selftest_point on raw 16-word records -> an (n, 16) array of result words"""
    p = np.array(pwords, "<u4").view(np.uint8)
    q = np.array(qwords, "<u4").view(np.uint8)
    out, inf = eng.selftest_point(K.cid, op, p, None, q)
    assert not inf.any()
    return np.asarray(out).view("<u4").reshape(-1, 16)


def in_fours(items):
    items = list(items)
    items += items[: (-len(items)) % 4]
    return [items[i: i + 4] for i in range(0, len(items), 4)]


# ---- the row field, limb for limb ---------------------------------------------------------------------------------------------------

def test_device_row_mul_limbs_equal_the_model(eng):
    """Op 20 on every row-multiplication vector, four different pairs per wave (the other sixty lanes hold junk that must not matter):
    all 64 lanes of a wave return the product of row (lane mod 4), whose nine limbs are the model's nine limbs."""
    vec = mt.row_mul_vectors()
    mt.check_coverage_rows(vec)
    waves = in_fours(vec)
    got = raw(eng, 20, mt.raw_records([[v[3] for v in w] for w in waves]), mt.raw_records([[v[4] for v in w] for w in waves], 0xB0B))
    bad = []
    for wi, w in enumerate(waves):
        want = [mt.row_mul_expected(v[3], v[4]) for v in w]
        for lane in range(64):
            g = [int(x) for x in got[64 * wi + lane]]
            v, wl = w[lane % 4], want[lane % 4]
            assert g[9:] == [0] * 7
            value_ok = mt.value(g[:9]) % mt.P == mt.value(v[3]) * mt.value(v[4]) % mt.P
            if g[:9] != wl or max(g[:9]) >= mt.LB or not value_ok:
                bad.append("%s, lane %d: device %s, model %s; value %s, limbs below LB: %s" % (
                    v[0], lane, [hex(x) for x in g[:9]], [hex(x) for x in wl], "agrees" if value_ok else "DIFFERS", max(g[:9]) < mt.LB))
    assert not bad, "%d lanes differ; first: %s" % (len(bad), bad[0])


def test_device_norm64_limbs_equal_the_model(eng):
    vec = mt.norm64_vectors()
    waves = in_fours(vec)
    lo = mt.raw_records([[[x & 0xFFFFFFFF for x in v[1]] for v in w] for w in waves])
    hi = mt.raw_records([[[x >> 32 for x in v[1]] for v in w] for w in waves], 0xB0B)
    got = raw(eng, 21, lo, hi)
    for wi, w in enumerate(waves):
        for lane in range(64):
            g = [int(x) for x in got[64 * wi + lane]][:9]
            label, v = w[lane % 4]
            assert g == mt.norm64_expected(v), (label, lane, [hex(x) for x in g])
            assert max(g) < 2 * mt.LB and mt.value(g) % mt.P == mt.value(v) % mt.P, (label, lane)


@pytest.mark.parametrize("steps", mt.DBL_STEPS)
def test_device_row_doubling_chain_limbs_equal_the_model(eng, steps):
    """Op 22: X, Y, Z as 27 raw limbs at magnitudes up to (2, 2, 1) -> enter, `steps` doublings, leave: the 27 limbs of the model,
    X and Z below LB, Y below 2 LB, the values of the doubling formulas on integers; every lane of the wave holds the same point."""
    vec = mt.dbl_vectors()
    got = raw(eng, 22 | steps << 8, mt.raw_records([[v[1], v[2], v[3]] for v in vec]), [0] * (16 * 64 * len(vec)))
    for wi, (label, X, Y, Z) in enumerate(vec):
        limbs, values = mt.dbl_expected(X, Y, Z, steps)
        for lane in range(64):
            g = [int(x) for x in got[64 * wi + lane]][:9]
            which = lane % 3
            assert g == limbs[which], (label, steps, lane, "XYZ"[which], [hex(x) for x in g], [hex(x) for x in limbs[which]])
            assert max(g) < (2 * mt.LB if which == 1 else mt.LB) and mt.value(g) % mt.P == values[which]


def test_device_raw_ops_reject_partial_waves_and_other_sets(eng):
    ecgpu = ecgpu_module()
    rec = np.zeros(64 * 63, np.uint8)
    for op in (20, 21, 22 | 1 << 8, 23, 25):
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.selftest_point(K.cid, op, rec, None, rec)
        assert e.value.code == ecgpu.ERR_ARG
    for name, op in (("p256", 20), ("p256", 23), ("k256", 26 | 1 << 8), ("bp256", 26 | 1 << 8), ("bp256t1", 26 | 1 << 8), ("k256", 27)):
        c = pyec.CURVES[name]
        rec = np.frombuffer(pyec.enc_point(c, pyec.G(c))[0] * 64, np.uint8)
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.selftest_point(c.cid, op, rec, None, rec)
        assert e.value.code == ecgpu.ERR_SCALAR_RANGE, (name, op)


# ---- the quad addition, the tree, the lane-shared doubling ---------------------------------------------------------------------------

def enc_points(c, pts):
    return (np.frombuffer(b"".join(pyec.enc_point(c, x)[0] for x in pts), np.uint8), np.array([pyec.enc_point(c, x)[1] for x in pts], np.uint8))


def dec_points(c, out, inf):
    return [pyec.dec_point(c, bytes(out[2 * c.L * i: 2 * c.L * (i + 1)]), int(inf[i])) for i in range(len(inf))]


def spread_over_quads(c, firsts, others, per):
    """`firsts` in the first lane of consecutive groups of `per` lanes, `others` (which must not matter) in the rest; padded to whole
    waves"""
    out = []
    for i, f in enumerate(firsts):
        out += [f] + [others[(i + j) % len(others)] for j in range(per - 1)]
    while len(out) % 64:
        out.append(others[0])
    return out


def test_device_quad_addition_on_every_edge_pair(eng):
    """Op 23: msm_hom_add_quad on P + P, P - P, O + P, P + O, O + O and generic pairs — a different pair in every quad of a wave, the
    other three lanes of the quad holding other points — against pyec, against Group::add (op 0) on the same pairs, all four copies
    equal.  Op 24: generic Z on both sides, X = Group::add(P, Q), Y = Group::dbl(Q), with X = Y, X = -Y and X = O among them."""
    c = K
    junk = [p for _, p in mt.base_points("k256")][::-1] + [pyec.INF]
    pairs = mt.quad_pairs("k256")
    P = spread_over_quads(c, [a for a, _ in pairs], junk, 4)
    Q = spread_over_quads(c, [b for _, b in pairs], junk[3:] + junk[:3], 4)
    pxy, pinf = enc_points(c, P)
    qxy, qinf = enc_points(c, Q)
    got = dec_points(c, *eng.selftest_point(c.cid, 23, pxy, pinf, qxy, qinf))
    lanewise = dec_points(c, *eng.selftest_point(c.cid, 0, pxy, pinf, qxy, qinf))
    for i, (a, b) in enumerate(pairs):
        want = pyec.add(c, a, b)
        assert lanewise[4 * i] == want
        assert got[4 * i: 4 * i + 4] == [want] * 4, (i, a, b, got[4 * i: 4 * i + 4])
    trip = mt.quad_pairs_generic("k256")
    P = spread_over_quads(c, [t[0] for t in trip], junk, 4)
    Q = spread_over_quads(c, [t[1] for t in trip], junk[5:] + junk[:5], 4)
    pxy, pinf = enc_points(c, P)
    qxy, qinf = enc_points(c, Q)
    got = dec_points(c, *eng.selftest_point(c.cid, 24, pxy, pinf, qxy, qinf))
    x, xi = eng.selftest_point(c.cid, 0, pxy, pinf, qxy, qinf)                  # the same by the per-lane formulas of the older ops
    y, yi = eng.selftest_point(c.cid, 2, qxy, qinf)
    lanewise = dec_points(c, *eng.selftest_point(c.cid, 0, x, xi, y, yi))
    for i, (a, b, want) in enumerate(trip):
        assert lanewise[4 * i] == want
        assert got[4 * i: 4 * i + 4] == [want] * 4, (i, got[4 * i: 4 * i + 4], want)


def test_device_quad_tree_sums_a_workgroup(eng):
    """Op 25: msm_block_sum over the 256 points of a workgroup (the first level per lane, the other seven on quads): random multiples
    with identities and opposite pairs among them, 256 times the same point (equal points at every level), P, -P alternating (the
    identity at the first level, identities all the way up), one point among identities, the identity first."""
    c = K
    n = c.n
    bp = mt.base_points("k256")
    logs = []
    blocks = [[bp[(7 * i) % len(bp)][0] * (i + 1) % n if i % 9 else 0 for i in range(256)],
              [bp[8][0]] * 256,
              [bp[9][0] if i % 2 == 0 else n - bp[9][0] for i in range(256)],
              [0] * 255 + [5],
              [0] + [bp[10][0]] * 127 + [n - bp[10][0]] * 127 + [3]]
    G = pyec.G(c)
    cache = {}
    pts = []
    for blk in blocks:
        for s in blk:
            if s not in cache:
                cache[s] = pyec.mul(c, s, G) if s else pyec.INF
            pts.append(cache[s])
        logs.append(sum(blk) % n)
    pxy, pinf = enc_points(c, pts)
    got = dec_points(c, *eng.selftest_point(c.cid, 25, pxy, pinf, pxy, pinf))
    for b, lg in enumerate(logs):
        assert got[256 * b] == (pyec.mul(c, lg, G) if lg else pyec.INF), b
        assert all(g is pyec.INF for g in got[256 * b + 1: 256 * b + 256])
    assert logs[2] == 0 and logs[0] != 0


@pytest.mark.parametrize("name", MINUS3_SETS)
def test_device_lane_shared_doubling(eng, name):
    """Op 26 on every set whose k_msm_combine takes msm_jac_dbl_lanes (p521's 17 limbs included): the wave's first point — the
    identity first, then G, -G, small and random multiples, with a generic Z (P + Q) and with Z = 1 — through (X Z : Y Z^2 : Z), s
    doublings shared by lanes 0 .. 2, jac_to_proj: 2^s (P + Q) in all 64 lanes; s = 1 also against jac_dbl (op 6) on the same point."""
    c = pyec.CURVES[name]
    G = pyec.G(c)
    bp = mt.base_points(name)
    firsts = [(0, 0), (0, 5), (7, 0), (1, c.n - 1)] + [(bp[i][0], bp[(i + 3) % len(bp)][0]) for i in range(len(bp))]
    others = [p for _, p in bp]
    cache = {0: pyec.INF}
    pt = lambda s: cache.setdefault(s, pyec.mul(c, s, G) if s else pyec.INF)
    P = spread_over_quads(c, [pt(a) for a, _ in firsts], others, 64)
    Q = spread_over_quads(c, [pt(b) for _, b in firsts], others[4:] + others[:4], 64)
    pxy, pinf = enc_points(c, P)
    qxy, qinf = enc_points(c, Q)
    for steps in (1, 4, 13, 16):
        got = dec_points(c, *eng.selftest_point(c.cid, 26 | steps << 8, pxy, pinf, qxy, qinf))
        for i, (a, b) in enumerate(firsts):
            want = pt((a + b) * (1 << steps) % c.n)
            assert got[64 * i: 64 * i + 64] == [want] * 64, (name, steps, i, a, b)
        got = dec_points(c, *eng.selftest_point(c.cid, 26 | steps << 8, pxy, pinf))               # Z = 1
        for i, (a, _) in enumerate(firsts):
            assert got[64 * i: 64 * i + 64] == [pt(a * (1 << steps) % c.n)] * 64, (name, steps, i, a)
    finite = [i for i, (a, _) in enumerate(firsts) if a]
    lanewise = dec_points(c, *eng.selftest_point(c.cid, 6, pxy, pinf))
    got = dec_points(c, *eng.selftest_point(c.cid, 26 | 1 << 8, pxy, pinf))
    assert all(got[64 * i + 5] == lanewise[64 * i] for i in finite)


# ---- the Horner chain ---------------------------------------------------------------------------------------------------------------

def engine_for(eng, keng, name, glv, monkeypatch):
    if name == "k256" and not glv:
        monkeypatch.setenv("ECGPU_MSM_GLV", "0")
        assert (keng.msm_plan_window(0, 1 << 19), keng.msm_plan_window(0, 1 << 12)) == (13, 9)
        return keng
    return eng


def enc_case(c, case):
    scal = np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in case.ks), np.uint8)
    pxy, pinf = enc_points(c, case.points)
    return scal, pxy, pinf


def want_of(c, log):
    return pyec.mul(c, log, pyec.G(c)) if log else pyec.INF


def chain_windows(name, glv, cbits):
    """every window at the widths the plan picks, a sample at c = 4"""
    return mt.event_windows(name, glv, cbits, sample=cbits == 4)


CHAIN_CASES = [(name, glv, cbits, kind) for name, glv in CHAIN_SETS for cbits in (13, 16, 4) for kind in mt.EVENTS]


@pytest.mark.parametrize("name,glv,cbits,kind", CHAIN_CASES,
                         ids=["%s-%s-%d-%s" % (n, "glv" if g else "plain", cb, k) for n, g, cb, k in CHAIN_CASES])
def test_device_horner_chain_events(eng, keng, name, glv, cbits, kind, monkeypatch):
    """One event kind planted at every window (c = 13, 16) or at top - 1, a straddling window, the middle, 1 and 0 (c = 4, the longest
    chain): each term list is one lincomb with the width forced, against the dot product; the first also with the automatic plan
    (the small-MSM path) as a control."""
    c = pyec.CURVES[name]
    e = engine_for(eng, keng, name, glv, monkeypatch)
    cases = mt.cases_for(name, glv, cbits, kind, chain_windows(name, glv, cbits))
    assert cases
    try:
        e.set_msm_window(cbits)
        for case in cases:
            mt.check_coverage_chain(case)
            scal, pxy, pinf = enc_case(c, case)
            assert e.msm_plan_window(c.cid, len(case.ks)) == cbits
            o, f = e.lincomb(c.cid, scal, pxy, pinf)
            got = pyec.dec_point(c, bytes(o), f)
            assert got == want_of(c, case.want_log), "%s %s c = %d, %s planted at %r: the chain gives %r" % (
                name, "GLV" if glv else "plain", cbits, kind, case.planted, got)
    finally:
        e.set_msm_window(0)
    scal, pxy, pinf = enc_case(c, cases[0])
    o, f = e.lincomb(c.cid, scal, pxy, pinf)
    assert pyec.dec_point(c, bytes(o), f) == want_of(c, cases[0].want_log), (name, glv, cbits, kind, "automatic plan")


TWO_RANK = [(name, glv, leave) for name, glv in (("k256", True), ("p256", False), ("bp256", False)) for leave in (None, 0, 3)]


@pytest.mark.parametrize("name,glv,leave", TWO_RANK, ids=["%s-%s" % (n, "all" if l is None else "but-%d" % l) for n, _, l in TWO_RANK])
def test_device_two_ranks_cancel_in_every_window(eng, name, glv, leave):
    """ecgpu_msm_parts_dev on two shards, the second the first with every point negated (every window: the identity out of
    non-identity parts, met in k_msm_window_sums) — and the same with one window left standing —, ecgpu_msm_finish_dev over both."""
    c = pyec.CURVES[name]
    L = c.L
    a, b, want = mt.two_rank_terms(name, glv, 13, leave)
    plan_terms = max(len(a.ks), len(b.ks))
    pad = lambda x: (x + 15) // 16 * 16
    try:
        eng.set_msm_window(13)
        nbytes = eng.msm_parts_bytes(c.cid, plan_terms)
        d_all = eng.dev_alloc(2 * nbytes)
        for r, case in enumerate((a, b)):
            bufs = [eng.to_device(x) for x in enc_case(c, case)]
            eng.msm_parts_dev(c.cid, bufs[0], bufs[1], bufs[2], len(case.ks), plan_terms, d_all.at(r * nbytes))
            for x in bufs:
                x.free()
        d_o, d_f = eng.dev_alloc(pad(2 * L)), eng.dev_alloc(16)
        eng.msm_finish_dev(c.cid, d_all, 2, plan_terms, d_o, d_f)
        got = pyec.dec_point(c, bytes(eng.to_host(d_o, 2 * L)), int(eng.to_host(d_f, 1)[0]))
        for x in (d_all, d_o, d_f):
            x.free()
    finally:
        eng.set_msm_window(0)
    assert got == want_of(c, want), (name, leave)


BUCKETS = [(name, glv, cbits) for name, glv in (("k256", True), ("k256", False), ("p256", False)) for cbits in (9, 13)]


@pytest.mark.parametrize("name,glv,cbits", BUCKETS, ids=["%s-%s-%d" % (n, "glv" if g else "plain", cb) for n, g, cb in BUCKETS])
def test_device_adjacent_buckets(eng, keng, name, glv, cbits, monkeypatch):
    """The same point, and opposite points, in two adjacent buckets of one window: inside a segment of the bucket reduction, across
    segment boundaries, and in the highest live window (the top window's sub-buckets where the layout has them)."""
    c = pyec.CURVES[name]
    e = engine_for(eng, keng, name, glv, monkeypatch)
    G = pyec.G(c)
    try:
        e.set_msm_window(cbits)
        for label, ks, ss in mt.bucket_cases(name, glv, cbits):
            scal = np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in ks), np.uint8)
            pxy, pinf = enc_points(c, [pyec.mul(c, s, G) for s in ss])
            o, f = e.lincomb(c.cid, scal, pxy, pinf)
            assert pyec.dec_point(c, bytes(o), f) == want_of(c, sum(k * s for k, s in zip(ks, ss)) % c.n), (name, glv, cbits, label)
    finally:
        e.set_msm_window(0)
