"""-m gpu: the adversarial scalars of tests/scalar_vectors.py on gfx950 — the k256 GLV split (family G), both ladders (G's corner
and boundary vectors, family X), and the bucket MSM at EVERY window width 4 .. 16 for all twelve parameter sets (family D; k256 on
its GLV halves through the product library and on the plain folded scalar through the tool build with ECGPU_MSM_GLV=0), plus the
top window's sub-bucket spread over every sub-bucket.  tests/test_scalar_vectors.py runs the same vectors through the g++ twin
digit for digit; what only the device has is take()'s v_alignbit, and a wrong digit here is a wrong sum that no error code reports.

Expected values: (sum k_i s_i mod n) G by the oracle's fixed-base multiplication for terms P_i = s_i G, the oracle's MSM for the
sets it sums in well under a second, the oracle's batch_mul for the ladders."""
import random
import time

import numpy as np
import pytest

import oracle_lib
import pyec
import scalar_vectors as sv
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu

ORACLE_MSM_TERMS = 1500            # the oracle's MSM is summed next to the dot product up to this many terms


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


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


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
    print("\nslowest cases of test_gpu_scalar_vectors:")
    for dt, name in sorted(_durations, reverse=True)[:12]:
        print("  %6.2f s  %s" % (dt, name))


def enc(c, ks):
    return np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in ks), np.uint8)


def be32(k):
    return k.to_bytes(32, "big")


# ---- the split ------------------------------------------------------------------------------------------------------------------

def test_device_split_equals_oracle(eng):
    ks = sv.g_all() + sv.family_x("k256")
    sv.check_coverage_g()
    r1, r2 = eng.k256_glv_decompose(enc(pyec.K256, ks))
    r1, r2 = bytes(r1), bytes(r2)
    for i, k in enumerate(ks):
        got = (r1[32 * i: 32 * i + 32], r2[32 * i: 32 * i + 32])
        if got != oracle_lib.k256_glv_decompose(be32(k)):
            s1, s2, c1, c2 = sv.glv_split(k)
            raise AssertionError("vector %d, k = %#x: the device splits into %s, %s, the oracle into %#x, %#x (signed %#x, %#x; rounded "
                                 "quotients %#x, %#x)" % ((i, k, got[0].hex(), got[1].hex(), c1, c2, s1, s2) + sv.glv_quotients(k)))


# ---- the ladders ----------------------------------------------------------------------------------------------------------------

def ladder_scalars(name):
    ks = list(sv.family_x(name))
    if name == "k256":
        g = sv.family_g()
        ks += g["corners"] + g["boundary"]
    return ks


@pytest.mark.parametrize("name", sv.CURVES)
def test_device_ladders_on_radix16_words_and_split_extremes(eng, name):
    """ecgpu_batch_mul, its constant-time form and mul_by_generator_and_mul_add (a = 0: b P alone; a = b on P = G: 2 b G) on family X
    — for k256 also G's corners and rounding boundary — with three random points and G, against the oracle's batch_mul."""
    c = pyec.CURVES[name]
    sv.check_coverage_x(name)
    ks = ladder_scalars(name)
    scal = enc(c, ks)
    n = len(ks)
    zeros = np.zeros(n * c.L, np.uint8)
    rng = np.random.default_rng(0x1ADD + c.cid)
    rp, _ = oracle_lib.batch_mul_base(c.cid, enc(c, [int(rng.integers(2, 2 ** 62)) for _ in range(3)]))
    G = pyec.enc_point(c, pyec.G(c))[0]
    for j, P in enumerate([G] + [bytes(rp[2 * c.L * i: 2 * c.L * (i + 1)]) for i in range(3)]):
        pxy = np.frombuffer(P * n, np.uint8)
        want, winf = oracle_lib.batch_mul(c.cid, scal, pxy, None)
        for what, (out, inf) in (("mul", eng.mul(c.cid, scal, pxy)), ("mul_ct", eng.mul(c.cid, scal, pxy, constant_time=True)),
                                 ("mul_add", eng.mul_by_generator_and_mul_add(c.cid, zeros, scal, pxy))):
            if bytes(out) != bytes(want) or bytes(inf) != bytes(winf):
                o = np.asarray(out).reshape(n, 2 * c.L)
                i = next(i for i in range(n) if bytes(o[i]) != bytes(want[2 * c.L * i: 2 * c.L * (i + 1)]) or inf[i] != winf[i])
                raise AssertionError("%s %s, point %d: first mismatch at vector %d, k = %#x, recoded %s" % (
                    name, what, j, i, ks[i], ["%#x" % v for v, _ in sv.x_recoded(name, ks[i])]))
    out, inf = eng.mul_by_generator_and_mul_add(c.cid, scal, scal, np.frombuffer(G * n, np.uint8))
    want, winf = oracle_lib.batch_mul_base(c.cid, enc(c, [2 * k % c.n for k in ks]))
    assert bytes(out) == bytes(want) and bytes(inf) == bytes(winf)


# ---- the MSM at every width ---------------------------------------------------------------------------------------------------------

SPLITS = [(name, False) for name in sv.CURVES] + [("k256", True)]
MSM_CASES = [(name, glv, cbits) for name, glv in SPLITS for cbits in sv.WIDTHS]
_points = {}


def points_for(eng, name, count):
    """(s, prefix sums of s, P_i = s_i G as an (m, 2 L) array), made once per parameter set by mul_by_generator."""
    c = pyec.CURVES[name]
    if name not in _points:
        rng = random.Random(0x5EED + c.cid)
        m = (1 << 15) + 128 if name == "k256" else (1 << 14) + 128 if scalar_bits(name) == 255 else 3000
        s = [rng.randrange(1, c.n) for _ in range(m)]
        pts, inf = eng.mul_by_generator(c.cid, enc(c, s))
        assert not inf.any()
        want, _ = oracle_lib.batch_mul_base(c.cid, enc(c, s[:64]))
        assert bytes(pts[: 64 * 2 * c.L]) == bytes(want)
        pre = [0]
        for x in s:
            pre.append(pre[-1] + x)
        _points[name] = (s, pre, np.asarray(pts).reshape(m, 2 * c.L).copy())
    s, pre, pts = _points[name]
    assert count <= len(s), (name, count)
    return s, pre, pts


def scalar_bits(name):
    return sv.geometry(name, False)[0]


def engine_for(eng, keng, name, glv, monkeypatch):
    """k256 on the plain folded scalar: the tool build with ECGPU_MSM_GLV=0.  The variable is set after the module's engine was
    made; that works because the tool build's knob() is getenv at every call (ecgpu_knobs.h), and the automatic plans below show
    that it did: at 2^19 terms the planner gives the GLV halves c = 15 and the plain scalar c = 13, at 2^12 terms 10 and 9."""
    if name == "k256" and not glv:
        monkeypatch.setenv("ECGPU_MSM_GLV", "0")
        assert (keng.msm_plan_window(0, 1 << 19), keng.msm_plan_window(0, 1 << 12)) == (13, 9)
        assert (eng.msm_plan_window(0, 1 << 19), eng.msm_plan_window(0, 1 << 12)) == (15, 10)
        return keng
    return eng


def want_dot(c, ks, s, inf):
    total = sum(k * x for k, x, f in zip(ks, s, inf) if not f) % c.n
    w, wf = oracle_lib.batch_mul_base(c.cid, pyec.enc_scalar(c, total))
    return bytes(w), int(wf[0])


def bisect_msm(e, c, name, glv, cbits, ks, s, pts, inf):
    """The MSM over ks differs from the dot product: halve the term list until one term is left (each call is a valid MSM)."""
    lo, hi = 0, len(ks)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        o, f = e.lincomb(c.cid, enc(c, ks[lo:mid]), pts[lo:mid].reshape(-1), inf[lo:mid])
        if (bytes(o), f) != want_dot(c, ks[lo:mid], s[lo:mid], inf[lo:mid]):
            hi = mid
        else:
            lo = mid
    o, f = e.lincomb(c.cid, enc(c, ks[lo:hi]), pts[lo:hi].reshape(-1), inf[lo:hi])
    alone = (bytes(o), f) != want_dot(c, ks[lo:hi], s[lo:hi], inf[lo:hi])
    kbits, _ = sv.geometry(name, glv)
    digs = [sv.msm_digits(sub, kbits, cbits, lo, flip) for sub, flip in sv.subs(name, glv, ks[lo])]
    return "%s %s c = %d: narrowed to term %d (%s on its own), k = %#x, subs %s, model digits (bucket, neg, nonzero) %r" % (
        name, "GLV" if glv else "plain", cbits, lo, "wrong" if alone else "right", ks[lo],
        [("%#x" % sub, flip) for sub, flip in sv.subs(name, glv, ks[lo])], digs)


@pytest.mark.parametrize("name,glv,cbits", MSM_CASES, ids=["%s-%s-%d" % (n, "glv" if g else "plain", cb) for n, g, cb in MSM_CASES])
def test_device_msm_on_digit_strings_at_every_width(eng, keng, name, glv, cbits, monkeypatch):
    """The D set of (set, split, c) as one MSM with the window width forced to c (which also switches the small-MSM path off, so
    these few hundred terms do reach k_msm_prepare), a few flagged identities among the terms; then the same terms with the automatic
    plan (below 2^16 terms: one multiplication per term and a tree sum)."""
    c = pyec.CURVES[name]
    e = engine_for(eng, keng, name, glv, monkeypatch)
    ks = sv.family_d(name, glv, cbits)
    sv.check_coverage_d(name, glv, cbits, ks)
    n = len(ks)
    s, _, pts = points_for(eng, name, n)
    s, pts = s[:n], pts[:n].copy()
    inf = np.zeros(n, np.uint8)
    for i in (3, 64, n - 1):
        inf[i] = 1
        pts[i] = 0
    want = want_dot(c, ks, s, inf)
    scal = enc(c, ks)
    try:
        e.set_msm_window(cbits)
        assert e.msm_plan_window(c.cid, n) == cbits
        o, f = e.lincomb(c.cid, scal, pts.reshape(-1), inf)
        if (bytes(o), f) != want:
            raise AssertionError(bisect_msm(e, c, name, glv, cbits, ks, s, pts, inf))
    finally:
        e.set_msm_window(0)
    if n <= ORACLE_MSM_TERMS:
        w, wf = oracle_lib.msm(c.cid, scal, pts.reshape(-1), inf, vartime=True)
        assert (bytes(w), wf) == want
    o, f = e.lincomb(c.cid, scal, pts.reshape(-1), inf)
    assert (bytes(o), f) == want, (name, glv, cbits, "automatic plan")


def _spread_cases():
    out = []
    for name, glv in SPLITS:
        kbits, value_bits = sv.geometry(name, glv)
        if not glv and value_bits < kbits:
            continue                                  # p521: no canonical scalar reaches the top window (asserted in check_coverage_d)
        out += [(name, glv, cbits) for cbits in sv.WIDTHS if sv.top_shift(kbits, cbits) > 0]
    return out


SPREAD_CASES = _spread_cases()


def spread_scalars(name, glv, cbits):
    """The distinct scalars among: k with top digit 1, k with the largest top digit the D set holds (2^rem on the plain split), by
    the model.  In GLV mode the second is taken, where the set has one, from the half that the first does not use, so that the
    spread runs over i and over npad + i; should only one half of the set reach its top window, both come from that half, and
    should they coincide, one scalar remains."""
    kbits, _ = sv.geometry(name, glv)
    best = {}                                        # (half, top digit) -> first k that has it
    for k in sv.family_d(name, glv, cbits):
        for h, (sub, _) in enumerate(sv.subs(name, glv, k)):
            d = sv.signed_digits(sub, kbits, cbits)[-1]
            if d:
                best.setdefault((h, d), k)
    ones = [h for h in (0, 1) if (h, 1) in best]
    assert ones, (name, glv, cbits)
    h1 = ones[0]
    other = [key for key in best if key[0] != h1] or list(best)
    top = max(d for _, d in other)
    h2 = min(h for h, d in other if d == top)
    if not glv:
        assert top == 1 << (kbits % cbits)
    return list(dict.fromkeys([best[(h1, 1)], best[(h2, top)]]))


@pytest.mark.parametrize("name,glv,cbits", SPREAD_CASES, ids=["%s-%s-%d" % (n, "glv" if g else "plain", cb) for n, g, cb in SPREAD_CASES])
def test_device_top_window_sub_buckets(eng, keng, name, glv, cbits, monkeypatch):
    """One scalar with a non-zero top digit tiled over 2^shift + 65 consecutive terms of distinct points — every sub-bucket
    ((d - 1) << shift) | (index mod 2^shift) of the top window is used, the first 65 twice — starting at term 0 and behind 63 filler
    terms (in GLV mode the second half sits at npad + i, another alignment again).  Against the exact dot product."""
    c = pyec.CURVES[name]
    e = engine_for(eng, keng, name, glv, monkeypatch)
    kbits, _ = sv.geometry(name, glv)
    m = (1 << sv.top_shift(kbits, cbits)) + 65
    s, pre, pts = points_for(eng, name, m + 63)
    filler = sv.family_d(name, glv, cbits)[-63:]
    try:
        e.set_msm_window(cbits)
        for k in spread_scalars(name, glv, cbits):
            for lead in (0, 63):
                ks = filler[:lead] + [k] * m
                n = lead + m
                assert e.msm_plan_window(c.cid, n) == cbits
                total = (sum(a * b for a, b in zip(filler[:lead], s)) + k * (pre[n] - pre[lead])) % c.n
                w, wf = oracle_lib.batch_mul_base(c.cid, pyec.enc_scalar(c, total))
                o, f = e.lincomb(c.cid, enc(c, ks), pts[:n].reshape(-1))
                assert (bytes(o), f) == (bytes(w), int(wf[0])), (name, glv, cbits, hex(k), lead)
    finally:
        e.set_msm_window(0)
