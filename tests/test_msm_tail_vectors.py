"""The vectors of tests/msm_tail_vectors.py against their models, no GPU: the row-field families make every named event of
tools/rows_field_model.py happen (and stop doing so when a family is taken away), the model's limbs are the integers mod p, and
the Horner-chain builder plants its events where it says — by scalar_vectors' digit model — with the dot product, by pyec.mul term
by term and by the oracle's MSM, as the expected result.  tests/test_gpu_msm_tail.py runs the same vectors on gfx950."""
import os

import numpy as np
import pytest

import msm_tail_vectors as mt
import oracle_lib
import pyec
import scalar_vectors as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_SETS = [("k256", True), ("k256", False), ("p256", False), ("p384", False), ("p521", False), ("bp256", False)]


def test_row_vectors_make_every_event_happen_and_the_record_is_current():
    top = mt.check_coverage_rows()
    assert top["th"] == 7 and top["out"] < mt.LB
    with open(os.path.join(ROOT, "profiles", "msm_tail", "coverage.txt")) as f:
        assert f.read() == mt.coverage_report(top)


@pytest.mark.parametrize("family,what", [("th = ", "th"), ("carry pattern", "out29"), ("b8 alone", "fold2")])
def test_coverage_fails_without_a_family(family, what):
    """Take one family away: the check that names what it was there for fails."""
    vec = mt.row_mul_vectors()
    if family == "th = ":
        rest = [v for v in vec if "th = " not in v[0] and "all max" not in v[0] and "climb" not in v[0] and "a8 b8" not in v[0]]
    elif family == "carry pattern":
        rest = [v for v in vec if "carry pattern" not in v[0] and "climb" not in v[0]]
    else:
        rest = [v for v in vec if v[3][8] == 0 or v[4][8] == 0]
    assert len(rest) < len(vec)
    with pytest.raises(AssertionError):
        mt.check_coverage_rows(rest)


def test_row_vectors_stay_inside_the_contract_and_equal_the_integers():
    for label, ma, mb, a, b in mt.row_mul_vectors():
        got = mt.row_mul_expected(a, b)
        assert max(got) < mt.LB and mt.value(got) % mt.P == mt.value(a) * mt.value(b) % mt.P, label
    for label, v in mt.norm64_vectors():
        assert max(v) < 1 << 38
        got = mt.norm64_expected(v)
        assert max(got) < 2 * mt.LB and mt.value(got) % mt.P == mt.value(v) % mt.P, label
    assert any(v[8] >> 29 == 511 and (v[7] & mt.M29) + (v[7] >> 29) > mt.M29 for _, v in mt.norm64_vectors())
    for label, X, Y, Z in mt.dbl_vectors():
        assert max(X) < 2 * mt.LB and max(Y) < 2 * mt.LB and max(Z) < mt.LB
        for steps in (1, 16):
            (x, y, z), want = mt.dbl_expected(X, Y, Z, steps)
            assert (mt.value(x) % mt.P, mt.value(y) % mt.P, mt.value(z) % mt.P) == want, (label, steps)
            assert max(x) < mt.LB and max(z) < mt.LB and max(y) < 2 * mt.LB
            if mt.value(Z) % mt.P == 0:
                assert want[2] == 0 and (want[0] == 0 or mt.value(X) % mt.P != 0), "the identity stays the identity"
    labels = " ".join(l for l, *_ in mt.dbl_vectors())
    assert all(s in labels for s in ("limits", "identity", "Z = 1", "[p, 2p)", "random"))


def test_quad_pairs_hold_every_edge():
    c = pyec.K256
    pairs = mt.quad_pairs("k256")
    kinds = set()
    for a, b in pairs:
        kinds.add("O+O" if a is b is pyec.INF else "O+P" if a is pyec.INF else "P+O" if b is pyec.INF else "P+P" if a == b
                  else "P-P" if a == pyec.neg(c, b) else "generic")
    assert kinds == {"O+O", "O+P", "P+O", "P+P", "P-P", "generic"}
    kinds = set()
    for p, q, want in mt.quad_pairs_generic("k256"):
        x, y = pyec.add(c, p, q), pyec.add(c, q, q)
        assert pyec.add(c, x, y) == want
        kinds.add("X=O" if x is pyec.INF else "X=Y" if x == y else "X=-Y" if x == pyec.neg(c, y) else "generic")
    assert kinds == {"X=O", "X=Y", "X=-Y", "generic"}


def true_dot(case):
    c = pyec.CURVES[case.name]
    acc = pyec.INF
    for k, p, f in zip(case.ks, case.points, case.inf):
        if not f:
            acc = pyec.add(c, acc, pyec.mul(c, k, p))
    return acc


@pytest.mark.parametrize("name,glv", CHAIN_SETS, ids=["%s-%s" % (n, "glv" if g else "plain") for n, g in CHAIN_SETS])
def test_chain_events_happen_where_planted(name, glv):
    """Every event kind at a sample of windows for c = 13 (and c = 4, 16 for k256): the digit model shows the event at its window
    and nowhere else; one case per kind also against pyec.mul term by term and the oracle's MSM."""
    c = pyec.CURVES[name]
    oracle_lib.build()
    lam_g = pyec.mul(pyec.K256, sv.LAMBDA, pyec.G(pyec.K256))
    assert lam_g == (pyec.K256_BETA * pyec.G(pyec.K256)[0] % pyec.K256.p, pyec.G(pyec.K256)[1])
    for cbits in (13, 4, 16) if name == "k256" else (13,):
        for kind in mt.EVENTS:
            cases = mt.cases_for(name, glv, cbits, kind, mt.event_windows(name, glv, cbits, sample=True))
            assert cases, (name, glv, cbits, kind)
            for case in cases:
                classes = mt.check_coverage_chain(case)
                if kind in ("cancel", "equal", "flip"):
                    assert classes.count(kind) == 1
                if kind == "cancel3":
                    assert classes.count("cancel") == 1 and classes.count("idle") >= 2
                assert all(p is pyec.INF or pyec.on_curve(c, p) for p in case.points)
            case = cases[0]
            want = pyec.mul(c, case.want_log, pyec.G(c)) if case.want_log else pyec.INF
            if cbits == 13:
                if kind in ("cancel", "flip", "empty_mid"):
                    assert true_dot(case) == want, (name, glv, cbits, kind)
                scal = np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in case.ks), np.uint8)
                pxy = np.frombuffer(b"".join(pyec.enc_point(c, p)[0] for p in case.points), np.uint8)
                w, wf = oracle_lib.msm(c.cid, scal, pxy, np.array(case.inf, np.uint8), vartime=True)
                assert pyec.dec_point(c, bytes(w), int(wf)) == want


def test_chain_check_fails_when_the_fixup_term_goes():
    case = mt.build_chain("p256", False, 5, [("cancel", 30)])
    assert mt.layout("p256", False, 5)[2] == 52
    mt.check_coverage_chain(case)
    case.ks[-1] = 1 << (5 * 29)                                  # the fix-up digit one window too low
    case.want_log = sum(k * s for k, s, f in zip(case.ks, case.ss, case.inf) if not f) % pyec.P256.n
    with pytest.raises(AssertionError):
        mt.check_coverage_chain(case)


def test_two_rank_and_bucket_terms():
    for name, glv in (("k256", True), ("p256", False)):
        c = pyec.CURVES[name]
        a, b, want = mt.two_rank_terms(name, glv, 13)
        assert want == 0 and (a.want_log + b.want_log) % c.n == 0 and a.want_log != 0
        la = [mt.term_logs(name, glv, 13, k, s)[0] for k, s, f in zip(a.ks, a.ss, a.inf) if not f]
        assert all(sum(col) % c.n != 0 for col in list(zip(*la))[: mt.layout(name, glv, 13)[3]])     # non-identity parts per window
        a, b, want = mt.two_rank_terms(name, glv, 13, leave=3)
        assert want != 0 and (a.want_log + b.want_log) % c.n == want
        for cbits in (9, 13):
            cases = mt.bucket_cases(name, glv, cbits)
            assert len(cases) >= 6
            kbits = sv.geometry(name, glv)[0]
            for label, ks, ss in cases:
                d0, d1 = (sv.signed_digits(sv.subs(name, glv, k)[0][0], kbits, cbits) for k in ks[:2])
                w = [i for i, d in enumerate(d0) if d]
                assert len(w) == 1 and d1[w[0]] == d0[w[0]] + 1 and sum(1 for d in d1 if d) == 1, label
