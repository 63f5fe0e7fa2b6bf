"""The comb vectors of tests/comb_vectors.py checked without a GPU: the recoding model reconstructs every scalar, every emitted
vector decodes to what its record says, the sample keeps its minimum contents — and the g++ twin of the lane body
(tests/hostcheck, the same fixed_base_mul the device runs) returns the table entry, bit for bit against the big-integer model, for
every reachable entry at w = 4, 5, 8 and for the structured sample at w = 13 and 16."""
import random

import numpy as np
import pytest

import comb_vectors as cv
import hostcheck_lib as hc
import pyec
from gpu_common import comb_corner_scalars, edge_scalars

ALL_WIDTHS = (4, 5, 8, 15, 16, 17, 20, 22, 24, 26)


def test_geometry_read_from_the_sources():
    for name in cv.CURVES:
        c = pyec.CURVES[name]
        ws = cv.WIDTHS[name]
        assert ws[0] == 16 and ws[-1] == cv.widest(c) and set(ws) <= {16, 22, cv.widest(c)} and list(ws) == sorted(set(ws))
        assert set(ws) == {cv.table_tier(s, cv.widest(c)) for s in (1, cv.tier_thresholds()[0], cv.tier_thresholds()[1])}
        assert cv.ct_base_luts(c) * 6 > c.n.bit_length() >= (cv.ct_base_luts(c) - 1) * 6
        for w in ALL_WIDTHS:
            assert 1 <= cv.slab_windows(c, w) <= cv.window_count(c, w)
            assert cv.entry_lanes(w) * 64 >= 1 << (w - 1) or cv.entry_lanes(w) == 1 << 17
    assert cv.table_tier((1 << 26) - 1, 26) < cv.table_tier(1 << 26, 26) < cv.table_tier(1 << 29, 26)


@pytest.mark.parametrize("curve", cv.CURVES)
def test_recode_reconstructs_every_scalar(curve):
    """sum d_j 2^(w j) = +-k (mod n) with every digit in (-2^(w-1), 2^(w-1)], for the comb's corner scalars, the edge scalars and
    random ones at all ten widths; the module's own vectors decode to their records (sample_vectors asserts it for each) and the
    sample keeps its minimum contents.  On the 256-bit sets the digits are also those of signed_window_step / get_bits as the g++
    twin compiles them (hc_signed_windows: 256-bit scalars, no fold, one window more where w divides 256)."""
    c = pyec.CURVES[curve]
    rng = random.Random(0x2EC0DE + c.cid)
    for w in ALL_WIDTHS:
        half = 1 << (w - 1)
        cv.check_sample_coverage(c, w)
        vecs = cv.sample_vectors(c, w)
        assert {v.form for v in vecs} == {"pos", "neg", "nk"}
        # every sampled entry is aimed at by a single-digit scalar
        aimed = {(v.j, v.e) for v in vecs if v.form == "pos"}
        assert aimed == {(j, e) for j, es in cv.entry_sample(c, w).items() for e in es}
        assert all(v.digits == {v.j: v.e} and not v.flip for v in vecs if v.form == "pos")
        own = [v.k for v in vecs[::11]]
        for k in comb_corner_scalars(c, w) + edge_scalars(c) + [rng.randrange(c.n) for _ in range(300)] + own:
            flip, digits = cv.recode(c, w, k)
            assert len(digits) == cv.window_count(c, w) and all(-half < d <= half for d in digits), (curve, w, hex(k))
            assert cv.decode(c, w, flip, digits) == k, (curve, w, hex(k))
            if c.L == 32:
                folded = c.n - k if flip else k
                got = hc.signed_windows(folded.to_bytes(32, "big"), w)
                assert got is not None and len(got) in (len(digits), len(digits) + 1), (curve, w, hex(k))
                assert [int(d) for d in got[: len(digits)]] == digits and not got[len(digits):].any(), (curve, w, hex(k))


def test_ct_lut_scalars_select_every_entry():
    for name in cv.CURVES:
        c = pyec.CURVES[name]
        ks = cv.ct_lut_scalars(c)
        assert all(0 < k < c.n for k in ks)
        pos = set(ks[0::2])
        nl = cv.ct_base_luts(c)
        full = {e << (6 * i) for i in range(nl - 1) for e in range(1, 33)}
        assert full <= pos and len(ks) >= 2 * 32 * (nl - 1)
        assert all(ks[i] + ks[i + 1] == c.n for i in range(0, len(ks), 2))
        # the top LUT is reached: by a digit of its own, or (order of 6 i bits: its only entry in use is 1) by the carry of e = 32
        assert any(k >> (6 * (nl - 1) - 1) for k in pos)


# ---- the twin against the big-integer model --------------------------------------------------------------------------------------

def _dbl(c, P, times):
    for _ in range(times):
        P = pyec.add(c, P, P)
    return P


def _multiples(c, P, count):
    """[O, P, 2P, .., (count-1) P]"""
    out = [pyec.INF, P]
    for _ in range(count - 2):
        out.append(pyec.add(c, out[-1], P))
    return out[:count]


def expected_points(c, w, vecs):
    """The big-integer model's k G for vectors of comb_vectors, from the ENTRY each one names: e 2^(w j) G by two table lookups and
    one addition, the signed forms from it (2^(w (j+1)) G - entry, - entry)."""
    nwin = cv.window_count(c, w)
    bases = [pyec.G(c)]
    for _ in range(nwin):
        bases.append(_dbl(c, bases[-1], w))
    s = (w + 1) // 2
    out = []
    tabs = {}
    for v in vecs:
        if v.j not in tabs:
            tabs.clear()                                                  # vectors come window by window
            tabs[v.j] = (_multiples(c, bases[v.j], 1 << s), _multiples(c, _dbl(c, bases[v.j], s), (1 << (w - 1 - s)) + 2))
        lo, hi = tabs[v.j]
        P = pyec.add(c, lo[v.e & ((1 << s) - 1)], hi[v.e >> s])
        if v.form == "neg":
            P = pyec.add(c, bases[v.j + 1], pyec.neg(c, P))
        elif v.form == "nk":
            P = pyec.neg(c, P)
        out.append(P)
    return out


def _twin_against_model(c, w, vecs):
    want = expected_points(c, w, vecs)
    rc, out, inf = hc.batch_mul_base(c.cid, w, cv.enc(c, [v.k for v in vecs]), 5)
    assert rc == 0
    assert not inf.any()
    got = np.asarray(out).reshape(len(vecs), 2 * c.L)
    exp = np.frombuffer(b"".join(pyec.enc_point(c, P)[0] for P in want), np.uint8).reshape(len(vecs), 2 * c.L)
    bad = np.flatnonzero((got != exp).any(axis=1))
    if bad.size:
        v = vecs[int(bad[0])]
        pytest.fail("%s w = %d: %d of %d differ, first: window %d, entry %d, form %s, k = %#x" % (
            c.name, w, bad.size, len(vecs), v.j, v.e, v.form, v.k))


def test_expected_points_model():
    """The shortcut above is the plain double-and-add of the model (a sample of the vectors, both ways)."""
    c = pyec.CURVES["p224"]
    vecs = cv.sample_vectors(c, 8, cv.all_entries(c, 8))[::97]
    for v, P in zip(vecs, expected_points(c, 8, vecs)):
        assert P == pyec.mul(c, v.k, pyec.G(c)), v


@pytest.mark.parametrize("w", [4, 5, 8])
@pytest.mark.parametrize("curve", ["k256", "p256", "p384", "p224", "bp256", "p521"])
def test_twin_returns_every_reachable_entry(curve, w):
    c = pyec.CURVES[curve]
    entries = cv.all_entries(c, w)
    R = cv.reachable(c, w)
    assert sum(len(r) for r in entries.values()) == sum(R) and R[0] == 1 << (w - 1)
    _twin_against_model(c, w, cv.sample_vectors(c, w, entries))


@pytest.mark.parametrize("w", [13, 16])
@pytest.mark.parametrize("curve", ["k256", "p256"])
def test_twin_on_the_entry_sample(curve, w):
    c = pyec.CURVES[curve]
    _twin_against_model(c, w, cv.sample_vectors(c, w))
