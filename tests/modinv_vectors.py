"""Adversarial inputs for the division-step inversion of csrc/ecgpu_modinv.h, shared by tests/test_modinv_vectors.py (the model and
the g++ twin) and tests/test_gpu_modinv_vectors.py (gfx950).  Plain module: deterministic, seeded per curve id; both moduli, p and
n, of all twelve parameter sets.  Every vector is THE INTEGER THAT REACHES ModInv::invert (for a Montgomery field that is a R mod p
of the canonical operand a: `canonical_operand` turns a vector into what ops 4 and 17 take); every expected value is a Python integer.

  L  the 30-bit layout: field_vectors.structured on the inversion's own limbs (30 bits, NL of them); values whose low 1 .. NL - 1
     limbs are zero (whole batches of thirty zero steps, u = 2^30) as integers t 2^(30 k) and as products t 2^(30 k) mod m; 2^k and
     m - 2^k for every k; (m +- 1) / 2, m - 1, m - 2, 1 .. 64; low limbs equal to +-(the low limb of m) and low limbs with 1 .. 29
     trailing zeros.
  T  results steered: x = t^-1 mod m for every structured t, so that normalize and to_words produce every structured output.
  S  search-steered constants (tests/modinv_search_constants.py, written by tools/modinv_search.py, which reproduces them): inputs
     that push the traces of tools/modinv_model.py to the most batches until g = 0 in both forms, d or e nearest -2p and nearest p,
     the largest |md| and the largest accumulator, each sign combination entering normalize, d < -p with f of either sign, and every
     `limit` 1 .. 6 and the swap branch of divsteps_30_var in the first, a middle and the last working batch.

check_coverage recomputes family S's traces with the model: every recorded threshold is met, and is at least what RANDOM_COUNT
seeded random inputs reach for that modulus (measured by the model, there and then).  What it does NOT promise is the proven step
bound (590 steps for 256 bits): with f = p the random inputs stay below 531 steps and a bit-flip climb gains a handful; the last
batches of `invert` only ever run on g = 0, which the tests therefore exercise as such (a lane that is done early keeps its value).
Nothing is dropped by try / skip: a vector the big-integer reference cannot evaluate is a bug here."""
import os
import random
import sys

import numpy as np

import pyec
from field_vectors import CURVES, layout, structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import modinv_model as mm                                                     # noqa: E402

WHICH = ("p", "n")
MODULI = [(name, which) for name in CURVES for which in WHICH]
RANDOM_COUNT = 20000

# the extremes family S aims at: name -> (form, the figure of a Trace, per lane, larger = more extreme)
S_EXTREMES = {
    "batches": ("ct", lambda tr: tr.batches.astype(float)),
    "batches_var": ("var", lambda tr: tr.batches + tr.steps / 4096.0),
    "low": ("ct", lambda tr: -np.minimum(tr.dmin, tr.emin)),                  # d or e nearest -2p
    "high": ("ct", lambda tr: np.maximum(tr.dmax, tr.emax)),                  # d or e nearest p
    "md": ("ct", lambda tr: tr.md.astype(float)),
    "acc": ("ct", lambda tr: tr.acc.astype(float)),
}
# the states family S must show: name -> (form, predicate on a Trace, per lane)
# The signs entering normalize are those of the VARIABLE form, which normalises right after the batch that brought g to 0.  In the
# branch-free form every input runs at least one further batch on g = 0 (u = 2^30), and such a batch brings a negative d into
# [0, p): there d >= 0 always enters normalize (asserted in tests/test_modinv_vectors.py on every vector).
S_STATES = {
    "d+f+": ("var", lambda tr: ~tr.dneg & ~tr.fneg),
    "d+f-": ("var", lambda tr: ~tr.dneg & tr.fneg),
    "d-f+": ("var", lambda tr: tr.dneg & ~tr.fneg),
    "d-f-": ("var", lambda tr: tr.dneg & tr.fneg),
    "dlow f+": ("var", lambda tr: tr.dlow & ~tr.fneg),
    "dlow f-": ("var", lambda tr: tr.dlow & tr.fneg),
}


def batch_at(tr, where):
    """index of the first / a middle / the last working batch of every lane (lanes with no working batch: 0)"""
    last = np.maximum(tr.batches - 1, 0)
    return {"first": np.zeros_like(last), "middle": last // 2, "last": last}[where]


def _limit_state(where, k):
    def f(tr):
        b = batch_at(tr, where)
        return (tr.batches > 0) & (((tr.limits_batch[b, np.arange(len(b))] >> k) & 1) == 1)
    return f


def _swap_state(where):
    def f(tr):
        b = batch_at(tr, where)
        return (tr.batches > 0) & tr.swaps[b, np.arange(len(b))]
    return f


for _w in ("first", "middle", "last"):
    for _k in range(1, 7):
        S_STATES["limit %d %s" % (_k, _w)] = ("var", _limit_state(_w, _k))
    S_STATES["swap %s" % _w] = ("var", _swap_state(_w))


def modulus(name, which):
    c = pyec.CURVES[name]
    return c.p if which == "p" else c.n


def nw(name):
    return (8 * pyec.CURVES[name].L + 31) // 32


def seed(name, which, salt):
    return salt * 64 + 2 * pyec.CURVES[name].cid + WHICH.index(which)


def mont_r(name):
    """R of the field's Montgomery form (1 for k256)"""
    lay = layout(name)
    return (1 << (lay.nl * lay.b)) if lay.mont else 1


def canonical_operand(name, v):
    """the canonical a for which F::inv(from_canonical(a)) hands v to ModInv::invert"""
    p = pyec.CURVES[name].p
    return v * pow(mont_r(name), -1, p) % p


def want_field_inv(name, v):
    """ops 4 and 17 on canonical_operand(name, v)"""
    p = pyec.CURVES[name].p
    a = canonical_operand(name, v)
    return pow(a, -1, p) if a else 0


def want_raw_inv(name, w):
    """ops 46 and 47 on the raw operand w (it may exceed p): pack(F::inv(unpack(w))).  F::inv inverts the packed integer (pack
    reduces w in [p, 2p) first: ModInv::invert wants x < p, and by the model invert(p) would be 1, not 0), unpacks
    the result r — as an internal-domain value that is r R^-1 — and multiplies twice by R^2: r R^-1 R^2 R^2 R^-2 = r R^2."""
    p = pyec.CURVES[name].p
    r = mont_r(name)
    return pow(w, -1, p) * r * r % p if w % p else 0


def raw_lim(name):
    c = pyec.CURVES[name]
    return min(2 * c.p, 1 << (8 * c.L)) if layout(name).mont else 1 << 256


# ---- families L and T -------------------------------------------------------------------------------------------------------------

def structured30(name, which):
    m = modulus(name, which)
    return structured(30, mm.NLIMBS[nw(name)], pyec.CURVES[name].L, m, m)


def family_l(name, which):
    m = modulus(name, which)
    nl = mm.NLIMBS[nw(name)]
    rng = random.Random(seed(name, which, 0x30))
    out = set(structured30(name, which))
    bits = m.bit_length()
    small = [1, 2, 3, 5, (1 << 30) - 1, (1 << 29) + 1]
    for k in range(1, nl):                                        # low k limbs zero
        room = m >> (30 * k)
        if room < 2:                                              # (p521: 19 limbs hold 570 bits, the top limb of m is zero)
            assert name == "p521" and k == nl - 1
            continue
        ts = [t for t in small if t < room] + [rng.randrange(1, room) for _ in range(3)] + [rng.randrange(1, room) | 1, room - 1]
        for t in ts:
            assert (t << (30 * k)) < m
            out.add(t << (30 * k))
            out.add((t << (30 * k)) % m)
        for t in small + [rng.randrange(1, m) for _ in range(2)]:
            out.add(t * (1 << (30 * k)) % m)                      # ... and as a product mod m
            out.add(t * pow(1 << (30 * k), -1, m) % m)
    for k in range(bits):
        if (1 << k) < m:
            out.add(1 << k)
            out.add(m - (1 << k))
    out |= {(m + 1) // 2, (m - 1) // 2, m - 1, m - 2} | set(range(1, 65))
    p0 = m & mm.M30
    for _ in range(6):
        hi = rng.randrange(m >> 30) << 30
        out |= {hi | p0, hi | ((1 << 30) - p0), p0, (1 << 30) - p0}
    for tz in range(1, 30):
        for _ in range(2):
            hi = rng.randrange(m >> 30) << 30
            out.add(hi | (((rng.randrange(1 << (30 - tz)) | 1) << tz) & mm.M30))
    out = sorted(v for v in out if 0 <= v < m)
    return out


def family_t(name, which):
    m = modulus(name, which)
    return sorted({pow(t, -1, m) for t in structured30(name, which) if t % m})


# ---- family S ---------------------------------------------------------------------------------------------------------------------

def s_constants(name, which):
    """{goal: (input, threshold or None)} as tools/modinv_search.py wrote them"""
    import modinv_search_constants as sc
    return sc.FAMILY_S[name][which]


def family_s(name, which):
    return sorted({x for x, _ in s_constants(name, which).values()})


def random_inputs(name, which, count=RANDOM_COUNT):
    rng = random.Random(seed(name, which, 0xBA5E))
    m = modulus(name, which)
    return [rng.randrange(m) for _ in range(count)]


def traces(name, which, xs, check_result=False):
    """{form: Trace} of the model on xs (the variable form lane by lane: wave = 1).  The extremes are all figures of the
    branch-free form; of the variable form only counts and states are read, so a run without expected values leaves its
    interval assertions to tests/test_modinv_vectors.py, which makes them on every vector."""
    m = modulus(name, which)
    _, ct, _ = mm.invert(xs, m, nw(name), check_result=check_result)
    _, var = mm.invert_var(xs, m, nw(name), wave=1, check=check_result, check_result=check_result)
    return {"ct": ct, "var": var}


def random_baseline(name, which, count=RANDOM_COUNT):
    """{extreme: the largest figure among `count` seeded random inputs}, by the model"""
    tr = traces(name, which, random_inputs(name, which, count))
    return {goal: float(fig(tr[form]).max()) for goal, (form, fig) in S_EXTREMES.items()}


def check_coverage(name, which, baseline=None):
    """Family S does what it is there for: every extreme reaches its recorded threshold, every threshold is at least the random
    baseline, every state is shown by the input recorded for it."""
    consts = s_constants(name, which)
    assert set(consts) == set(S_EXTREMES) | set(S_STATES), sorted(set(consts) ^ (set(S_EXTREMES) | set(S_STATES)))
    goals = sorted(consts)
    xs = [consts[g][0] for g in goals]
    tr = traces(name, which, xs, check_result=True)
    if baseline is None:
        baseline = random_baseline(name, which)
    for j, g in enumerate(goals):
        x, threshold = consts[g]
        if g in S_EXTREMES:
            form, fig = S_EXTREMES[g]
            got = float(fig(tr[form])[j])
            assert got >= threshold, "%s %s, %s: the recorded input reaches %r, recorded %r" % (name, which, g, got, threshold)
            assert threshold >= baseline[g], "%s %s, %s: %d random inputs reach %r, the search only %r" % (
                name, which, g, RANDOM_COUNT, baseline[g], threshold)
        else:
            form, pred = S_STATES[g]
            assert threshold is None and bool(pred(tr[form])[j]), "%s %s: %#x does not show the state '%s'" % (name, which, x, g)


# ---- what the tests share ---------------------------------------------------------------------------------------------------------

def all_vectors(name, which):
    """families L, T and S, in this order, distinct"""
    return list(dict.fromkeys(family_l(name, which) + family_t(name, which) + family_s(name, which)))


def enc(c, vals):
    return b"".join(v.to_bytes(c.L, c.order) for v in vals)


def dec(c, data):
    data = bytes(data)
    return [int.from_bytes(data[i: i + c.L], c.order) for i in range(0, len(data), c.L)]


def first_mismatch(name, what, xs, got, want):
    """None, or a message with the first differing index, the vector that reached the inversion and both values."""
    assert len(got) == len(want) == len(xs), (name, what, len(got), len(want), len(xs))
    if got == want:
        return None
    i = next(k for k in range(len(want)) if got[k] != want[k])
    bad = sum(1 for g, w in zip(got, want) if g != w)
    return "%s %s: %d of %d differ, first at %d: the inversion receives %#x, got %#x, want %#x" % (name, what, bad, len(want), i, xs[i], got[i], want[i])
