"""Adversarial inputs for the part of the MSM behind the buckets — the k256 field on rows of 16 lanes (csrc/ecgpu_rows.h), the
complete addition on quad lanes, the quad tree, the lane-shared Jacobian doubling and k_msm_combine's Horner chain (csrc/ecgpu_msm.h)
— shared by tests/test_msm_tail_vectors.py (the models, no GPU) and tests/test_gpu_msm_tail.py (gfx950: ops 20 - 26 of
ecgpu_selftest_point, csrc/ecgpu_selftest_msm.h, and whole MSMs).  Plain module: deterministic, seeded; every expected value comes
from tools/rows_field_model.py (limbs), Python's integers (values) or tests/pyec.py (points).

Row field (raw limbs, nothing between the vector and RowsK256::mul):
  at every magnitude pair of MAG_PAIRS — all limbs at m LB - 1; one limb of a at its maximum against one limb of b at its maximum,
  all 81 position pairs; limb 8 alone on both sides with the top column's third piece th = 1 .. ma mb; all limbs at 2^29 - 1;
  products steered to 0, 1, p - 1, 2^256 - 1 mod p; the carry patterns b = .., 2^29, 2^30 - 1, 2^29 - 2, .. under a = 1 that leave an
  output limb at 2^29 or above; operands a seeded climb over the model drives to the largest stage-2 value, stage-3 carry and output
  limb.  check_coverage_rows asserts through the model's events that all of it happens.
Horner chain: build_chain(name, glv, cbits, events) -> a Case whose MSM makes the accumulator of k_msm_combine cancel, meet an equal
  point, change sign, cross runs of empty windows, at windows of the caller's choice.  All points are known multiples of G, so the
  chain is walked on discrete logarithms mod n (the groups have prime order: the identity is the logarithm 0); the digits come from
  scalar_vectors' model of the recoding applied to the finished scalars, and the expected result is (sum k_i s_i) G, which knows
  nothing of windows.  check_coverage_chain asserts every planted event at its window and none elsewhere."""
import functools
import os
import random
import sys

import pyec
import scalar_vectors as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import rows_field_model as rm                                                 # noqa: E402

P = rm.P
LB = rm.LB
M29 = rm.M
K256 = pyec.CURVES["k256"]
# (ma, mb) with ma mb <= 7: the limit of RowsK256::mul's contract, and what RowsDblK256::step forms ((2, 2), (2, 1), (1, 1) on
# level 1, (2, 2) on level 2)
MAG_PAIRS = ((1, 1), (2, 2), (2, 1), (1, 7), (7, 1), (2, 3), (3, 2))
STEP_PAIRS = ((2, 2), (2, 1), (1, 1))


def limbs9(v):
    """v < 2^(29 * 8 + 32) as nine limbs: eight of 29 bits and the rest"""
    out = [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]
    assert out[8] < 1 << 32
    return out


def value(limbs):
    return sum(x << (29 * i) for i, x in enumerate(limbs))


# ---- row multiplication -------------------------------------------------------------------------------------------------------

def _climb(rng, ma, mb, objective, start, rounds=900):
    """Seeded hill climb over the model: add or subtract a power of two in one limb, keep what raises the objective."""
    a, b = list(start[0]), list(start[1])

    def score(a, b):
        ev = {}
        rm.mul_rows(rm.row(a), rm.row(b), None, ev)
        return objective(ev)
    best = score(a, b)
    for _ in range(rounds):
        side, i, k, sign = rng.randrange(2), rng.randrange(9), rng.randrange(32), rng.choice((1, -1))
        v = (a if side == 0 else b)[i] + sign * (1 << k)
        lim = (ma if side == 0 else mb) * LB
        v = min(max(v, 0), lim - 1)
        na, nb = list(a), list(b)
        (na if side == 0 else nb)[i] = v
        s = score(na, nb)
        if s > best:
            a, b, best = na, nb, s
    return a, b


@functools.lru_cache(maxsize=None)
def row_mul_vectors():
    """[(label, ma, mb, a limbs, b limbs)]"""
    out = []
    rng = random.Random(0x7A11)
    for ma, mb in MAG_PAIRS:
        ta, tb = ma * LB - 1, mb * LB - 1
        tag = "%dx%d " % (ma, mb)
        out.append((tag + "all max", ma, mb, [ta] * 9, [tb] * 9))
        for i in range(9):
            for j in range(9):
                out.append((tag + "a%d b%d alone" % (i, j), ma, mb, [ta if t == i else 0 for t in range(9)], [tb if t == j else 0 for t in range(9)]))
        for th in range(1, ma * mb + 1):                       # limb 8 alone: the top column a_8 b_8 with its third piece equal to th
            b8 = -(-(th << 58) // ta)
            assert b8 <= tb and (ta * b8) >> 58 == th
            out.append((tag + "th = %d" % th, ma, mb, [0] * 8 + [ta], [0] * 8 + [b8]))
            out.append((tag + "th = %d under all max" % th, ma, mb, [ta] * 9, [tb] * 8 + [b8]))
        out.append((tag + "all 2^29 - 1", ma, mb, [M29] * 9, [M29] * 9))
        for target in (0, 1, P - 1, (2 ** 256 - 1) % P):
            x = rng.randrange(1, P)
            y = target * pow(x, -1, P) % P
            if mb > 1:
                y += P                                          # the second representative, limb 8 above 2^24
            out.append((tag + "product %#x" % target, ma, mb, limbs9(x), limbs9(y)))
        out.append((tag + "p times random", ma, mb, limbs9(P), limbs9(rng.randrange(P))))
        for _ in range(12):
            out.append((tag + "random", ma, mb, [rng.randrange(ma * LB) for _ in range(9)], [rng.randrange(mb * LB) for _ in range(9)]))
    # an output limb at 2^29 or above, positions 3 .. 8: under a = 1 the columns are b's limbs, and the two carry passes leave
    # (2^29 - 1) + 1 at position p when b_(p - 2), b_(p - 1), b_p = 2^29, 2^30 - 1, 2^29 - 2
    for p in range(2, 9):
        b = [0] * 9
        b[p - 2], b[p - 1], b[p] = 1 << 29, (1 << 30) - 1, (1 << 29) - 2
        out.append(("2x2 carry pattern at %d" % p, 2, 2, [1] + [0] * 8, b))
    # ... positions 1 and 2, which stage 5 carries into: b_7, b_8 = 2^29, 2^30 - 1 send 1 to position 9 twice over (stage 2 folds
    # F0 into position 0 and F1 into position 1, stage 4 once more), and b_0, b_1, b_2 are cut so that position 0 resp. 1 passes
    # 2^29 only at stage 4 and its neighbour sits at 2^29 - 1
    tail = [0] * 4 + [1 << 29, (1 << 30) - 1]
    out.append(("2x2 carry pattern at 1", 2, 2, [1] + [0] * 8, [(1 << 29) - 1 - rm.F0, (1 << 29) - 1 - 2 * rm.F1, 0] + tail))
    out.append(("2x2 carry pattern at 2, folded", 2, 2, [1] + [0] * 8, [0, (1 << 29) - 2 * rm.F1, (1 << 29) - 1] + tail))
    # the climbs: from a = 1 (the landscape is b's limbs: smooth) and from the all-max pair
    climbs = [("stage2", lambda ev: ev["stage2"]), ("carry3", lambda ev: ev["carry3"]), ("out", lambda ev: max(ev["out"]))]
    for what, obj in climbs:
        for ma, mb in ((1, 7), (2, 2)):
            pool = []
            for _ in range(300):                                # the best of 300 random pairs (some limbs at their maximum) as a third start
                a = [rng.randrange(ma * LB) if rng.random() < 0.8 else ma * LB - 1 for _ in range(9)]
                b = [rng.randrange(mb * LB) if rng.random() < 0.8 else mb * LB - 1 for _ in range(9)]
                ev = {}
                rm.mul_rows(rm.row(a), rm.row(b), None, ev)
                pool.append((obj(ev), a, b))
            best = max(pool)
            starts = [([1] + [0] * 8, [rng.randrange(mb * LB) for _ in range(9)]), ([ma * LB - 1] * 9, [mb * LB - 1] * 9), (best[1], best[2])]
            for si, st in enumerate(starts):
                a, b = _climb(rng, ma, mb, obj, st, 400)
                out.append(("%dx%d climb %s from start %d" % (ma, mb, what, si), ma, mb, a, b))
    for label, ma, mb, a, b in out:
        assert len(a) == len(b) == 9 and max(a) < ma * LB and max(b) < mb * LB and ma * mb <= 7, label
    return out


def row_mul_expected(a, b, events=None):
    """the model's nine output limbs"""
    return rm.mul_rows(rm.row(a), rm.row(b), None, events)[:9]


def check_coverage_rows(vectors=None):
    """-> {name: maximum reached}; asserts every named event of the issue over the vector set, through the model"""
    vectors = row_mul_vectors() if vectors is None else vectors
    seen = {"th": set(), "tm28": False, "h0": False, "h15": False, "fold2": set(), "fold4": set(), "carry5": set(), "out29": set()}
    top = {"stage2": 0, "carry3": 0, "out": 0, "th": 0, "tm": 0}
    pairs = set()
    for label, ma, mb, a, b in vectors:
        ev = {}
        got = row_mul_expected(a, b, ev)
        assert value(got) % P == value(a) * value(b) % P, label
        pairs.add((ma, mb))
        seen["th"].add(ev["th"])
        seen["tm28"] |= bool(ev["tm"] >> 28)
        seen["h0"] |= ev["h0"] != 0
        seen["h15"] |= ev["h15"] != 0
        seen["fold2"] |= {p for p in range(11) if ev["fold2"][p]}
        seen["fold4"] |= {9 + t for t in range(2) if ev["fold4"][t]}
        seen["carry5"] |= {p for p in range(3) if ev["carry5"][p]}
        seen["out29"] |= {p for p in range(9) if ev["out"][p] >> 29}
        assert ev["out"][0] >> 29 == 0                      # position 0 takes no carry: its limb is 29 bits by construction
        for k in top:
            top[k] = max(top[k], max(ev[k]) if isinstance(ev[k], list) else ev[k])
    assert pairs == set(MAG_PAIRS) and set(STEP_PAIRS) <= pairs
    assert seen["th"] >= set(range(8)), seen["th"]
    assert seen["tm28"] and seen["h0"] and seen["h15"]
    assert seen["fold2"] == set(range(11)), seen["fold2"]
    assert seen["fold4"] == {9, 10}, seen["fold4"]
    assert seen["carry5"] == {0, 1, 2}, seen["carry5"]
    assert seen["out29"] == set(range(1, 9)), seen["out29"]
    return top


def coverage_report(top=None):
    """the text of profiles/msm_tail/coverage.txt: what the vector set reaches in the model, next to what the model asserts"""
    import math
    top = check_coverage_rows() if top is None else top
    lines = ["Row-parallel k256 multiplication (csrc/ecgpu_rows.h), model tools/rows_field_model.py: the maxima that the %d products of" % len(row_mul_vectors()),
             "tests/msm_tail_vectors.py reach, next to the bounds the model asserts at every product.  Written by",
             "`python tests/msm_tail_vectors.py`; tests/test_msm_tail_vectors.py compares.", "",
             "figure                     reached                       bound the model asserts",
             "top column, third piece    th = %d                        64-bit column; ma mb <= 7 gives th <= 7" % top["th"],
             "top column, second piece   tm = %#x (bit 28 set)    29 bits" % top["tm"],
             "stage-2 value              2^%.3f                      64 bits" % math.log2(top["stage2"]),
             "stage-3 carry              2^%.3f                      32 bits" % math.log2(top["carry3"]),
             "largest output limb        2^29 + %-7d                below LB = 2^29 + 2^20" % (top["out"] - (1 << 29)),
             "", "Events every run of check_coverage_rows asserts: th of every value 0 .. 7, tm with bit 28, h != 0 in columns 0 and 15, a",
             "non-zero stage-2 fold into each of positions 0 .. 10, a non-zero stage-4 fold from positions 9 and 10, a stage-5 carry out of",
             "positions 0, 1 and 2, an output limb at or above 2^29 at each of positions 1 .. 8.  Position 0 cannot: it takes no carry",
             "(out_0 = r2_0 mod 2^29), which the check asserts on every vector instead.", ""]
    return "\n".join(lines)


def raw_records(rows_per_wave, filler_seed=0x51DE):
    """[(limbs per wave row)] -> 16-word records, 64 per wave: the wave's lanes 0 .. len - 1 hold the given limbs, the other lanes
    junk that must not matter"""
    rng = random.Random(filler_seed)
    words = []
    for rows in rows_per_wave:
        assert len(rows) <= 4
        for lane in range(64):
            limbs = rows[lane] if lane < len(rows) else [rng.randrange(1 << 32) for _ in range(9)]
            words += list(limbs) + [0] * 7
    return words


# ---- norm64 ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def norm64_vectors():
    """[(label, nine values below 2^38)]"""
    rng = random.Random(0x6464)
    top = (1 << 38) - 1
    out = [("all 2^38 - 1", [top] * 9)]
    out += [("position %d alone" % i, [top if t == i else 0 for t in range(9)]) for i in range(9)]
    out += [("limb 9 of v1 at its largest", [0] * 7 + [M29 | (511 << 29), top])]
    out += [("all 2^29 - 1 and a carry", [M29] * 8 + [1 << 29]), ("zero", [0] * 9)]
    out += [("random", [rng.randrange(1 << 38) for _ in range(9)]) for _ in range(30)]
    # what step forms: small multiples of magnitude-1 limbs (63 (33 p - t2) + t0 is the largest)
    out += [("step's linear forms", [64 * (LB - 1) + rng.randrange(LB) for _ in range(9)]) for _ in range(4)]
    return out


def norm64_expected(v):
    return rm.norm64_rows(rm.row(v))[:9]


# ---- the doubling chain -------------------------------------------------------------------------------------------------------

DBL_STEPS = (1, 2, 4, 5, 13, 16)


@functools.lru_cache(maxsize=None)
def dbl_vectors():
    """[(label, X, Y, Z)] as nine raw limbs each, magnitudes up to (2, 2, 1); not all on the curve (the doubling is a polynomial
    identity, rm.ref_dbl is the expectation)"""
    rng = random.Random(0xDB1)
    G = pyec.G(K256)
    pt = pyec.mul(K256, 0x1234567, G)
    out = [("limits", [2 * LB - 1] * 9, [2 * LB - 1] * 9, [LB - 1] * 9),
           ("identity 0 : 1 : 0", [0] * 9, limbs9(1), [0] * 9),
           ("identity 0 : y : 0, lazy y", [0] * 9, [2 * LB - 1] * 9, [0] * 9),
           ("Z = 0 with X != 0", limbs9(rng.randrange(P)), limbs9(rng.randrange(1, P)), [0] * 9),
           ("G, Z = 1", limbs9(G[0]), limbs9(G[1]), limbs9(1)),
           ("a point in [p, 2p)", limbs9(pt[0] + P), limbs9(pt[1] + P), limbs9(1)),
           ("a point of order two would need y = 0: Y = 0", limbs9(pt[0]), [0] * 9, limbs9(1))]
    for _ in range(9):
        out.append(("random rows", [rng.randrange(2 * LB) for _ in range(9)], [rng.randrange(2 * LB) for _ in range(9)],
                    [rng.randrange(LB) for _ in range(9)]))
    return out


def dbl_expected(X, Y, Z, steps):
    """(X, Y, Z limbs by the model, (x, y, z) mod p by the formulas on integers)"""
    rx, ry, rz = rm.row(X), rm.row(Y), rm.row(Z)
    v = (value(X) % P, value(Y) % P, value(Z) % P)
    for _ in range(steps):
        rx, ry, rz = rm.dbl_rows(rx, ry, rz)
        v = rm.ref_dbl(*v)
    return (rx[:9], ry[:9], rz[:9]), v


# ---- points for the quad addition, the tree and the lane-shared doubling ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def base_points(name, count=12, seed=0x9A7):
    """[(s, s G)]: G, -G, 2 G, small and random multiples"""
    c = pyec.CURVES[name]
    rng = random.Random(seed + c.cid)
    ss = [1, c.n - 1, 2, c.n - 2, 3, (c.n - 1) // 2, (c.n + 1) // 2] + [rng.randrange(1, c.n) for _ in range(count - 7)]
    return [(s, pyec.mul(c, s, pyec.G(c))) for s in ss]


def quad_pairs(name):
    """[(P, Q)] for op 23: every edge pair (P + P, P - P, O + P, P + O, O + O) and generic pairs"""
    c = pyec.CURVES[name]
    pts = [pyec.INF] + [p for _, p in base_points(name)]
    out = [(a, b) for a in pts for b in pts]
    assert any(a == b and a is not pyec.INF for a, b in out) and any(a is not pyec.INF and b == pyec.neg(c, a) for a, b in out)
    return out


def quad_pairs_generic(name):
    """[(P, Q, P + 3 Q)] for op 24, X = P + Q and Y = 2 Q: with X = Y (P = Q), X = -Y (P = -3 Q), X = O (P = -Q), and generic"""
    c = pyec.CURVES[name]
    G = pyec.G(c)
    bp = base_points(name)
    out = []
    for s, q in bp:
        for t in (s, (-3 * s) % c.n, (-s) % c.n, (2 * s) % c.n, (5 * s + 7) % c.n):
            out.append((pyec.mul(c, t, G), q, pyec.mul(c, (t + 3 * s) % c.n, G)))
    return out


# ---- the Horner chain -----------------------------------------------------------------------------------------------------------

EVENTS = ("cancel", "cancel_end", "equal", "flip", "cancel2", "cancel3", "empty_top", "empty_mid", "single")
NFILL = 20


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def _fill_points(name):
    c = pyec.CURVES[name]
    rng = random.Random(0xF177 + c.cid)
    ss = [rng.randrange(1, c.n) for _ in range(NFILL)]
    return ss, [pyec.mul(c, s, pyec.G(c)) for s in ss]


def layout(name, glv, cbits):
    """(kbits, value_bits, nwin, wtop): wtop is the highest window a sub-scalar below 2^value_bits reaches"""
    kbits, value_bits = sv.geometry(name, glv)
    return kbits, value_bits, sv.window_count(kbits, cbits), (value_bits - 1) // cbits


def _digit_scalar(rng, kbits, value_bits, cbits, masked):
    """A sub-scalar from random signed digits, zero in the masked windows; the digits it was built from are the digits the recoding
    gives back (asserted by check_coverage_chain through the model)."""
    nwin = sv.window_count(kbits, cbits)
    half = 1 << (cbits - 1)
    rem = kbits % cbits
    digs = []
    for w in range(nwin):
        avail = min(cbits, value_bits - cbits * w)
        if w in masked or avail <= 0:
            digs.append(0)
        elif w == nwin - 1:
            digs.append(rng.randrange(1 << min(avail, rem)) if min(avail, rem) > 0 else 0)
        elif avail < cbits:
            digs.append(rng.randrange(1 << (avail - 1)))
        else:
            digs.append(rng.randrange(-(half - 1), half))
    live = [w for w in range(nwin) if digs[w]]
    if live:
        digs[live[-1]] = abs(digs[live[-1]])
    sub = sum(d << (cbits * w) for w, d in enumerate(digs))
    assert 0 <= sub < 1 << value_bits
    return sub


def term_logs(name, glv, cbits, k, s):
    """per window: the discrete logarithm of the term's contribution to the window sum, and whether the term has a digit there — from
    scalar_vectors' model of the split and the recoding"""
    c = pyec.CURVES[name]
    kbits = sv.geometry(name, glv)[0]
    nwin = sv.window_count(kbits, cbits)
    logs, live = [0] * nwin, [False] * nwin
    for h, (sub, flip) in enumerate(sv.subs(name, glv, k)):
        base = s * (sv.LAMBDA if h else 1) * (-1 if flip else 1)
        for w, d in enumerate(sv.signed_digits(sub, kbits, cbits)):
            if d:
                logs[w] = (logs[w] + d * base) % c.n
                live[w] = True
    return logs, live


def walk(c, cbits, wlogs):
    """the chain of k_msm_combine on logarithms: [(window, 2^c acc, W, acc after)] from the top window down"""
    nwin = len(wlogs)
    acc = wlogs[nwin - 1]
    steps = []
    for w in range(nwin - 2, -1, -1):
        t = acc * (1 << cbits) % c.n
        acc = (t + wlogs[w]) % c.n
        steps.append((w, t, wlogs[w], acc))
    return steps


def classify(c, t, W):
    if t == 0:
        return "from_identity" if W else "idle"
    if W == 0:
        return "plain_empty"
    if (t + W) % c.n == 0:
        return "cancel"
    if t == W:
        return "equal"
    if (W + 2 * t) % c.n == 0:
        return "flip"
    return "generic"


def build_chain(name, glv, cbits, events, seed=0):
    """events: [(kind, window)] with kind in EVENTS (empty_*: (kind, window, length): windows window .. window - length + 1 hold no
    digit).  -> Case(ks, ss, inf, points, planted, want_log)"""
    c = pyec.CURVES[name]
    kbits, value_bits, nwin, wtop = layout(name, glv, cbits)
    rng = random.Random(0xC4A1 + 1000 * c.cid + 16 * cbits + int(glv) + 7919 * seed)
    masked = set()
    for ev in events:
        kind, w = ev[0], ev[1]
        assert kind in EVENTS and 0 <= w <= wtop
        if kind in ("empty_top", "empty_mid"):
            masked |= set(range(w - ev[2] + 1, w + 1))
            assert w - ev[2] + 1 >= 0
        elif kind == "cancel_end":
            masked |= set(range(w))
        elif kind == "single":
            masked.add(w)
    fs, fp = _fill_points(name)
    ks, ss, pts, inf = [], [], [], []

    def scalar_of(subs_):
        if glv:
            return sv._glv_checked(tuple(subs_))
        sub, flip = subs_
        k = c.n - sub if flip and 0 < sub and sv.fold(c, c.n - sub) == (sub, True) else sub
        return k
    lim_bits = value_bits
    for i in range(NFILL):
        if glv:
            pair = tuple(rng.choice((1, -1)) * _digit_scalar(rng, kbits, lim_bits, cbits, masked) for _ in range(2))
            k = scalar_of(pair)
        else:
            k = scalar_of((_digit_scalar(rng, kbits, lim_bits, cbits, masked), i % 5 == 4))
        ks.append(k)
        ss.append(fs[i])
        pts.append(fp[i])
        inf.append(0)
    for pos in (2, 11):                                       # flagged identities: whatever their scalars, they add nothing
        ks.insert(pos, rng.randrange(c.n))
        ss.insert(pos, 0)
        pts.insert(pos, pyec.INF)
        inf.insert(pos, 1)

    def window_logs():
        wl = [0] * nwin
        for k, s, f in zip(ks, ss, inf):
            if not f:
                logs, _ = term_logs(name, glv, cbits, k, s)
                wl = [(a + b) % c.n for a, b in zip(wl, logs)]
        return wl

    planted = []
    G = pyec.G(c)
    # the fix-up terms, from the top window down: each one's point follows from the chain above its window
    todo = []
    for ev in events:
        kind, w = ev[0], ev[1]
        if kind in ("cancel", "cancel_end", "equal", "flip", "single"):
            todo.append((w, kind))
        elif kind in ("cancel2", "cancel3"):
            todo += [(w - j, "cancel" if j == 0 else "stay") for j in range(2 if kind == "cancel2" else 3)]
            assert w - (1 if kind == "cancel2" else 2) >= 0
        else:
            planted.append((kind, w, ev[2]))
    for w, kind in sorted(todo, reverse=True):
        assert w < wtop or kind == "single", "an event needs a window above it"
        wl = window_logs()
        steps = {st[0]: st for st in walk(c, cbits, wl)}
        t = steps[w][1] if w < nwin - 1 else 0
        have = wl[w]
        if kind in ("cancel", "cancel_end", "stay"):
            target = (-t) % c.n
        elif kind == "equal":
            target = t
        elif kind == "flip":
            target = (-2 * t) % c.n
        else:
            target = rng.randrange(1, c.n)                    # single: whatever point, alone in its window
        if kind in ("cancel", "cancel_end", "equal", "flip"):
            assert t != 0, "the accumulator above window %d is the identity: nothing to %s" % (w, kind)
        f = (target - have) % c.n
        assert f != 0, "window %d already holds what the event needs" % w
        half = w & 1 if glv else 0
        if glv:
            k = sv._glv_checked((1 << (cbits * w), 0) if half == 0 else (0, 1 << (cbits * w)))
            if half:
                f = f * pow(sv.LAMBDA, -1, c.n) % c.n
        else:
            k = 1 << (cbits * w)
        ks.append(k)
        ss.append(f)
        pts.append(pyec.mul(c, f, G))
        inf.append(0)
        planted.append((kind, w))
    want_log = sum(k * s for k, s, f in zip(ks, ss, inf) if not f) % c.n
    return Case(name=name, glv=glv, cbits=cbits, events=list(events), ks=ks, ss=ss, inf=inf, points=pts, planted=planted,
                masked=masked, want_log=want_log)


def check_coverage_chain(case):
    """Recompute the window sums from the finished scalars (the split and digit models of scalar_vectors), walk the chain, and
    assert: every planted event happens at its window, no exceptional step happens anywhere else, the masked windows hold no digit,
    and the chain's result is the dot product.  -> the classes of all steps, top window first"""
    c = pyec.CURVES[case.name]
    kbits, value_bits, nwin, wtop = layout(case.name, case.glv, case.cbits)
    wl, live = [0] * nwin, [0] * nwin
    for k, s, f in zip(case.ks, case.ss, case.inf):
        assert 0 <= k < c.n
        if f:
            continue
        logs, lv = term_logs(case.name, case.glv, case.cbits, k, s)
        wl = [(a + b) % c.n for a, b in zip(wl, logs)]
        live = [a + int(b) for a, b in zip(live, lv)]
    steps = walk(c, case.cbits, wl)
    assert (steps[-1][3] if steps else wl[0]) == case.want_log, "the chain does not end at the dot product"
    classes = {w: classify(c, t, W) for w, t, W, _ in steps}
    after = {w: a for w, _, _, a in steps}
    expected = {}
    for ev in case.planted:
        kind, w = ev[0], ev[1]
        if kind in ("cancel", "cancel_end"):
            expected[w] = "cancel"
            assert live[w] >= 2 and after[w] == 0
        elif kind == "stay":
            expected[w] = "idle"
            assert live[w] >= 2 and wl[w] == 0, "a window of non-identity parts that sum to the identity"
        elif kind in ("equal", "flip"):
            expected[w] = kind
        elif kind == "single":
            assert live[w] == 1 and wl[w] != 0
        else:
            for x in range(w - ev[2] + 1, w + 1):
                assert live[x] == 0, (kind, x)
    for w in case.masked:
        assert live[w] == (1 if ("single", w) in case.planted else 0), w
    for w, cl in classes.items():
        if w in expected:
            assert cl == expected[w], "window %d: planted %s, the chain shows %s" % (w, expected[w], cl)
        else:
            assert cl not in ("cancel", "equal", "flip"), "window %d: an accidental %s" % (w, cl)
    for ev in case.planted:
        if ev[0] == "cancel_end":
            assert case.want_log == 0
        if ev[0] == "cancel" and ev[1] > 0 and not any(e[0] == "cancel_end" for e in case.planted):
            assert any(live[x] for x in range(ev[1])), "a cancellation with nothing below it"
    return [classes[w] for w in sorted(classes, reverse=True)]


def event_windows(name, glv, cbits, sample=False):
    """the windows an event is planted at: every one below the highest live window, or top - 1, the first straddling one, middle, 1, 0"""
    kbits, value_bits, nwin, wtop = layout(name, glv, cbits)
    if not sample:
        return list(range(wtop - 1, -1, -1))
    strad = [w for w, _ in sv.straddling_windows(kbits, cbits, value_bits) if w < wtop]
    return sorted({wtop - 1, wtop // 2, 1, 0} | set(strad[:1]), reverse=True)


def cases_for(name, glv, cbits, kind, windows):
    """[Case] of one event kind over the given windows (empty runs: every length that fits, from the top and from `window`)"""
    kbits, value_bits, nwin, wtop = layout(name, glv, cbits)
    out = []
    if kind == "empty_top":
        return [build_chain(name, glv, cbits, [(kind, wtop, ln)]) for ln in range(1, wtop + 1)]
    if kind == "empty_mid":
        mid = max(wtop - 1, 1)
        return [build_chain(name, glv, cbits, [(kind, mid, ln)]) for ln in range(1, mid + 1)]
    for w in windows:
        need = {"cancel2": 1, "cancel3": 2}.get(kind, 0)
        if w - need < 0 or (kind == "cancel" and w == 0):
            continue
        out.append(build_chain(name, glv, cbits, [(kind, w)]))
    return out


# ---- two ranks, bucket reduction --------------------------------------------------------------------------------------------------

def two_rank_terms(name, glv, cbits, leave=None):
    """-> (Case of shard 0, Case of shard 1): shard 1 holds shard 0's terms with every point negated — every window sums to the
    identity out of non-identity parts — except, with `leave` = a window, one more term with the digit 1 in that window only."""
    c = pyec.CURVES[name]
    a = build_chain(name, glv, cbits, [], seed=5)
    b = Case(**dict(a.__dict__))
    b.ss = [(-s) % c.n for s in a.ss]
    b.points = [pyec.neg(c, p) if p is not pyec.INF else p for p in a.points]
    b.ks, b.inf = list(a.ks), list(a.inf)
    want = 0
    if leave is not None:
        k = sv._glv_checked((1 << (cbits * leave), 0)) if glv else 1 << (cbits * leave)
        s = 0xB0B + leave
        b.ks.append(k)
        b.ss.append(s)
        b.points.append(pyec.mul(c, s, pyec.G(c)))
        b.inf.append(0)
        want = k * s % c.n
    b.want_log = sum(k * s for k, s, f in zip(b.ks, b.ss, b.inf) if not f) % c.n
    return a, b, want


def bucket_cases(name, glv, cbits):
    """[(label, ks, ss)]: the same point / opposite points in two adjacent buckets d, d + 1 of one window — inside a segment, across a
    segment boundary (segments of four buckets: d = 4 j + 3 and 4 j + 4 as bucket indices d - 1), and in the top window's sub-buckets —
    among a few filler terms"""
    c = pyec.CURVES[name]
    kbits, value_bits, nwin, wtop = layout(name, glv, cbits)
    rng = random.Random(0xB0C + c.cid + cbits)
    out = []
    s0 = rng.randrange(1, c.n)
    mk = (lambda v: sv._glv_checked((v, 0))) if glv else (lambda v: v)
    top_digits = min(value_bits - cbits * wtop, kbits % cbits if wtop == nwin - 1 else cbits - 1)
    for where, w, ds in (("inside a segment", 1, (5, 6)), ("across a segment boundary", 1, (4, 5)), ("across the boundary of 8", 2, (8, 9)),
                         ("highest live window", wtop, (1, 2) if top_digits >= 2 else None)):
        if ds is None:
            continue
        for opposite in (False, True):
            ks = [mk(ds[0] << (cbits * w)), mk(ds[1] << (cbits * w))]
            ss = [s0, (-s0) % c.n if opposite else s0]
            for _ in range(6):
                ks.append(mk(_digit_scalar(rng, kbits, value_bits, cbits, set())))
                ss.append(rng.randrange(1, c.n))
            out.append(("%s, %s" % (where, "opposite points" if opposite else "the same point"), ks, ss))
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "profiles", "msm_tail", "coverage.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(coverage_report())
    print(open(path).read())
