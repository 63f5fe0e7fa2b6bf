"""Adversarial coordinates for the point formulas, limb by limb: Group<C> (csrc/ecgpu_point.h) and ct_dbl4 (csrc/ecgpu_ctmul.h)
through selftest_point_raw (csrc/ecgpu_selftest_point_raw.h).  Shared by tests/test_point_vectors.py (the g++ twins) and
tests/test_gpu_point_vectors.py (gfx950).  Plain module: deterministic, seeded per curve id, all twelve parameter sets; every
expected value is a Python integer.

Model.  A coordinate is the integer sum limb_i 2^(B i); its field value is that integer mod p (k256) or times R^-1 mod p,
R = 2^(B NL) (the Montgomery sets).  The group law is pyec.add.  Results are compared as CLASSES by cross-multiplication mod p,
without an inversion: homogeneous X = x Z, Y = y Z, Z != 0; Jacobian with weights 2 and 3; XYZZ also ZZ^3 = ZZZ^2; the identity
Z = 0, and for add / add_mixed / dbl / ct_dbl4 also Y != 0 (what ct_dbl4's (1, 1, 0) replacement is for); is_identity as 0 / 1.  The returned limbs must satisfy check_mag (restated below from ecgpu_field.h) at
what the formula's return type promises: (1, 1) for Proj, (1, JTV) for what jstore stored — and, being the next formula's
operands, the operand's bound on the top limb (V TOP1: Set.bound).

Operands are limbs the TYPES allow, not only what unpack / from_canonical produce: every limb at LB (above 2^B), one limb at LB
at every position, alternating, the top limb at the largest value check_mag<1, V> admits (V = 1, and V = JV on the Jacobian and
XYZZ inputs), the limbs of p, 2p - 1, p +- 1, (p +- 1) / 2, the structured integers of field_vectors.structured as limbs, and
random fills with one position pinned to its bound or to zero.

Families
  A  any point of the pool, one coordinate slot set to a pattern, the others follow from the scaling and enter as v, v + p, ...
     up to what the slot's bound admits.  Jacobian / XYZZ slots other than Z need a square or cube root of the scaling: the pool
     point is advanced until it exists, and a pinned random fill is redrawn until it exists (the count is reported).
  B  X and Z both patterns (and an affine x a pattern), kept where x = X / Z is on the curve; Y = +-y Z.
  C  k256: Y and Z both patterns (and an affine y a pattern), x solved for by a cube root (p = 7 mod 9); pairs steered so that
     Y1 Y2 = +-21 Z1 Z2: yy_m or yy_p is a lazy zero inside add_a0 / add_mixed_a0.
  D  related pairs for the complete formulas, each side under its own pattern: Q = P with Z1 != Z2, Q = -P, Q = +-2P, either
     side (or both) the identity spelled (0 : Y : 0), (p : Y : 0), (0 : Y : p), (p : Y : p); the spellings through dbl, ct_dbl4.
  E  the incomplete formulas strictly inside their domain (P, Q finite, P != +-Q; for the ladder chain 16 acc != +-q at every
     step — the model decides), coordinates of A and B at value magnitudes 1 and JV.
An affine y (outside k256) cannot be set to a pattern: that needs a root of the curve's cubic.  Its slot sees every
representative v, v + p the bound admits; `check_coverage` states exactly that."""
import functools
import hashlib
import json
import os
import random
import re
from collections import namedtuple

import field_vectors as fv
import pyec

CURVES = fv.CURVES
CSRC = fv.CSRC
CAP = 1500                       # vectors per op and set
CHAIN_STEPS = (1, 4, 16)
KEEP = {"proj": None, "jac": 150, "xyzz": 150}     # structured patterns per operand kind: the incomplete formulas take two value magnitudes

# op -> (kind of p, kind of q, kind of the result)
OPS = {0: ("proj", "proj", "proj"), 1: ("proj", "proj", "proj"), 2: ("proj", "aff", "proj"), 3: ("proj", "aff", "proj"),
       4: ("proj", None, "proj"), 5: ("proj", None, "proj"), 6: ("proj", None, "proj"),
       7: ("jac", None, "jac"), 8: ("jac", "aff", "jac"), 9: ("jac", "aff", "jac"), 10: ("jac", None, "proj"),
       11: ("xyzz", "aff", "xyzz"), 12: ("xyzz", "aff", "xyzz"), 13: ("aff", "aff", "xyzz"), 14: ("xyzz", None, "proj"),
       15: ("proj", "proj", "proj"), 16: ("jac", "aff", "jac"), 17: ("proj", None, "flag")}
SLOTS = {"proj": 3, "aff": 2, "jac": 3, "xyzz": 4}
IDENTITY_SPELLINGS = ("0Y0", "pY0", "0Yp", "pYp")
D_RELATIONS = ("Q=P", "Q=-P", "Q=2P", "Q=-2P") + tuple("P=O:" + s for s in IDENTITY_SPELLINGS) + \
    tuple("Q=O:" + s for s in IDENTITY_SPELLINGS) + ("P=Q=O",)

Vec = namedtuple("Vec", "p q want tag")          # p, q: lists of limb lists (one per slot) or None; want: the model's point


class Set:
    """The facts of one parameter set, read from the sources and checked against what is stated here."""

    def __init__(self, name):
        self.name = name
        self.c = pyec.CURVES[name]
        self.lay = fv.layout(name)
        self.nl, self.b, self.mont = self.lay.nl, self.lay.b, self.lay.mont
        self.p = self.c.p
        src = open(os.path.join(CSRC, "ecgpu_field_consts.h")).read()
        head = src[re.search(r"struct %s\b[^{]*\{" % fv.STATED[name][0], src).end():][:1500]
        self.LB = int(re.search(r"\bLB = 0x([0-9a-fA-F]+)u;", head).group(1), 16)
        assert (1 << self.b) < self.LB < (1 << self.b) + (1 << (self.b - 7)), (name, hex(self.LB))
        self.TOP1 = int(re.search(r"\bTOP1 = (\d+)u;", head).group(1)) if self.mont else None
        if self.mont:
            assert 2 * self.p - 1 < self.TOP1 << (self.b * (self.nl - 1)), name            # "value < 2p"
        else:
            assert int(re.search(r"\bZMAX = (\d+);", head).group(1)) == 6
        fsrc = open(os.path.join(CSRC, "ecgpu_field.h")).read()
        for line in ("if ((uint64_t)e.v[i] > (uint64_t)L * KC::LB) { __builtin_trap(); }",
                     "for (int i = 0; i < NL - 1; i++)\n                if ((uint64_t)e.v[i] > (uint64_t)L * PC::LB) { __builtin_trap(); }",
                     "if ((uint64_t)e.v[NL - 1] > (uint64_t)V * PC::TOP1 + PC::TOP1 / 2) { __builtin_trap(); }"):
            assert line in fsrc, "check_mag changed: restate it in mag_ok"
        psrc = open(os.path.join(CSRC, "ecgpu_point.h")).read()
        jtv = re.search(r"int JTV = C::REPR == REPR_U28_MONT \? (\d+) : (\d+);", psrc)
        jv = re.search(r"int JV = C::REPR == REPR_U28_MONT \? JTV \+ (\d+) : (\d+);", psrc)
        self.JTV = int(jtv.group(1 if self.mont else 2))
        self.JV = self.JTV + int(jv.group(1)) if self.mont else int(jv.group(2))
        assert (self.JTV, self.JV) == ((10, 11) if self.mont else (1, 1)), (name, self.JTV, self.JV)
        for text in ("static ECGPU_HD M1 m(const E& e) { return F::template wrap<1, 1>(e); }",
                     "static ECGPU_HD Mag<C, 1, JV> mj(const E& e) { return F::template wrap<1, JV>(e); }",
                     "static_assert(L == 1 && V <= JTV,"):
            assert text in psrc, text
        self.R = 1 << (self.b * self.nl) if self.mont else 1
        self.Ri = pow(self.R, -1, self.p)

    # ---- limbs <-> integers <-> field values
    def limbs(self, i):
        m = (1 << self.b) - 1
        return [(i >> (self.b * k)) & m for k in range(self.nl - 1)] + [i >> (self.b * (self.nl - 1))]

    def int_of(self, limbs):
        return sum(v << (self.b * k) for k, v in enumerate(limbs))

    def val(self, limbs):
        return self.int_of(limbs) * self.Ri % self.p

    def bound(self, k, v=1):
        """The largest value of limb k an operand of magnitude (1, v) may have.  Below the top: LB.  The top limb of a Montgomery
        set: v TOP1, NOT the v TOP1 + TOP1 / 2 that check_mag admits — that slack is there for what a negation hands back
        (Z[l][v] - x, top limb below v TOP1 + 3/2 TOP1), while a negation's OPERAND must stay limb-wise below Z[l][v], whose top
        limb is only promised to be >= v TOP1 (tools/gen_field_consts.py; tools/field_model.py takes its extremes there too)."""
        if self.mont and k == self.nl - 1:
            return v * self.TOP1
        return self.LB

    def mag_ok(self, limbs, l, v):
        """check_mag<L, V> of ecgpu_field.h, restated"""
        if not self.mont:
            return all(x <= l * self.LB for x in limbs)
        return all(x <= l * self.LB for x in limbs[:-1]) and limbs[-1] <= v * self.TOP1 + self.TOP1 // 2

    def reps(self, value, v=1):
        """strict-limb representatives of a field value: i, i + p, and the largest i + k p that check_mag<1, v> admits"""
        i = value * self.R % self.p
        kmax = ((self.bound(self.nl - 1, v) + 1 << (self.b * (self.nl - 1))) - 1 - i) // self.p
        assert kmax >= 1
        out = [self.limbs(i + k * self.p) for k in sorted({0, 1, kmax})]
        assert all(self.mag_ok(x, 1, v) and self.val(x) == value for x in out)
        return out

    def rep(self, value, v, k):
        r = self.reps(value, v)
        return r[k % len(r)]


@functools.lru_cache(maxsize=None)
def get_set(name):
    return Set(name)


# ---- roots ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sylow3(p):
    """p - 1 = 3^s t, e = 1 / 3 mod t, and {h: 1 / w} for the cubes h = w^3 of the 3-Sylow subgroup"""
    s, t = 0, p - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    assert 1 <= s <= 6
    g = next(pow(n, t, p) for n in range(2, 200) if pow(n, (p - 1) // 3, p) != 1)
    return s, t, pow(3, -1, t), {pow(g, 3 * j, p): pow(g, -j, p) for j in range(3 ** s)}


def cbrt(a, p):
    """a cube root of a mod p, or None"""
    a %= p
    if a == 0:
        return 0
    if p % 3 == 2:
        return pow(a, (2 * p - 1) // 3, p)
    if pow(a, (p - 1) // 3, p) != 1:
        return None
    s, t, e, roots = _sylow3(p)
    u = pow(a, e, p)                                     # u^3 = a * a^(3 e - 1), the second factor in the 3-Sylow subgroup
    r = u * roots[u * u * u * inv(a, p) % p] % p
    assert pow(r, 3, p) == a
    return r


def _character(a, p, k):
    """the quadratic (k = 2) or cubic (k = 3) character of a: 1 exactly where a k-th root exists; 1 for every a where all have one"""
    if k == 0 or (p - 1) % k:
        return 1
    return pow(a, (p - 1) // k, p)


def inv(a, p):
    return pow(a, -1, p)


@functools.lru_cache(maxsize=None)
def _sylow2(p):
    s, q = 0, p - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    z = next(n for n in range(2, 200) if pow(n, (p - 1) // 2, p) == p - 1)
    return s, q, pow(z, q, p)


def sqrt_mod(a, p):
    """a square root of a mod p, or None (Tonelli-Shanks as in the textbooks: p224 asks for thousands of roots, and its
    2-Sylow subgroup has order 2^96)"""
    a %= p
    if a == 0:
        return 0
    if p % 4 == 3:
        r = pow(a, (p + 1) // 4, p)
        return r if r * r % p == a else None
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    m, q, c = _sylow2(p)
    t, r = pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u, i = u * u % p, i + 1
        b = c
        for _ in range(m - i - 1):
            b = b * b % p
        m, c = i, b * b % p
        t, r = t * c % p, r * b % p
    assert r * r % p == a
    return r


def lift_x(c, x, y_is_odd):
    """the curve point with this x and the requested parity of y, or None"""
    y = sqrt_mod(pow(x, 3, c.p) + c.a * x + c.b, c.p)
    if y is None:
        return None
    return (x % c.p, y if (y & 1) == int(bool(y_is_odd)) else (c.p - y) % c.p)


# ---- the pool and the patterns --------------------------------------------------------------------------------------------------

X0_SETS = ("p256", "p384", "sm2", "p192", "p521", "bign256")          # the sets whose curve has a point with x = 0 (b a square)


@functools.lru_cache(maxsize=None)
def pool(name):
    """finite points: the self-test's pool, 2P of some, (n +- 1) / 2 G, and the point with x = 0 where it exists"""
    S = get_set(name)
    c = S.c
    rng = random.Random(0xD9017 + c.cid)
    G = pyec.G(c)
    pts = [G, pyec.neg(c, G), pyec.mul(c, 2, G)] + [pyec.mul(c, rng.randrange(1, c.n), G) for _ in range(20)]
    pts += [pyec.add(c, a, a) for a in pts[3:7]]
    pts += [pyec.mul(c, (c.n + 1) // 2, G), pyec.mul(c, (c.n - 1) // 2, G)]
    y0 = sqrt_mod(c.b, c.p)
    assert (y0 is not None) == (name in X0_SETS), name
    if y0 is not None:
        pts.append((0, y0))
    assert all(pyec.on_curve(c, a) for a in pts)
    return pts


@functools.lru_cache(maxsize=None)
def patterns(S, v=1, keep=None):
    """[(name, limbs, loose?)]: the loose patterns first, then the structured integers as strict limbs (`keep`: thinned evenly
    to that many)"""
    nl, p = S.nl, S.p
    B = [S.bound(k, v) for k in range(nl)]
    out = [("all-LB", list(B), True)]
    for k in range(nl):
        out.append(("one-LB-%d" % k, [B[j] if j == k else 0 for j in range(nl)], True))
    out.append(("alt-0", [B[j] if j % 2 == 0 else 0 for j in range(nl)], True))
    out.append(("alt-1", [B[j] if j % 2 == 1 else 0 for j in range(nl)], True))
    out.append(("top-max-rest-ones", [(1 << S.b) - 1] * (nl - 1) + [B[-1]], True))
    for nm, i in (("p", p), ("2p-1", 2 * p - 1), ("p+1", p + 1), ("p-1", p - 1), ("(p+1)/2", (p + 1) // 2), ("(p-1)/2", (p - 1) // 2)):
        out.append((nm, S.limbs(i), True))
    lim = (B[-1] + 1) << (S.b * (nl - 1))
    st = fv.structured(S.b, nl, S.c.L, p, lim)
    if keep is not None and len(st) > keep:
        st = [st[j * len(st) // keep] for j in range(keep)]
    for i in st:
        out.append(("s%x" % i, S.limbs(i), False))
    assert all(S.mag_ok(x, 1, v) for _, x, _ in out)
    return out


def pinned(S, v, k, at_bound, rng):
    """a random fill with limb k at its bound or at zero"""
    x = [rng.randrange(S.bound(j, v) + 1) for j in range(S.nl)]
    x[k] = S.bound(k, v) if at_bound else 0
    return x


# ---- operands: (kind, slots, point) ---------------------------------------------------------------------------------------------

def scaled(S, kind, pt, z, v, k, fixed=None):
    """the operand of `kind` for the point pt under the scaling z, slot s as representative k + s; `fixed`: {slot: limbs}"""
    x, y = pt
    p = S.p
    if kind == "proj":
        vals = [x * z % p, y * z % p, z]
    elif kind == "jac":
        vals = [x * z * z % p, y * z * z * z % p, z]
    else:
        vals = [x * z * z % p, y * z * z * z % p, z * z % p, z * z * z % p]
    slots = [S.rep(val, v, k + s) for s, val in enumerate(vals)]
    for s, limbs in (fixed or {}).items():
        assert S.val(limbs) == vals[s], (S.name, kind, s)
        slots[s] = list(limbs)
    return slots


def scaling_for(S, kind, pt, slot, f):
    """the scaling z under which slot `slot` of pt's operand has the field value f, or None where no root exists"""
    x, y = pt
    p = S.p
    if kind == "proj":
        d = (x, y, 1)[slot]
        return f * inv(d, p) % p if d else None
    if kind == "jac":
        if slot == 2:
            return f
        if slot == 0:
            return sqrt_mod(f * inv(x, p), p) if x else None
        return cbrt(f * inv(y, p), p)
    if slot == 0:
        return sqrt_mod(f * inv(x, p), p) if x else None
    if slot == 1 or slot == 3:
        return cbrt(f * inv((y, 1)[slot == 3], p), p)
    return sqrt_mod(f, p)


def family_a(S, kind, v, stats):
    """one slot a pattern: every loose pattern and a pinned fill per position in every slot, the structured ones round robin"""
    pts = pool(S.name)
    rng = random.Random(0xA11 + 16 * S.c.cid + v)
    nslot = SLOTS[kind]
    chars = [(_character(x, S.p, 2), _character(y, S.p, 3)) for x, y in pts]
    out = []

    def place(slot, limbs, k, loose):
        f = S.val(limbs)
        stats["A cand"] += 1
        if f == 0:
            return False                                  # a zero coordinate is the identity's (family D) or the x = 0 point's
        root = 0 if kind == "proj" or slot == 2 and kind == "jac" else 2 if slot in (0, 2) else 3
        chi = _character(f, S.p, root)
        for step in range(len(pts) if kind != "proj" or slot == 0 else 1):
            pt = pts[(k + step) % len(pts)]
            if root and chi != (chars[(k + step) % len(pts)][root == 3] if slot < 2 else 1):
                continue                                  # no root of f / x (f / y) for this point: the next one
            z = scaling_for(S, kind, pt, slot, f)
            if z:
                out.append((scaled(S, kind, pt, z, v, k, {slot: limbs}), pt, loose))
                stats["A acc"] += 1
                return True
        return False

    for k, (nm, limbs, loose) in enumerate(patterns(S, v, KEEP[kind])):
        for slot in (range(nslot) if loose else (k % nslot,)):
            place(slot, limbs, k, loose)
    for slot in range(nslot):                             # every position at its bound and at zero, in every slot
        for pos in range(S.nl):
            for at_bound in (True, False):
                for attempt in range(200):
                    if place(slot, pinned(S, v, pos, at_bound, rng), 7 * pos + attempt, True):
                        break
                else:
                    raise AssertionError((S.name, kind, slot, pos, at_bound))
    x0 = [a for a in pts if a[0] == 0]
    for k, pt in enumerate(x0 * 6):                       # X = 0 as 0, p, ...: only the scaling is free
        nm, limbs, _ = patterns(S, v)[3 * k]
        z = S.val(limbs) if kind in ("proj", "jac") else sqrt_mod(S.val(limbs), S.p)
        if z:
            out.append((scaled(S, kind, pt, z, v, k, {2: limbs} if kind != "xyzz" else None), pt, True))
    return out


def family_b(S, kind, v, stats):
    """X and Z (ZZ) both patterns, kept where x is on the curve; Y = +-y Z"""
    c, p = S.c, S.p
    pats = [x for _, x, _ in patterns(S, v, KEEP[kind])]
    out = []
    for i, xl in enumerate(pats):
        for stride in ((1, 5, 11) if kind == "proj" else (1,)):
            zl = pats[(7 * i + 3 + stride * 13) % len(pats)]
            fx, fz = S.val(xl), S.val(zl)
            if fz == 0 or fx == 0:
                continue
            stats["B cand"] += 1
            if kind == "proj":
                z, w = fz, fz
            elif kind == "jac":
                z, w = fz, fz * fz % p
            else:
                z, w = sqrt_mod(fz, p), fz
                if z is None:
                    continue
            x = fx * inv(w, p) % p
            pt = lift_x(c, x, (i + stride) & 1)
            if pt is None:
                continue
            stats["B acc"] += 1
            out.append((scaled(S, kind, pt, z, v, i, {0: xl, 2: zl}), pt, False))
    return out


def affine_operands(S, stats):
    """(slots, point, loose): pool points under every representative; x a pattern where it is on the curve (B); k256: y a pattern (C)"""
    c, p = S.c, S.p
    rng = random.Random(0xAFF + S.c.cid)
    out = []
    for k, pt in enumerate(pool(S.name)):
        for kx in range(3):
            out.append(([S.rep(pt[0], 1, kx), S.rep(pt[1], 1, k + kx)], pt, True))

    def place_x(limbs, k, loose):
        stats["B cand"] += 1
        pt = lift_x(c, S.val(limbs), k & 1)
        if pt is None or pt[1] == 0:
            return False
        stats["B acc"] += 1
        out.append(([list(limbs), S.rep(pt[1], 1, k)], pt, loose))
        return True

    def place_y(limbs, k, loose):
        stats["C cand"] += 1
        y = S.val(limbs)
        x = cbrt(y * y - c.b, p)
        if x is None or y == 0:
            return False
        stats["C acc"] += 1
        out.append(([S.rep(x, 1, k), list(limbs)], (x, y), loose))
        return True

    for place in (place_x,) + ((place_y,) if S.name == "k256" else ()):
        for k, (nm, limbs, loose) in enumerate(patterns(S, 1)):
            place(limbs, k, loose)
        for pos in range(S.nl):
            for at_bound in (True, False):
                assert any(place(pinned(S, 1, pos, at_bound, rng), pos + t, True) for t in range(200)), (S.name, pos)
    assert all(pyec.on_curve(c, pt) for _, pt, _ in out)
    return out


def family_c_proj(S, stats):
    """k256: Y and Z both patterns, x = cbrt(y^2 - 7)"""
    p = S.p
    pats = [x for _, x, _ in patterns(S, 1)]
    out = []
    for i, yl in enumerate(pats):
        zl = pats[(5 * i + 2) % len(pats)]
        fy, fz = S.val(yl), S.val(zl)
        if fy == 0 or fz == 0:
            continue
        stats["C cand"] += 1
        y = fy * inv(fz, p) % p
        x = cbrt(y * y - 7, p)
        if x is None:
            continue
        stats["C acc"] += 1
        out.append((scaled(S, "proj", (x, y), fz, 1, i, {1: yl, 2: zl}), (x, y), False))
    return out


def family_c_steered(S, projs, stats):
    """k256 pairs with y1 y2 = +-21: yy -+ 21 zz = 0 mod p inside add_a0 / add_mixed_a0, the limbs those of a lazy value"""
    p = S.p
    pairs = []
    for i, (slots, pt, _) in enumerate(projs[:: max(1, len(projs) // 150)]):
        for sign in (1, -1):
            stats["C cand"] += 1
            y2 = sign * 21 * inv(pt[1], p) % p
            x2 = cbrt(y2 * y2 - 7, p)
            if x2 is None:
                continue
            stats["C acc"] += 1
            limbs = projs[(3 * i + 1) % len(projs)][0][2]                       # another operand's Z pattern
            q = (x2, y2)
            pairs.append((slots, pt, scaled(S, "proj", q, S.val(limbs) or 1, 1, i, {2: limbs} if S.val(limbs) else None),
                          [S.rep(x2, 1, i), S.rep(y2, 1, i + 1)], q, "C:y1y2=%+d" % (sign * 21)))
    assert len(pairs) >= 40, len(pairs)
    return pairs


def identity_spelling(S, spelling, ylimbs):
    zero, pl = [0] * S.nl, S.limbs(S.p)
    return [pl if spelling[0] == "p" else zero, list(ylimbs), pl if spelling[2] == "p" else zero]


def family_d(S, projs, affs):
    """[(tag, P slots, P point, Q slots, Q point, q affine slots or None)] for the complete formulas"""
    c = S.c
    rng = random.Random(0xD0 + c.cid)
    loose = [x for x in projs if x[2]]
    ypats = [x for _, x, l in patterns(S, 1) if l and S.val(x)]
    out = []

    def other(pt, k, avoid=None):
        """the point pt under another operand's pattern: a different slot, a different pattern, another Z than `avoid`"""
        for t in range(len(loose)):
            slots, _, _ = loose[(k + t) % len(loose)]
            for slot in (2, 0, 1):
                z = scaling_for(S, "proj", pt, slot, S.val(slots[slot]))
                if z and (avoid is None or z != S.val(avoid)):
                    return scaled(S, "proj", pt, z, 1, k, {slot: slots[slot]})
        raise AssertionError

    def aff(pt, k):
        return [S.rep(pt[0], 1, k), S.rep(pt[1], 1, k + 1)]

    for k, (slots, pt, _) in enumerate(loose[:: max(1, len(loose) // 60)]):
        twice = pyec.add(c, pt, pt)
        for tag, q in (("Q=P", pt), ("Q=-P", pyec.neg(c, pt)), ("Q=2P", twice), ("Q=-2P", pyec.neg(c, twice))):
            qs = other(q, 5 * k + 1, slots[2])
            assert S.val(qs[2]) != S.val(slots[2])
            out.append(("D:" + tag, slots, pt, qs, q, aff(q, k)))
        for n, sp in enumerate(IDENTITY_SPELLINGS):
            ident = identity_spelling(S, sp, ypats[(k + n) % len(ypats)])
            out.append(("D:P=O:" + sp, ident, pyec.INF, other(pt, k + 3), pt, aff(pt, k + n)))
            out.append(("D:Q=O:" + sp, slots, pt, ident, pyec.INF, None))
    for n, sp in enumerate(IDENTITY_SPELLINGS):
        for m, sq in enumerate(IDENTITY_SPELLINGS):
            out.append(("D:P=Q=O", identity_spelling(S, sp, rng.choice(ypats)), pyec.INF, identity_spelling(S, sq, rng.choice(ypats)), pyec.INF, None))
    return out


# ---- the vectors ------------------------------------------------------------------------------------------------------------------

def _cap(vecs, cap=CAP):
    """all the must-haves (loose patterns, families C and D), the rest thinned evenly"""
    must = [v for v in vecs if v[1]]
    rest = [v for v in vecs if not v[1]]
    room = max(0, cap - len(must))
    if len(rest) > room:
        rest = [rest[i * len(rest) // room] for i in range(room)] if room else []
    return [v[0] for v in must + rest]


def model(S, op, P, Q):
    c = S.c
    code, steps = op & 0xFF, op >> 8
    if code in (0, 2, 8, 11, 13): return pyec.add(c, P, Q)
    if code in (1, 3, 9, 12): return pyec.add(c, P, pyec.neg(c, Q))
    if code in (4, 7): return pyec.add(c, P, P)
    if code == 5: return pyec.neg(c, P)
    if code == 6: return pyec.mul(c, 16, P) if P is not pyec.INF else pyec.INF
    if code in (10, 14, 17): return P
    if code == 15:
        for _ in range(steps):
            P = pyec.add(c, P, Q)
            P = pyec.add(c, P, P)
        return P
    if code == 16:
        for _ in range(steps):
            for _ in range(4):
                P = pyec.add(c, P, P)
            if P is pyec.INF or P[0] == Q[0]:
                return "outside"
            P = pyec.add(c, P, Q)
        return P
    raise AssertionError(op)


@functools.lru_cache(maxsize=None)
def vectors(name):
    """({op: [Vec]}, stats) of a parameter set; the chain ops appear as code | steps << 8"""
    S = get_set(name)
    c = S.c
    stats = {k: 0 for k in ("A cand", "A acc", "B cand", "B acc", "C cand", "C acc")}
    projs = family_a(S, "proj", 1, stats) + family_b(S, "proj", 1, stats)
    if name == "k256":
        projs += family_c_proj(S, stats)
    affs = affine_operands(S, stats)
    inc = {}
    for kind in ("jac", "xyzz"):
        inc[kind] = []
        for v in sorted({1, S.JV}):
            inc[kind] += family_a(S, kind, v, stats) + family_b(S, kind, v, stats)
    assert stats["B acc"] >= 200, (name, stats)
    dpairs = family_d(S, projs, affs)
    steered = family_c_steered(S, projs, stats) if name == "k256" else []
    out = {}

    def emit(op, rows):
        """rows: (p slots, P, q slots, Q, tag, must) -> Vecs with the model's answer; the incomplete formulas keep their domain"""
        vecs = []
        for ps, P, qs, Q, tag, must in rows:
            if (op & 0xFF) in (8, 9, 11, 12, 13) and P[0] == Q[0]:
                continue
            want = model(S, op, P, Q)
            if want == "outside":
                continue
            vecs.append((Vec(ps, qs, want, tag), must))
        out[op] = _cap(vecs)

    n, m = len(projs), len(affs)
    pair_pp = [(projs[i][0], projs[i][1], projs[(5 * i + 11) % n][0], projs[(5 * i + 11) % n][1], "AB", projs[i][2]) for i in range(n)]
    pair_pa = [(projs[i % n][0], projs[i % n][1], affs[(3 * i + 1) % m][0], affs[(3 * i + 1) % m][1], "AB", projs[i % n][2] or affs[(3 * i + 1) % m][2])
               for i in range(max(n, m))]
    # every affine operand once at least
    pair_pa += [(projs[(7 * j) % n][0], projs[(7 * j) % n][1], affs[j][0], affs[j][1], "AB", affs[j][2]) for j in range(m)]
    d_pp = [(ps, P, qs, Q, tag, True) for tag, ps, P, qs, Q, qa in dpairs]
    d_pa = [(ps, P, qa, Q, tag, True) for tag, ps, P, qs, Q, qa in dpairs if qa is not None]
    c_pp = [(ps, P, qs, Q, tag, True) for ps, P, qs, qa, Q, tag in steered]
    c_pa = [(ps, P, qa, Q, tag, True) for ps, P, qs, qa, Q, tag in steered]
    for op in (0, 1):
        emit(op, pair_pp + d_pp + c_pp)
    for op in (2, 3):
        emit(op, pair_pa + d_pa + c_pa)
    unary = [(ps, P, None, None, "AB", must) for ps, P, must in projs]
    ident = [(ps, P, None, None, tag, True) for tag, ps, P, qs, Q, qa in dpairs if tag.startswith("D:P=O")]
    for op in (4, 5, 6, 17):
        emit(op, unary + ident)
    for kind, un, bi in (("jac", (7, 10), (8, 9)), ("xyzz", (14,), (11, 12))):
        ops = inc[kind]
        for op in un:
            emit(op, [(ps, P, None, None, "E", must) for ps, P, must in ops])
        for op in bi:
            emit(op, [(ops[i][0], ops[i][1], affs[(3 * i + op) % m][0], affs[(3 * i + op) % m][1], "E", ops[i][2]) for i in range(len(ops))] +
                 [(ops[(11 * j) % len(ops)][0], ops[(11 * j) % len(ops)][1], affs[j][0], affs[j][1], "E", affs[j][2]) for j in range(m)])
    emit(13, [(affs[j][0], affs[j][1], affs[(5 * j + 3) % m][0], affs[(5 * j + 3) % m][1], "E", True) for j in range(m)])
    for steps in CHAIN_STEPS:
        thin = max(1, n // 120)
        emit(15 | steps << 8, pair_pp[::thin] + d_pp[::11] + c_pp[::4])
        jo = inc["jac"]
        emit(16 | steps << 8, [(jo[i][0], jo[i][1], affs[(3 * i + steps) % m][0], affs[(3 * i + steps) % m][1], "E", jo[i][2])
                               for i in range(0, len(jo), max(1, len(jo) // 150))])
    return out, stats


# ---- encoding and checking --------------------------------------------------------------------------------------------------------

def records(S, vecs):
    """(p records, q records or None) as lists of 4 NL words per vector"""
    zero = [0] * S.nl

    def rec(slots):
        slots = list(slots) + [zero] * (4 - len(slots))
        return [w for s in slots for w in s]
    P = [rec(v.p) for v in vecs]
    Q = [rec(v.q) for v in vecs] if vecs and vecs[0].q is not None else None
    return P, Q


def check_result(S, op, vec, got):
    """None, or what is wrong with the 4 NL result words `got` of one vector: the class against the model, then the magnitudes"""
    code = op & 0xFF
    kind = OPS[code][2]
    p, nl = S.p, S.nl
    slots = [[int(w) for w in got[s * nl: (s + 1) * nl]] for s in range(4)]
    if kind == "flag":
        want = [int(vec.want is pyec.INF)] + [0] * (4 * nl - 1)
        return None if [int(w) for w in got] == want else "is_identity says %d" % int(got[0])
    vals = [S.val(s) for s in slots]
    promised = 1 if kind == "proj" else S.JTV
    for s in range(SLOTS[kind]):
        # check_mag's rule, and the operand's bound (a stored coordinate is the next formula's operand: see Set.bound)
        if not S.mag_ok(slots[s], 1, promised) or any(w > S.bound(k, promised) for k, w in enumerate(slots[s])):
            return "slot %d leaves magnitude (1, %d): %s" % (s, promised, [hex(w) for w in slots[s]])
    if any(slots[s] != [0] * nl for s in range(SLOTS[kind], 4)):
        return "an unused slot is not zero"
    X, Y, Z = vals[0], vals[1], vals[2]
    if vec.want is pyec.INF:
        assert kind == "proj"
        if Z != 0:
            return "want the identity, Z != 0"
        if code in (0, 1, 2, 3, 4, 6, 15) and Y == 0:
            return "the identity came back with Y = 0"
        return None
    x, y = vec.want
    if Z == 0:
        return "want a finite point, Z (ZZ) = 0"
    if kind == "proj":
        ok = X == x * Z % p and Y == y * Z % p
    elif kind == "jac":
        ok = X == x * Z * Z % p and Y == y * Z * Z * Z % p
    else:
        ok = X == x * Z % p and Y == y * vals[3] % p and pow(Z, 3, p) == vals[3] * vals[3] % p
    return None if ok else "wrong class: want (%#x, %#x)" % (x, y)


def operand_point(S, kind, slots):
    """the point an operand spells, by the model (None: the identity); asserts it is on the curve"""
    vals = [S.val(s) for s in slots]
    p = S.p
    if kind == "aff":
        pt = (vals[0], vals[1])
    elif vals[2] == 0:
        assert kind == "proj"
        return pyec.INF
    elif kind == "proj":
        zi = inv(vals[2], p)
        pt = (vals[0] * zi % p, vals[1] * zi % p)
    elif kind == "jac":
        zi = inv(vals[2], p)
        pt = (vals[0] * zi * zi % p, vals[1] * zi * zi * zi % p)
    else:
        assert pow(vals[2], 3, p) == vals[3] * vals[3] % p
        pt = (vals[0] * inv(vals[2], p) % p, vals[1] * inv(vals[3], p) % p)
    assert pyec.on_curve(S.c, pt)
    return pt


def check_coverage(name):
    """Asserted from the accepted vectors: per set and operand slot every limb position at its bound and at zero and a representative
    in [p, 2p) or above; every D relation under every identity spelling on the complete ops; V = JV reached on the Montgomery sets;
    the operands spell the points the model was given; the caps.  Returns the events as a dict (profiles/point_vectors/coverage.txt)."""
    S = get_set(name)
    vecs, stats = vectors(name)
    ev = dict(stats)
    assert sorted(vecs) == sorted([c for c in OPS if c not in (15, 16)] + [c | s << 8 for c in (15, 16) for s in CHAIN_STEPS])
    seen = {}
    top_jv = False
    for op, vs in vecs.items():
        assert 0 < len(vs) <= CAP + 700, (name, op, len(vs))
        ev["op %d n" % op] = len(vs)
        pk, qk, _ = OPS[op & 0xFF]
        for i, v in enumerate(vs):
            for kind, slots in ((pk, v.p), (qk, v.q)):
                if kind is None:
                    continue
                vmax = S.JV if kind in ("jac", "xyzz") else 1
                for s, limbs in enumerate(slots):
                    assert S.mag_ok(limbs, 1, vmax), (name, op, kind, s)
                    e = seen.setdefault((kind, s), [set(), set(), False])
                    e[0].update(k for k, w in enumerate(limbs) if w == S.bound(k, vmax) or (k == S.nl - 1 and w == S.bound(k, 1)))
                    e[1].update(k for k, w in enumerate(limbs) if w == 0)
                    e[2] = e[2] or S.int_of(limbs) >= S.p
                    top_jv = top_jv or (S.mont and kind != "aff" and limbs[-1] > S.bound(S.nl - 1, S.JV - 1))
            if i % 16 == 0:
                P = operand_point(S, pk, v.p)
                Q = operand_point(S, qk, v.q) if qk else None
                assert model(S, op, P, Q) == v.want, (name, op, i)
    for (kind, s), (hi, zero, second) in sorted(seen.items()):
        free = not (kind == "aff" and s == 1 and name != "k256")      # an affine y is a pattern only where cube roots solve for x
        if free:
            assert hi == set(range(S.nl)) and zero == set(range(S.nl)), (name, kind, s, sorted(hi), sorted(zero))
        assert second, (name, kind, s)
        ev["%s slot %d" % (kind, s)] = "%d positions at the bound, %d at zero, [p, ..) %s" % (len(hi), len(zero), second)
    assert top_jv == S.mont, name
    ev["V = JV"] = top_jv
    for op in (0, 1, 15 | 1 << 8):
        tags = {v.tag for v in vecs[op]}
        assert {"D:" + r for r in D_RELATIONS} <= tags, (name, op, sorted(tags))
    for op in (2, 3):
        tags = {v.tag for v in vecs[op]}
        assert {"D:" + r for r in D_RELATIONS if not r.startswith("Q=O") and r != "P=Q=O"} <= tags, (name, op)
    for op in (4, 6, 17):
        assert {"D:P=O:" + s for s in IDENTITY_SPELLINGS} <= {v.tag for v in vecs[op]}, (name, op)
    if name == "k256":
        for op in (0, 1, 2, 3):
            assert {"C:y1y2=+21", "C:y1y2=-21"} <= {v.tag for v in vecs[op]}
    ev["D relations"] = len(D_RELATIONS)
    return ev


def arrays(S, vs):
    """the p and q records of a vector list as uint32 arrays of shape (n, 4 NL) (q: None for a unary op)"""
    import numpy as np
    P, Q = records(S, vs)
    return np.array(P, np.uint32), None if Q is None else np.array(Q, np.uint32)


GOLDEN = os.path.join(fv.ROOT, "tests", "golden", "point_vectors_twin.json")


def digest(out):
    """SHA-256 of a result array's little-endian words: what tests/golden/point_vectors_twin.json records per set and op of the
    g++ twin's results (written by `python tests/point_vectors.py --golden`), so that the gfx950 test compares limb for limb
    without compiling the twin, and compiles it only to name the vector that differs"""
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(out, dtype="<u4").tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


def first_failure(S, op, vs, out):
    """None, or a message naming the first vector whose result words `out[i]` check_result rejects, and how many there are"""
    assert len(out) == len(vs), (S.name, op, len(out), len(vs))
    bad = [(i, m) for i, (v, g) in enumerate(zip(vs, out)) for m in (check_result(S, op, v, g),) if m]
    if not bad:
        return None
    i, m = bad[0]
    show = lambda slots: None if slots is None else [[hex(w) for w in s] for s in slots]
    return "%s op %d (steps %d): %d of %d fail, first at %d (%s): %s\n  p = %s\n  q = %s\n  got = %s" % (
        S.name, op & 0xFF, op >> 8, len(bad), len(vs), i, vs[i].tag, m, show(vs[i].p), show(vs[i].q), [hex(int(w)) for w in out[i]])


if __name__ == "__main__" and "--golden" in __import__("sys").argv:
    import hostcheck_lib
    table = {}
    for name in CURVES:
        S = get_set(name)
        table[name] = {}
        for op, vs in sorted(vectors(name)[0].items()):
            P, Q = arrays(S, vs)
            out = hostcheck_lib.point_raw(S.c.cid, op, P, Q)
            assert first_failure(S, op, vs, out) is None
            table[name][str(op)] = digest(out)
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
elif __name__ == "__main__":                             # the table of profiles/point_vectors/coverage.txt
    print("tests/point_vectors.py: candidates against accepted vectors and the coverage events reached, per parameter set")
    print("(A, B, C: operands; a candidate is dropped only where x is off the curve or a Jacobian / XYZZ slot has no root)\n")
    for name in CURVES:
        ev = check_coverage(name)
        S = get_set(name)
        print("%s  NL %d  B %d  LB %#x  TOP1 %s  JTV %d  JV %d" % (name, S.nl, S.b, S.LB, S.TOP1, S.JTV, S.JV))
        print("  family A %d / %d   B %d / %d   C %d / %d   (accepted / candidates)" % (
            ev["A acc"], ev["A cand"], ev["B acc"], ev["B cand"], ev["C acc"], ev["C cand"]))
        print("  vectors per op: " + "  ".join("%d%s: %d" % (op & 0xFF, "x%d" % (op >> 8) if op >> 8 else "", ev["op %d n" % op])
                                                for op in sorted(vectors(name)[0], key=lambda o: (o & 0xFF, o >> 8))))
        for k in sorted(k for k in ev if " slot " in k):
            print("  %-12s %s" % (k, ev[k]))
        print("  V = JV reached: %s   D relations on add / add_mixed / the chain: %d, each identity spelling through dbl, ct_dbl4, is_identity\n" % (
            ev["V = JV"], ev["D relations"]))
