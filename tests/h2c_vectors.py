"""Adversarial inputs for the hash-to-curve lanes of csrc/ecgpu_h2c.h, shared by tests/test_h2c_vectors.py (the g++ twin, with and
without -DECGPU_BOUNDS_CHECK) and tests/test_gpu_h2c_vectors.py (gfx950).  Plain module: deterministic, seeded per curve; every
expected value is a Python integer (`int.from_bytes(okm, "big") % m`) or comes from tests/h2c_model.py, and every comparison is exact.

Four families per suite (k256, p256, p384):
  R  OKM for h2c_reduce_field / h2c_reduce_scalar, which otherwise only ever see a digest: the 24-byte pieces the Horner steps
     cut, chosen one by one; k m + d; results steered onto every structured residue; the LAST addition steered onto m - 1, m, m + 1
     (the wrap of SignScalar::add and the same place in mul2) and, where the modulus allows it, past 2^(32 N) (the carry out of the
     words); the middle step of the 72-byte form steered the same way.
  U  u for the map: structured limbs (and, for the Montgomery sets, their images s R^-1, structured AFTER from_canonical),
     u = +-sqrt(t / Z) so that tv1 = Z u^2 is the structured t, u with tv2 = tv1^2 + tv1 steered onto t the same way, the nine
     special u, random ones.
  P  colliding pairs.  For u != 0, v = (Z u)^-1 has tv1(v) = 1 / tv1(u), and x2(tv1) = x1(1 / tv1): both map to the same x with
     different xd (and different isogeny denominators), so map(v) = +-map(u) in ANOTHER projective representation.  (u, +-v)
     drives the complete addition through its doubling case and through the identity with unequal Z.
  I  (k256) inputs of the isogeny as fractions (xn, xd, y): the forged double root x0 of x_den, honest points of E' scaled by
     lambda, the other rational roots of y_den (or the proof that there is none), x' = 0, y = 0, structured xn.

A class that cannot exist for a suite is shown not to exist by an assertion here, not by an empty loop.  Nothing is dropped by
try / skip; `check_coverage` asserts the families' sizes and that they reach their stated targets."""
import itertools
import random

import field_vectors as fv
import h2c_model as hm
import pyec

CURVES = ["k256", "p256", "p384"]
PIECE = 1 << 192
PIECE_PATTERNS = (0, 1, 1 << 191, PIECE - 2, PIECE - 1)
LAST_PIECES = (0, 1, PIECE - 1)
R_CLASSES_48 = ("pieces", "multiple", "steered", "last step", "random")       # and "carry" where carry_possible
R_CLASSES_72 = R_CLASSES_48 + ("middle step",)

_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def modulus(name, which):
    c = pyec.CURVES[name]
    return c.p if which == "p" else c.n


def targets(name, which):
    """the structured residues: the field's limb layout for p, 32-bit words for n (family N of tests/field_vectors.py)"""
    c = pyec.CURVES[name]
    if which == "p":
        lay = fv.layout(name)
        return fv.structured(lay.b, lay.nl, c.L, c.p, c.p)
    return fv.structured(32, (8 * c.L + 31) // 32, c.L, c.n, c.n)


def horner(okm, m):
    """the accumulator after each step of the kernels' reduction (the model of WHERE a row aims, not of the code): piece 0, then
    (acc 2^192 + piece) mod m"""
    acc, trail = 0, []
    for j in range(0, len(okm), 24):
        acc = (acc * PIECE + int.from_bytes(okm[j:j + 24], "big")) % m
        trail.append(acc)
    return trail


# ---- family R -----------------------------------------------------------------------------------------------------------------
def family_r(name, which):
    """[(class, OKM of L bytes, the residue)] for m = p (which == "p") or n"""
    return _once(("R", name, which), lambda: _family_r(name, which))


def _family_r(name, which):
    s = hm.SUITES[name]
    L, m = s.L, modulus(name, which)
    W = 1 << (8 * L)
    pieces = L // 24
    assert L % 24 == 0 and pieces in (2, 3) and PIECE < m < W
    rng = random.Random("h2c-R-%s-%s" % (name, which))
    rows = []

    def put(cls, v):
        assert 0 <= v < W, (cls, v)
        rows.append((cls, v.to_bytes(L, "big"), v % m))

    for combo in itertools.product(PIECE_PATTERNS, repeat=pieces):
        put("pieces", sum(d << (192 * (pieces - 1 - j)) for j, d in enumerate(combo)))
    kmax = (W - 1) // m
    ks = {0, 1, 2, kmax, kmax - 1} | {rng.randrange(kmax + 1) for _ in range(16)}
    i = 0
    while (1 << (32 * i)) <= kmax:
        ks.add(1 << (32 * i))
        i += 1
    for k in sorted(ks):
        for d in (-1, 0, 1):
            if 0 <= k * m + d < W:
                put("multiple", k * m + d)
    for t in targets(name, which):
        kt = (W - 1 - t) // m
        put("steered", t + rng.randrange(kt + 1) * m)
        put("steered", t + kt * m)
    # the last addition: acc 2^192 = m - r, the last piece r - 1, r, r + 1
    spread = [1, 2, 3, 5, kmax] + [rng.randrange(1, kmax + 1) for _ in range(8)]
    spread += [rng.getrandbits(b) | 1 << (b - 1) for b in range(8, kmax.bit_length(), max(1, kmax.bit_length() // 12))]
    spread += [1 << b for b in range(4, kmax.bit_length(), 16)]
    for k in spread:
        assert 1 <= k <= kmax
        d_hi, r = divmod(k * m, PIECE)
        if r == 0:                                           # (2^192 divides k: there is no r - 1, and the step lands on 0)
            continue
        assert r < m
        for last in (r - 1, r, r + 1):
            if not 0 <= last < PIECE:
                continue
            v = d_hi * PIECE + last
            okm = v.to_bytes(L, "big")
            before = horner(okm[:-24], m)[-1] * PIECE % m
            assert before == m - r and before + last == m + (last - r) and v % m == (last - r) % m, (name, which, k)
            put("last step", v)
    for lead, last in carry_rows(name, which, rng):
        put("carry", lead * PIECE + last)
    if pieces == 3:
        for lead in (m - 1, m, m + 1, (1 << 384) - 1, 0, 1):
            assert 0 <= lead < (1 << 384)
            for last in LAST_PIECES:
                put("middle step", lead * PIECE + last)
    for _ in range(64):
        put("random", rng.getrandbits(8 * L))
    return rows


def carry_possible(name, which):
    """whether the last addition t + w (t below m, w below 2^192) can leave the words of the modulus at all"""
    return modulus(name, which) + PIECE - 2 >= 1 << (8 * pyec.CURVES[name].L)


def _gauss(b1, b2):
    """a reduced basis of the plane lattice spanned by b1, b2 (Lagrange's reduction)"""
    n2 = lambda v: v[0] * v[0] + v[1] * v[1]
    while True:
        if n2(b2) < n2(b1):
            b1, b2 = b2, b1
        mu = (2 * (b1[0] * b2[0] + b1[1] * b2[1]) + n2(b1)) // (2 * n2(b1))
        if mu == 0:
            return b1, b2
        b2 = (b2[0] - mu * b1[0], b2[1] - mu * b1[1])


def carry_rows(name, which, rng):
    """(leading pieces, last piece): the accumulator times 2^192 is t = m - s with s so small that t + w reaches 2^(32 N) for a
    w below 2^192 — the `carry != 0` half of SignScalar::add's select, which a sum that merely lands on m never sets.  Last pieces:
    the sum is 2^(32 N) - 1 (no carry, all ones), 2^(32 N) exactly (carry, zero words) and t + 2^192 - 1.  Where m lies below
    2^(32 N) - 2^192 (p256: both moduli) no such sum exists, which `carry_possible` states and `check_coverage` asserts.
    72 bytes: the two leading pieces hold t 2^-192 mod m itself.  48 bytes: the one leading piece d has only 192 bits, so (d, s) with
    d 2^192 = -s (mod m) and both below 2^192 is a short vector of the lattice {(d, s): d = -s 2^-192 mod m}, of determinant m."""
    if not carry_possible(name, which):
        return []
    m, F = modulus(name, which), pyec.CURVES[name].L
    top = 1 << (8 * F)
    smax = m - top + PIECE - 1                               # t + (2^192 - 1) >= 2^(32 N)  <=>  s <= smax
    assert 0 < smax < PIECE
    inv = pow(PIECE, -1, m)
    if hm.SUITES[name].L == 72:
        found = [((m - s) * inv % m, s) for s in (1, 2, smax, smax - 1) + tuple(rng.randrange(1, smax) for _ in range(4))]
    else:
        b1, b2 = _gauss((m, 0), ((-inv) % m, 1))
        found = []
        for a in range(-6, 7):
            for b in range(-6, 7):
                d, sv = a * b1[0] + b * b2[0], a * b1[1] + b * b2[1]
                if 0 < d < PIECE and 0 < sv <= smax:
                    found.append((d, sv))
        assert len(found) >= 4, (name, which, len(found))
        found = found[:8]
    out = []
    for lead, sv in found:
        t = lead * PIECE % m
        assert t == m - sv and top - t <= PIECE - 1
        for last in (top - t - 1, top - t, PIECE - 1):
            assert 0 <= last < PIECE
            out.append((lead, last))
    return out


# ---- family U -----------------------------------------------------------------------------------------------------------------
def _is_square(a, p):
    return pow(a % p, (p - 1) // 2, p) in (0, 1)


def tv3_zero_u(name):
    """the u with tv2 + 1 = tv1^2 + tv1 + 1 = 0 (tv3 = 0, x1 = 0): tv1 = Z u^2 would be a primitive cube root of unity w with w / Z
    a square.  None exists for any of the three suites: p384 has no such root (p = 2 mod 3), and on k256 and p256 neither root
    gives a square w / Z.  Asserted, so that a new suite cannot pass this by silently."""
    s = hm.SUITES[name]
    p, Z = s.curve.p, s.Z % s.curve.p
    if p % 3 == 2:
        assert pyec.sqrt_mod(p - 3, p) is None               # -3 is a non-residue: x^2 + x + 1 has no root
        return []
    r = pyec.sqrt_mod(p - 3, p)
    assert r is not None and r * r % p == p - 3
    out = []
    for w in ((-1 + r) * pow(2, -1, p) % p, (-1 - r) * pow(2, -1, p) % p):
        assert (w * w + w + 1) % p == 0
        t = w * pow(Z, -1, p) % p
        if _is_square(t, p):
            u = pyec.sqrt_mod(t, p)
            out += [u, p - u]
    assert out == [], (name, out)
    return out


def family_u(name):
    """[(class, u)], every u below p"""
    return _once(("U", name), lambda: _family_u(name))


def _family_u(name):
    s = hm.SUITES[name]
    c = s.curve
    p, Z = c.p, s.Z % c.p
    lay = fv.layout(name)
    rng = random.Random("h2c-U-" + name)
    S = fv.structured(lay.b, lay.nl, c.L, p, p)
    rows = [("structured", t) for t in S]
    ts = list(S)
    if lay.mont:
        ri = pow(1 << (lay.nl * lay.b), -1, p)
        mont = [t * ri % p for t in S]
        rows += [("montgomery", t) for t in mont]
        ts += mont
    zi = pow(Z, -1, p)
    for t in ts:                                            # tv1 = Z u^2 = t enters sqr / add with structured limbs
        if t and _is_square(t * zi, p):
            u = pyec.sqrt_mod(t * zi % p, p)
            assert u is not None and Z * u * u % p == t
            rows += [("tv1", u), ("tv1", p - u)]
    i2 = pow(2, -1, p)
    for t in ts:                                            # tv2 = tv1^2 + tv1 = t: what is_zero sees after its normalisation
        r = pyec.sqrt_mod((1 + 4 * t) % p, p) if t else None
        for tv1 in ([] if r is None else sorted({(r - 1) * i2 % p, (-r - 1) * i2 % p})):
            assert (tv1 * tv1 + tv1) % p == t
            if tv1 and _is_square(tv1 * zi, p):
                u = pyec.sqrt_mod(tv1 * zi % p, p)
                rows += [("tv2", u), ("tv2", p - u)]
    rows += [("tv3 = 0", u) for u in tv3_zero_u(name)]
    rows += [("special", u) for u in hm.special_u(s).values()]
    rows += [("random", rng.randrange(p)) for _ in range(32)]
    assert all(0 <= u < p for _, u in rows)
    return rows


# ---- family P -----------------------------------------------------------------------------------------------------------------
def collide(s, u, model_map=hm.map_to_curve):
    """(v_same, v_opp) of u != 0: v = (Z u)^-1 and p - v, sorted by the model into map(v) == map(u) and map(v) == -map(u)"""
    c = s.curve
    p, Z = c.p, s.Z % c.p
    v = pow(Z * u % p, -1, p)
    Q = model_map(s, u)
    assert Q is not pyec.INF
    same = [w for w in (v, p - v) if model_map(s, w) == Q]
    opp = [w for w in (v, p - v) if model_map(s, w) == pyec.neg(c, Q)]
    assert len(same) == 1 and len(opp) == 1, (c.name, u)
    return same[0], opp[0]


def family_p(name, model_map=hm.map_to_curve):
    """[(u0, u1, expected sum, collapsed?)]: (u, v_same), (v_same, u) -> 2 map(u); (u, v_opp), (v_opp, u) -> the identity.
    collapsed: u = +-sqrt(-1 / Z), where Z u^2 = -1 makes v = -u, so that v_same is u itself (the row stays: it is the (u, u) and
    (u, -u) of the existing tests, the one place where both summands DO share their representation)."""
    return _once(("P", name), lambda: _family_p(name, model_map))


def _family_p(name, model_map):
    s = hm.SUITES[name]
    c = s.curve
    p, Z = c.p, s.Z % c.p
    rng = random.Random("h2c-P-" + name)
    special = [u for u in hm.special_u(s).values() if u]
    assert len(special) == 8
    # (tv1 = p - 1 is a structured target, so family U holds +-sqrt(-1 / Z) outside its special class too: they are in `special`)
    from_u = rng.sample(sorted({u for cls, u in family_u(name) if u and cls != "special" and Z * u * u % p != p - 1}), 16)
    us = [rng.randrange(1, p) for _ in range(16)] + special + from_u
    root = pyec.sqrt_mod((-pow(Z, -1, p)) % p, p)
    rows = []
    for u in us:
        same, opp = collide(s, u, model_map)
        collapsed = u in (root, p - root)
        assert collapsed == (same == u) and collapsed == (Z * u * u % p == p - 1), (name, u)
        if not collapsed:                                   # tv1(v) = 1 / tv1(u) != tv1(u): another xd, another representation
            assert (Z * same * same % p) * (Z * u * u % p) % p == 1 and Z * same * same % p != Z * u * u % p
        Q = model_map(s, u)
        dbl = pyec.add(c, Q, Q)
        assert dbl is not pyec.INF and pyec.on_curve(c, dbl)
        rows += [(u, same, dbl, collapsed), (same, u, dbl, collapsed), (u, opp, pyec.INF, collapsed), (opp, u, pyec.INF, collapsed)]
    return rows


# ---- family I (k256) ----------------------------------------------------------------------------------------------------------
def k256_x0():
    """the double root of x_den, also a root of y_den, on no point of E'"""
    p = pyec.K256.p
    x0 = (-hm.K256_ISO_XDEN[1]) * pow(2, -1, p) % p
    assert hm._poly(hm.K256_ISO_XDEN, x0, p) == 0 and hm._poly(hm.K256_ISO_YDEN, x0, p) == 0
    assert not _is_square(pow(x0, 3, p) + hm.K256_ISO_A * x0 + hm.K256_ISO_B, p)
    return x0


def k256_yden_other_roots():
    """the rational roots of y_den other than x0: y_den = (x - x0) (x^2 + b x + c), the quadratic solved by pyec.sqrt_mod"""
    p = pyec.K256.p
    x0 = k256_x0()
    k0, k1, k2, k3 = hm.K256_ISO_YDEN
    assert k3 == 1
    b = (k2 + x0) % p                                        # synthetic division by (x - x0)
    c = (k1 + x0 * b) % p
    assert (k0 + x0 * c) % p == 0
    r = pyec.sqrt_mod((b * b - 4 * c) % p, p)
    if r is None:
        return []
    roots = sorted({(-b + r) * pow(2, -1, p) % p, (-b - r) * pow(2, -1, p) % p})
    assert all(hm._poly(hm.K256_ISO_YDEN, x, p) == 0 for x in roots)
    return [x for x in roots if x != x0]


def iso_model(xn, xd, y):
    """the isogeny as a rational map on x' = xn / xd, y' = y (the point need not be on E'): an affine point or pyec.INF"""
    p = pyec.K256.p
    assert xd % p
    return hm.k256_isogeny((xn * pow(xd, -1, p) % p, y % p))


def family_i(name):
    """[(class, xn, xd, y, expected)] for k256; no other suite has an isogeny"""
    if name != "k256":
        assert hm.SUITES[name].map_a % hm.SUITES[name].curve.p == hm.SUITES[name].curve.a % hm.SUITES[name].curve.p
        return []
    return _once(("I", name), _family_i)


def _family_i():
    s = hm.SUITES["k256"]
    p = s.curve.p
    lay = fv.layout("k256")
    rng = random.Random("h2c-I-k256")
    x0 = k256_x0()
    lams = [1, 2, p - 1] + [1 << (lay.b * i) for i in range(1, lay.nl)] + [1 << (32 * i) for i in range(1, 8)]
    lams += [rng.randrange(1, p) for _ in range(8)]
    rows = []

    def put(cls, xn, xd, y):
        rows.append((cls, xn % p, xd % p, y % p, iso_model(xn, xd, y)))

    for lam in lams:
        put("forged", x0 * lam, lam, rng.randrange(p))
        x, y = hm.sswu(s, rng.randrange(p))
        put("honest", x * lam, lam, y)
    others = k256_yden_other_roots()
    for x in others:                                         # a root of y_den alone: the kernel's rule gives the identity there too
        for lam in (1, lams[-1]):
            put("y_den root", x * lam, lam, rng.randrange(p))
    x, y = hm.sswu(s, rng.randrange(p))
    put("x' = 0", 0, 1, y)
    put("x' = 0", 0, lams[-1], 0)
    put("y = 0", x, 1, 0)
    put("y = 0", x * lams[-2], lams[-2], 0)
    for t in fv.structured(lay.b, lay.nl, 32, p, p):
        put("structured", t, 1, rng.randrange(p))
    assert all((want is pyec.INF) == (cls in ("forged", "y_den root")) for cls, _, _, _, want in rows)
    return rows


# ---- coverage -----------------------------------------------------------------------------------------------------------------
def check_coverage(name):
    """every family is there for the suite and reaches what it says it reaches"""
    s = hm.SUITES[name]
    c = s.curve
    p, Z = c.p, s.Z % c.p
    pieces = s.L // 24
    for which in ("p", "n"):
        m = modulus(name, which)
        rows = family_r(name, which)
        by = {}
        for cls, okm, want in rows:
            assert len(okm) == s.L and want == int.from_bytes(okm, "big") % m
            by.setdefault(cls, []).append((okm, want))
        want_cls = set(R_CLASSES_72 if pieces == 3 else R_CLASSES_48) | ({"carry"} if carry_possible(name, which) else set())
        assert set(by) == want_cls, (name, which, tuple(by))
        assert carry_possible(name, which) == (name != "p256")
        if carry_possible(name, which):
            top = 1 << (8 * c.L)
            sums = [horner(o, m)[-2] * PIECE % m + int.from_bytes(o[-24:], "big") for o, _ in by["carry"]]
            assert top - 1 in sums and top in sums and sum(1 for v in sums if v > top) >= 4 and len(sums) >= 12
        assert len(by["pieces"]) == 5 ** pieces and len(by["random"]) == 64
        assert bytes(s.L) in [o for o, _ in by["pieces"]] and b"\xff" * s.L in [o for o, _ in by["pieces"]]
        vals = {int.from_bytes(o, "big") for o, _ in by["multiple"]}
        kmax = ((1 << (8 * s.L)) - 1) // m
        assert {0, 1, m - 1, m, m + 1, 2 * m, kmax * m, (kmax - 1) * m, kmax * m - 1} <= vals and len(vals) >= 3 * 20
        assert {w for _, w in by["steered"]} == set(targets(name, which)) and len(by["steered"]) == 2 * len(targets(name, which))
        assert {w for _, w in by["last step"]} == {m - 1, 0, 1} and len(by["last step"]) >= 3 * 16
        # both shapes of the leading pieces: full ones, and (72 bytes) a zero piece first for the k with k m below 2^384
        assert any(o[0] & 0x80 for o, _ in by["last step"])
        assert any(o[:24] == bytes(24) for o, _ in by["last step"]) == (pieces == 3)
        if pieces == 3:
            assert len(by["middle step"]) == 18
            mids = {horner(o, m)[1] for o, _ in by["middle step"]}
            assert {0, 1, m - 1} <= mids                     # the accumulator after the middle step
        lands = {horner(o, m)[-2] * PIECE % m + int.from_bytes(o[-24:], "big") for o, _ in by["last step"]}
        assert lands == {m - 1, m, m + 1}
    lay = fv.layout(name)
    rows = family_u(name)
    by = {}
    for cls, u in rows:
        by.setdefault(cls, []).append(u)
    want_cls = ("structured",) + (("montgomery",) if lay.mont else ()) + ("tv1", "tv2", "special", "random")
    assert tuple(by) == want_cls, (name, tuple(by))
    assert lay.mont == (name != "k256")
    S = fv.structured(lay.b, lay.nl, c.L, p, p)
    full = (1 << (lay.b * lay.nl)) - 1
    assert by["structured"] == S and {0, 1, p - 1, p - 2} <= set(S) and any(t & full == t and bin(t).count("1") >= lay.b * (lay.nl - 1) for t in S)
    assert len(by["special"]) == 9 and len(by["random"]) == 32
    tv1s = {Z * u * u % p for u in by["tv1"]}
    reach = set(S) | ({t * pow(1 << (lay.nl * lay.b), -1, p) % p for t in S} if lay.mont else set())
    assert tv1s == {t for t in reach if t and _is_square(t * pow(Z, -1, p), p)} and len(by["tv1"]) == 2 * len(tv1s)
    assert len(tv1s) >= len(reach) // 3                      # about half of the targets are reachable
    tv2s = {(Z * u * u) ** 2 % p + Z * u * u % p for u in by["tv2"]}
    tv2s = {t % p for t in tv2s}
    assert tv2s <= reach and len(tv2s) >= len(reach) // 3 and 0 not in tv2s
    assert tv3_zero_u(name) == []
    rows = family_p(name)
    assert len(rows) == 4 * 40
    assert sum(1 for r in rows if r[3]) == 4 * 2             # +-sqrt(-1 / Z) of special_u, nothing else
    assert sum(1 for r in rows if r[2] is pyec.INF) == len(rows) // 2
    rows = family_i(name)
    if name == "k256":
        by = {}
        for r in rows:
            by.setdefault(r[0], []).append(r)
        need = ("forged", "honest", "x' = 0", "y = 0", "structured") + (("y_den root",) if k256_yden_other_roots() else ())
        assert set(by) == set(need), set(by)
        assert len(by["forged"]) == len(by["honest"]) >= 26 and all(r[4] is pyec.INF for r in by["forged"])
        assert (k256_x0(), 1) in [(r[1], r[2]) for r in by["forged"]]
        assert all(r[4] is not pyec.INF and pyec.on_curve(c, r[4]) for r in by["honest"])
    else:
        assert rows == []
