"""Adversarial limb-level vectors for Field<C> and ScalarN<C>, shared by tests/test_field_adversarial.py (the g++ twin) and
tests/test_gpu_field_adversarial.py (gfx950).  Plain module: deterministic, seeded per curve id; every expected value is a
Python integer and every comparison is exact.

Three families per parameter set (all twelve):
  C  canonical domain, the existing self-test ops 0 1 2 3 4 5 7 8 9 13 14 17.  Operands: the structured integers S below p AND
     s * R^-1 mod p for each of them — the second half is what arrives in the Montgomery domain as structured LIMBS (from_canonical
     multiplies by R^2).  Pairs: a fixed stride, and result-steered pairs (a * b, a + b, a - b land on every structured target).
  R  raw domain, ops 30 - 39 (csrc/ecgpu_selftest_raw.h): operands enter through Field::unpack, so values in [p, 2p) and limbs of
     all ones reach the reductions as written, scaled to the magnitude limits (MAXPROD, MAXMAG, SQLIM) by repeated addition.
  N  ScalarN<C>, ops 40 - 44: structured 32-bit words mod n, each also times R_n^+-1, products steered to every target,
     reduce_wire on k n - 1, k n, k n + 1 for every k that fits the wire, is_high around (n - 1) / 2.

The limb layouts are stated here and asserted against csrc/ecgpu_field_consts.h (and the k256 limits against ecgpu_field.h), so a
changed layout cannot leave the vectors aiming at the old one.  The generator asserts its own coverage (`check_coverage`); nothing
is dropped by try / skip: a vector the big-integer reference cannot evaluate is a bug here."""
import os
import random
import re
from collections import namedtuple

import pyec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")

CURVES = ["k256", "p256", "p384", "sm2", "p224", "p192", "p521", "bp256", "bp384", "bp256t1", "bp384t1", "bign256"]

# name -> (header struct, limbs, bits per limb, Montgomery form)
STATED = {"k256": ("K256U", 9, 29, False), "p256": ("P256U", 10, 28, True), "sm2": ("SM2U", 10, 28, True),
          "bp256": ("BP256U", 10, 28, True), "bp256t1": ("BP256T1U", 10, 28, True), "bign256": ("BIGN256U", 10, 28, True),
          "p384": ("P384U", 15, 27, True), "bp384": ("BP384U", 15, 27, True), "bp384t1": ("BP384T1U", 15, 27, True),
          "p224": ("P224U", 9, 27, True), "p192": ("P192U", 8, 26, True), "p521": ("P521U", 20, 27, True)}

Layout = namedtuple("Layout", "nl b mont maxprod maxmag sqlim")

C_BINARY_OPS = (0, 1, 2, 8, 9, 13, 14)
C_UNARY_OPS = (3, 4, 5, 7, 17)
R_OPS = tuple(range(30, 40))
N_OPS = (40, 41, 42, 43, 44)
# the CPU twin's scalar_op number of each device op
N_OP_TO_HOSTCHECK = {40: 0, 41: 1, 42: 2, 43: 3, 44: 4}

_layouts = {}


def layout(name):
    """(NL, B, Montgomery?, MAXPROD, MAXMAG, SQLIM) of a parameter set, read from the headers and checked against STATED."""
    if name in _layouts:
        return _layouts[name]
    struct, nl, b, mont = STATED[name]
    src = open(os.path.join(CSRC, "ecgpu_field_consts.h")).read()
    start = re.search(r"struct %s\b[^{]*\{" % struct, src).end()
    head = src[start: start + 400]
    got = {k: int(v) for k, v in re.findall(r"\b(NL|B|MAXPROD|MAXMAG)\s*=\s*(\d+)", head)}
    assert (got["NL"], got["B"]) == (nl, b), (name, got)
    if mont:
        mp, mm = got["MAXPROD"], got["MAXMAG"]
    else:
        fsrc = open(os.path.join(CSRC, "ecgpu_field.h")).read()
        mp = int(re.search(r"int MAXPROD = REPR == REPR_U29_K256 \? (\d+) :", fsrc).group(1))
        mm = int(re.search(r"int MAXMAG = REPR == REPR_U29_K256 \? (\d+) :", fsrc).group(1))
    fsrc = open(os.path.join(CSRC, "ecgpu_field.h")).read()
    assert "SQLIM = MAXPROD >= 49 ? 7 : (MAXPROD >= 16 ? 4 : (MAXPROD >= 4 ? 2 : 1))" in fsrc
    sq = 7 if mp >= 49 else 4 if mp >= 16 else 2 if mp >= 4 else 1
    _layouts[name] = Layout(nl, b, mont, mp, mm, sq)
    return _layouts[name]


def enc(c, vals):
    return b"".join(v.to_bytes(c.L, c.order) for v in vals)


def dec(c, data):
    data = bytes(data)
    return [int.from_bytes(data[i: i + c.L], c.order) for i in range(0, len(data), c.L)]


def structured(bits, nl, wire_bytes, modulus, lim):
    """The structured integers: limbs of `bits` bits, `nl` of them, `wire_bytes` on the wire, around `modulus`, below `lim`.
    Sorted, distinct."""
    mask = (1 << bits) - 1
    full = (1 << (bits * nl)) - 1
    base = [full]
    base += [full ^ (mask << (bits * i)) for i in range(nl)]                         # one limb cleared
    base += [mask << (bits * i) for i in range(nl)]                                  # a single limb set
    for i in range(nl + 1):
        base += [1 << (bits * i), (1 << (bits * i)) - 1, (1 << (bits * i)) + 1]
    base += [sum((mask if i % 2 else 0) << (bits * i) for i in range(nl)), sum((0 if i % 2 else mask) << (bits * i) for i in range(nl))]
    for i in range((8 * wire_bytes + 31) // 32 + 1):
        base += [1 << (32 * i), (1 << (32 * i)) - 1]
    base += [0, 1, 2, 3, lim - 1, lim - 2]
    base += [modulus + d for d in range(-2, 3)]
    base += [modulus // 2 + d for d in range(-3, 4)]
    # what does not fit below lim as it stands also enters with its top limb cut to the largest (and second largest) that fits:
    # all the low limbs as written, the value just below lim
    top_w = bits * (nl - 1)
    top = (lim - 1) >> top_w
    for v in list(base):
        if v >= lim:
            low = v & ((1 << top_w) - 1)
            base += [low + (top << top_w), low + ((top - 1) << top_w)]
    out = set()
    for v in base:
        for d in (-1, 0, 1):
            if 0 <= v + d < lim:
                out.add(v + d)
    return sorted(out)


# ---- family C -----------------------------------------------------------------------------------------------------------------

def _c_want(op, a, b, p):
    if op == 0: return (a + b) % p
    if op == 1: return (a - b) % p
    if op == 2: return a * b % p
    if op == 3: return a * a % p
    if op in (4, 17): return pow(a, -1, p) if a else 0
    if op == 5: return (-a) % p
    if op == 7: return 2 * a % p
    if op == 8: return (2 * a + b) % p
    if op == 9: return (-b * b) % p
    if op == 13: return (a * b - 2 * a - b) % p
    if op == 14: return ((a + b) ** 2 - 5 * b) % p
    raise AssertionError(op)


def family_c(name):
    """{op: (a values, b values or None, expected)} in the canonical domain (every value below p)."""
    c = pyec.CURVES[name]
    lay = layout(name)
    p = c.p
    rng = random.Random(0xC0FFEE + c.cid)
    ri = pow(1 << (lay.nl * lay.b), -1, p) if lay.mont else 1
    s = structured(lay.b, lay.nl, c.L, p, p)
    ops = s + [t * ri % p for t in s]
    cases = {op: ([], [], []) for op in C_BINARY_OPS}

    def put(op, a, b):
        A, B, W = cases[op]
        A.append(a)
        B.append(b)
        W.append(_c_want(op, a, b, p))
    for i, a in enumerate(ops):
        b = ops[(7 * i + 3) % len(ops)]
        for op in C_BINARY_OPS:
            put(op, a, b)
    # result-steered pairs: the product, the sum and the difference land on every structured target
    for t in ops:
        for a in rng.sample(ops, 4) + [rng.randrange(1, p) for _ in range(3)]:
            if a == 0:
                a = 1
            put(2, a, t * pow(a, -1, p) % p)
            put(0, a, (t - a) % p)
            put(1, a, (a - t) % p)
    for op in (0, 1, 2):
        A, B, W = cases[op]
        steered = len(A) - len(ops)
        assert steered == 7 * len(ops)
    out = {op: (A, B, W) for op, (A, B, W) in cases.items()}
    inv_shapes = [rng.randrange(2 ** k) % p for k in range(1, 8 * c.L, 5)] + [2 ** k % p for k in range(0, 8 * c.L, 29)]
    for op in C_UNARY_OPS:
        vals = ops + (inv_shapes if op in (4, 17) else [])
        out[op] = (vals, None, [_c_want(op, a, None, p) for a in vals])
    return out


def c_binary_count(fam):
    return sum(len(fam[op][0]) for op in C_BINARY_OPS)


# ---- family R -----------------------------------------------------------------------------------------------------------------

def raw_lim(name):
    c = pyec.CURVES[name]
    return min(2 * c.p, 1 << (8 * c.L)) if layout(name).mont else 1 << 256


def r_want(name, op, a, b):
    """Expected value of raw-domain op 30 - 39 on the integers a, b (below raw_lim; they may exceed p)."""
    c = pyec.CURVES[name]
    lay = layout(name)
    p = c.p
    ri = pow(1 << (lay.nl * lay.b), -1, p) if lay.mont else 1
    mp, mm, sq = lay.maxprod, lay.maxmag, lay.sqlim
    a1 = min(mp, mm)
    b1 = mp // a1
    a2 = 5 if mp >= 25 else 4 if mp >= 16 else 3 if mp >= 9 else 2
    b2 = mp // a2
    s = 6 if lay.mont else 3
    if op == 30: return a1 * b1 * a * b * ri % p
    if op == 31: return a2 * b2 * a * b * ri % p
    if op == 32: return (sq * a) ** 2 * ri % p
    if op == 33: return a * b * ri % p
    if op == 34: return (a2 * b2 * a * b * ri - 6 * b) % p
    if op == 35: return ((sq * a) ** 2 * ri - 6 * b) % p
    if op == 36: return (a2 * (b2 // 2) + a2 * (b2 - b2 // 2)) * a * b * ri % p
    if op == 37: return (s * a - s * b) % p
    if op == 38: return a * ri % p
    if op == 39: return 1 if a % p == 0 else 0
    raise AssertionError(op)


def r_pairs(name):
    """Raw-domain operand pairs: every structured s with six others, with itself and with every 2^(B i) (a one-limb operand
    leaves the low product columns zero: the u = 0 rows of the reductions), then 300 random pairs below the limit."""
    c = pyec.CURVES[name]
    lay = layout(name)
    lim = raw_lim(name)
    rng = random.Random(0x4A77 + c.cid)
    s = structured(lay.b, lay.nl, c.L, c.p, lim)
    pairs = []
    for a in s:
        pairs += [(a, b) for b in rng.sample(s, 6)]
        pairs.append((a, a))
    for i in range(lay.nl):
        one_limb = 1 << (lay.b * i)
        assert one_limb < lim
        for a in s:
            pairs.append((a, one_limb))
            pairs.append((one_limb, a))
    pairs += [(rng.randrange(lim), rng.randrange(lim)) for _ in range(300)]
    return pairs


def family_r(name):
    """{op: (a values, b values, expected)} for ops 30 - 39, all on the same pairs."""
    pairs = r_pairs(name)
    A = [a for a, _ in pairs]
    B = [b for _, b in pairs]
    return {op: (A, B, [r_want(name, op, a, b) for a, b in pairs]) for op in R_OPS}


# ---- family N -----------------------------------------------------------------------------------------------------------------

def n_operands(name):
    c = pyec.CURVES[name]
    n = c.n
    words = (8 * c.L + 31) // 32
    r = 1 << (32 * words)
    s = structured(32, words, c.L, n, n)
    return sorted(set(s + [t * pow(r, -1, n) % n for t in s] + [t * r % n for t in s]))


def family_n(name):
    """{op: (a values, b values or None, expected)} for the scalar ops 40 - 44.  Operands are below n, except reduce_wire's,
    which are any value the wire holds (they may exceed p where n > p: no canonical check of the field applies)."""
    c = pyec.CURVES[name]
    n = c.n
    rng = random.Random(0x5CA1A + c.cid)
    ops = n_operands(name)
    A, B, W = [], [], []
    for i, a in enumerate(ops):
        b = ops[(7 * i + 3) % len(ops)]
        A.append(a); B.append(b); W.append(a * b % n)
    for t in ops:                                                # products steered to every target
        for a in rng.sample(ops, 3) + [rng.randrange(1, n)]:
            if a == 0:
                a = n - 1
            A.append(a); B.append(t * pow(a, -1, n) % n); W.append(t)
    out = {40: (A, B, W),
           41: (ops, None, [pow(a, -1, n) if a else 0 for a in ops]),
           43: (ops, None, [1 if a > (n - 1) // 2 else 0 for a in ops]),
           44: (ops, None, list(ops))}
    wire = 1 << (8 * c.L)
    red = []
    k = 0
    while k * n - 1 < wire:
        red += [v for v in (k * n - 1, k * n, k * n + 1) if 0 <= v < wire]
        k += 1
    assert (wire - 1) // n == k - 1                              # every multiple of n the wire can hold was visited
    red += structured(32, (8 * c.L + 31) // 32, c.L, n, wire) + ops
    out[42] = (red, None, [v % n for v in red])
    return out


# ---- coverage -----------------------------------------------------------------------------------------------------------------

def check_coverage(name, fam_c=None, fam_r=None, fam_n=None):
    """The families' own minimum sizes (a refactoring must not thin them silently)."""
    if fam_c is not None:
        assert set(fam_c) == set(C_BINARY_OPS + C_UNARY_OPS)
        assert c_binary_count(fam_c) >= 5000, (name, c_binary_count(fam_c))
        assert all(len(a) == len(w) > 0 and (b is None or len(b) == len(a)) for a, b, w in fam_c.values())
    if fam_r is not None:
        assert set(fam_r) == set(R_OPS)
        assert all(len(a) == len(b) == len(w) >= 650 for a, b, w in fam_r.values()), name
        lim = raw_lim(name)
        p = pyec.CURVES[name].p
        A = fam_r[33][0]
        assert all(0 <= v < lim for v in A + fam_r[33][1])
        assert any(v >= p for v in A) and p in A and 0 in A       # the second representative, and both forms of zero
    if fam_n is not None:
        assert set(fam_n) == set(N_OPS)
        assert len(fam_n[41][0]) >= 90, (name, len(fam_n[41][0]))
        assert all(len(a) == len(w) > 0 and (b is None or len(b) == len(a)) for a, b, w in fam_n.values())
        if name == "p521":
            assert (1 << 528) - 1 in fam_n[42][0] and len(fam_n[42][0]) >= 386


def first_mismatch(c, op, fam_entry, got):
    """None, or a message with the first differing index, its operands and both values."""
    a, b, want = fam_entry
    assert len(got) == len(want), (c.name, op, len(got), len(want))
    if got == want:
        return None
    i = next(k for k in range(len(want)) if got[k] != want[k])
    bad = sum(1 for g, w in zip(got, want) if g != w)
    return "%s op %d: %d of %d differ, first at %d: a = %#x, b = %s, got %#x, want %#x" % (
        c.name, op, bad, len(want), i, a[i], "%#x" % b[i] if b is not None else "-", got[i], want[i])
