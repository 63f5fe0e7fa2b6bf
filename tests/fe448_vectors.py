"""Adversarial operands for csrc/ecgpu_fe448.h (p = 2^448 - 2^224 - 1, 16 limbs of 28 bits), in the spirit of tests/field_vectors.py:
produced once, used by the g++ twin (tests/test_hostcheck_x448.py, plain and -DECGPU_BOUNDS_CHECK) and by the device
(tests/test_gpu_fe448.py) alike.  A row is (label, a, b): lists of 16 raw limbs, b None for the ops of one operand.

Expected limbs come from model(op, a, b): the ops restated on Python integers — the columns of a product are computed from their
definition (L = a0 b0 + a1 b1, H = a0 b1 + a1 b0 + a1 b1) and never overflow here, so a 64-bit column that wraps in the C++ shows
as a difference — and value(result) is held against plain arithmetic mod p as well."""
import random

P = 2 ** 448 - 2 ** 224 - 1
NL, LB = 16, 28
MASK = (1 << LB) - 1
T = (1 << LB) + 256                                  # limb bound of a tight element
A24 = 39082
MUL, SQR, ADD, SUB, MUL_SMALL, CARRY, CANON, INVERT, BYTES = range(9)
OP_NAMES = ("mul", "sqr", "add", "sub", "mul_small", "carry", "canon", "invert", "bytes")
# the widest limbs each op accepts, as a multiple of T (carry: any 32-bit word; bytes: a 56-byte record)
ACCEPTS = {MUL: 2, SQR: 2, ADD: 1, SUB: 2, MUL_SMALL: 2, CANON: 15, INVERT: 1}
SPECIAL = {"p-1": P - 1, "p": P, "p+1": P + 1, "2^224-1": 2 ** 224 - 1, "2^224": 2 ** 224, "2^224+1": 2 ** 224 + 1,
           "2^448-1": 2 ** 448 - 1, "0": 0, "1": 1}


def limbs(v):
    """the limbs of v < 2^448 + (top limb may carry the excess of a value below 2^452)"""
    assert 0 <= v < 1 << (LB * NL + 4)
    out = [(v >> (LB * i)) & MASK for i in range(NL - 1)]
    return out + [v >> (LB * (NL - 1))]


def value(l):
    return sum(int(x) << (LB * i) for i, x in enumerate(l))


def p_limb(i):
    return MASK - 1 if i == 8 else MASK


# ---- the ops on Python integers, limb for limb -----------------------------------------------------------------------------------
def carry(a):
    top = a[NL - 1] >> LB
    r = [(a[i] & MASK) + (a[i - 1] >> LB) if i else (a[0] & MASK) + top for i in range(NL)]
    r[8] += top
    return r


def reduce_columns(c):
    r, acc = [], 0
    for j in range(NL):
        acc += c[j]
        r.append(acc & MASK)
        acc >>= LB
    lo, hi = r[0] + acc, r[8] + acc
    r[0], r[8] = lo & MASK, hi & MASK
    r[1] += lo >> LB
    r[9] += hi >> LB
    return r


def half_columns(x, y):
    c = [0] * 16
    for i in range(8):
        for j in range(8):
            c[i + j] += x[i] * y[j]
    return c


def product_columns(a, b):
    a0, a1, b0, b1 = a[:8], a[8:], b[:8], b[8:]
    L = [x + y for x, y in zip(half_columns(a0, b0), half_columns(a1, b1))]
    H = [x + y + z for x, y, z in zip(half_columns(a0, b1), half_columns(a1, b0), half_columns(a1, b1))]
    return [L[j] + H[8 + j] for j in range(8)] + [H[j] + L[8 + j] + H[8 + j] for j in range(8)]


def canon(a):
    return limbs(value(carry(a)) % P)


def model(op, a, b=None):
    b = b if b is not None else [0] * NL
    if op == MUL:
        return reduce_columns(product_columns(a, b))
    if op == SQR:
        return reduce_columns(product_columns(a, a))
    if op == ADD:
        return [x + y for x, y in zip(a, b)]
    if op == SUB:
        return carry([a[i] + 4 * p_limb(i) - b[i] for i in range(NL)])       # B = 2: 2B p
    if op == MUL_SMALL:
        return reduce_columns([x * A24 for x in a])
    if op == CARRY:
        return carry(a)
    if op == CANON:
        return canon(a)
    if op == INVERT:
        # the chain of ecgpu_fe448.h, on the same lazy limbs
        def sq(x, n):
            for _ in range(n):
                x = model(SQR, x)
            return x
        def mu(x, y):
            return model(MUL, x, y)
        x2 = mu(sq(a, 1), a); x3 = mu(sq(x2, 1), a); x6 = mu(sq(x3, 3), x3); x12 = mu(sq(x6, 6), x6); x24 = mu(sq(x12, 12), x12)
        x27 = mu(sq(x24, 3), x3); x54 = mu(sq(x27, 27), x27); x108 = mu(sq(x54, 54), x54); x111 = mu(sq(x108, 3), x3)
        x222 = mu(sq(x111, 111), x111); x223 = mu(sq(x222, 1), a)
        return mu(sq(mu(sq(x223, 223), x222), 2), a)
    if op == BYTES:
        v = sum(int(x) << (32 * i) for i, x in enumerate(a[:14]))
        c = v % P
        return [(c >> (32 * i)) & 0xFFFFFFFF for i in range(14)] + [0, 0]
    raise ValueError(op)


def expected_value(op, a, b=None):
    """what value(result) must be congruent to mod p (None: the op is not a map on residues)"""
    va, vb = value(a), value(b) if b is not None else 0
    return {MUL: va * vb, SQR: va * va, ADD: va + vb, SUB: va - vb, MUL_SMALL: A24 * va, CARRY: va, CANON: va,
            INVERT: pow(va % P, P - 2, P)}.get(op)


# ---- the rows ------------------------------------------------------------------------------------------------------------------
def _rand_limbs(rng, bound):
    return [rng.randrange(bound + 1) for _ in range(NL)]


def _second_rep(v):
    """v + p as raw limbs: a representative in [p, 2p)"""
    return limbs(v % P + P)


def _uncarry(l, where):
    """the same value with 2^28 moved down from limb where + 1 into limb where (a lazy form)"""
    l = list(l)
    if l[where + 1] > 0:
        l[where + 1] -= 1
        l[where] += 1 << LB
    return l


def _column_peak(k, bound):
    """operands whose plain 16 x 16 product has every term of column k at the bound, and nothing else"""
    a, b = [0] * NL, [0] * NL
    for i in range(NL):
        if 0 <= k - i < NL:
            a[i] = bound
            b[k - i] = bound
    return a, b


_cache = {}


def rows(op):
    if op in _cache:
        return _cache[op]
    rng = random.Random("fe448-vectors-%d" % op)
    out = []
    if op == BYTES:
        for name, v in SPECIAL.items():
            out.append((name, [(v >> (32 * i)) & 0xFFFFFFFF for i in range(14)] + [0, 0], None))
        for t in range(24):
            v = rng.getrandbits(448) if t % 2 else P + rng.getrandbits(rng.choice((1, 64, 223)))
            out.append(("random %d" % t, [(v >> (32 * i)) & 0xFFFFFFFF for i in range(14)] + [0, 0], None))
        _cache[op] = out
        return out
    bound = 0xFFFFFFFF if op == CARRY else ACCEPTS[op] * T
    two = op in (MUL, ADD, SUB)
    sp = {k: limbs(v) for k, v in SPECIAL.items()}

    def put(label, a, b=None):
        assert all(0 <= x <= bound for x in a) and (b is None or all(0 <= x <= bound for x in b)), label
        out.append((label, list(a), list(b) if two else None))

    full, top = [bound] * NL, [0] * (NL - 1) + [bound]
    put("all limbs at the bound", full, full)
    put("top limb at the bound", top, top)
    put("top limb at the bound x all", top, full)
    put("all x top limb", full, top)
    put("limb 7 and 8 at the bound", [bound if i in (7, 8) else 0 for i in range(NL)], full)
    for name, l in sp.items():
        put(name + " x random", l, _rand_limbs(rng, MASK))
        put("random x " + name, _rand_limbs(rng, MASK), l)
        put(name + " x " + name, l, l)
    for name in ("0", "1", "p-1", "2^224"):
        other = _second_rep(rng.randrange(P))
        if max(_second_rep(SPECIAL[name])) <= bound:
            put("second representative of " + name, _second_rep(SPECIAL[name]), other if max(other) <= bound else [x & MASK for x in other])
    if op == MUL:
        for t in range(6):
            x = rng.randrange(2, P)
            inv = pow(x, P - 2, P)
            put("product 0 (%d)" % t, limbs(x), sp["p"] if t % 2 else sp["0"])
            put("product 1 (%d)" % t, limbs(x), limbs(inv) if t % 2 else _second_rep(inv))
            put("product p - 1 (%d)" % t, limbs(x) if t % 2 else _second_rep(x), limbs(P - inv))
        for k in (0, 7, 8, 15, 22, 30):
            put("column %d maximal" % k, *_column_peak(k, bound))
            put("column %d maximal in a full product" % k, *[[max(x, MASK) for x in v] for v in _column_peak(k, bound)])
    if op == SQR:
        for k in (0, 7, 8, 15, 22, 30):
            a, b = _column_peak(k, bound)
            put("column %d maximal" % k, [max(x, y) for x, y in zip(a, b)])
    if op in (CANON, CARRY):
        for t in range(10):                                # the weak reduction lands in [p, 2^448)
            v = P + rng.getrandbits(rng.choice((1, 8, 100, 223)))
            assert P <= v < 2 ** 448
            put("in [p, 2^448) (%d)" % t, limbs(v))
            put("in [p, 2^448), lazy (%d)" % t, _uncarry(_uncarry(limbs(v), t), 8 + t % 7))
        put("2^448 - 1, lazy", _uncarry(sp["2^448-1"], 14))
        put("p, lazy at the fold", _uncarry(sp["p"], 7))
    if op == INVERT:
        for name in ("0", "1", "p-1", "2^224", "p", "p+1"):
            put("invert " + name, sp[name])
    n_random = 6 if op == INVERT else 40
    for t in range(n_random):
        put("random tight %d" % t, _rand_limbs(rng, MASK), _rand_limbs(rng, MASK))
        put("random at the bound %d" % t, _rand_limbs(rng, bound), _rand_limbs(rng, bound))
    if op == INVERT:                                       # the chain is 460 products: keep the list short
        out = [r for r in out if " x " not in r[0] or r[0].endswith("x random")][:40]
    _cache[op] = out
    return out


def flat(rows_, which):
    """the a (1) or b (2) limbs of the rows as one list of 32-bit words; b None -> None"""
    if rows_[0][which] is None:
        return None
    return [x for r in rows_ for x in r[which]]
