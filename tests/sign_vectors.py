"""Adversarial inputs for the signing finish steps (csrc/ecgpu_sign.h: ecdsa_sign_finish_words, SignScalar::add / neg,
ScalarN::is_high, reduce_wire, schnorr_sign_finish_words; csrc/ecgpu_sm2sign.h: sm2dsa_sign_finish_words, sm2_sub_mod): "s chosen
first".  Shared by tests/test_sign_vectors.py (the model and the g++ twins) and tests/test_gpu_sign_vectors.py (gfx950).  Plain
module: no GPU, no ctypes of its own, deterministic (seeded per set); every expected value is what the CONSTRUCTION says, a Python
integer, never a signer's answer.

The forms with the caller's nonce leave d, k and z (or e) free.  With k fixed, R = k G and r = x(R) mod n are known, and

  ECDSA   s = k^-1 (z + r d):  z = s k - r d puts s where the test wants it; d = v r^-1 makes r d = v, so the integer z + v is
          chosen; k = a^-1 and z = b - r d hand S::mul(kinv, sum) the operands (a, b).
  SM2DSA  s = (1 + d)^-1 (k - r d):  d = a^-1 - 1 makes (1 + d)^-1 = a; r = (k - b) d^-1 and e = r - x(R) make k - r d = b;
          s = a b with both operands chosen.
  BIP340  the challenge e = H(x(R) || x(P) || m) hashes x(R) and x(P): no input of ecgpu_schnorr_sign_raw_batch steers s.  Steered
          Schnorr vectors therefore exist only for the hook below (`hook_schnorr`).

ECDSA families (each of the ten sets of sign_model.ECDSA_SETS; every one is run with normalize_s 0 and 1):
  S    s chosen: 0 (ok = 0, a zero record, recid 0), 1, 2, n - 1, n - 2, (n - 1) / 2 and (n + 1) / 2 with their outer neighbours,
       2^(32 N - 1) and its neighbours where below n, and the structured scalars of field_vectors.n_operands.
  S+n  the twins z + n of the NAMED targets of S where z + n < 2^(8 L) (p521 also z + 2n, z + 127n and the largest z + j n that
       fits 66 bytes): the same signature.
  A    the integer z + r d at n - 1, n, n + 1, 2n - 2 and, where they do not exceed 2n - 2, at 2^(32 N) - 1, 2^(32 N), 2^(32 N) + 1.
  M    both operands of S::mul(kinv, sum): the pairs field_vectors.family_n uses for the scalar multiplication.
  I    the branch-free inversion in situ: nonces from modinv_vectors (family_l, family_t, the search constants of family_s).
  Z    p521 only: prehashes j n - 1, j n, j n + 1 for j in 1, 2, 64, 127, 128: the conditional subtractions of reduce_wire.
  P    position (`position_batches`): each failing vector among good neighbours in a batch of 257, at elements 0, 63, 64, 255, 256.
The families that reuse an existing list (the operands of S, M, I) take every ceil(len / cap)-th entry of it, first and last
included (`thin`): those lists run to thousands of entries per set and are already run in full by the scalar self-test ops 40 - 44
and the inversion suites; here they only have to reach the finish step in situ, and a set's list stays at a few hundred vectors.
`report` states how many of how many were taken.

What could not be built is listed (`missing`), and tests/test_sign_vectors.py asserts that list.

The hook vectors (`hook_ecdsa`, `hook_sm2`, `hook_schnorr`) are stages no pipeline input produces — x(R) in [n, p), x(R) = n,
r_inf = 1, a cleared flag beside a valid k, a Schnorr k that cancels e d' — for the CPU twins (hs_ecdsa_sign_finish, ...) and for
ecgpu_selftest_sign_finish, which launches the product's finish kernels on them."""
import hashlib
import random
from collections import Counter, namedtuple

import field_vectors
import modinv_vectors
import pyec
import sign_model
import sm2sign_model

# d, k, z: what the entry point is handed.  s: the construction's s before NORMALIZE_S (0: the element must fail; None: a range
# failure of d or k, the element must fail whatever else).  target: the value the vector was built to hit.
Vec = namedtuple("Vec", "family label target d k z s")
# SM2DSA: r and s as the construction gives them (ok False: the element must fail)
Sm2Vec = namedtuple("Sm2Vec", "family label target d k e r s ok")
# a finish-step record for the hook: everything the kernel reads
HookVec = namedtuple("HookVec", "family label target d k flag z x y r_inf s")
SchnorrHookVec = namedtuple("SchnorrHookVec", "family label target d px k flag x y r_inf msg s")

ECDSA_FAMILIES = ("S", "S+n", "A", "M", "I", "Z")
SM2_FAMILIES = ("S", "M", "B", "R", "E+n")
CAP_OPERANDS, CAP_PAIRS, CAP_INV_L, CAP_INV_T = 120, 160, 120, 60
POSITIONS = (0, 63, 64, 255, 256)
BATCH = 257
TWIN_SETS = ("bp256", "bp384", "bp256t1", "bp384t1", "p521")      # the sets that must have z + n twins


def thin(seq, cap):
    """every ceil(len / cap)-th entry, the first and the last included"""
    seq = list(seq)
    if len(seq) <= cap:
        return seq
    idx = sorted({round(i * (len(seq) - 1) / (cap - 1)) for i in range(cap)})
    return [seq[i] for i in idx]


def words(c):
    return (8 * c.L + 31) // 32


class Points:
    """k -> affine k G.  `prefetch` takes a batch from the oracle's C code where the caller has it; a single k is
    sign_model.mul_g."""

    def __init__(self, c, oracle=None):
        self.c, self.oracle, self.cache = c, oracle, {}

    def prefetch(self, ks):
        ks = [k for k in dict.fromkeys(ks) if k not in self.cache]
        if not ks:
            return
        if self.oracle is None:
            for k in ks:
                self.cache[k] = sign_model.mul_g(self.c, k)
            return
        c = self.c
        xy, inf = self.oracle.batch_mul_base(c.cid, b"".join(k.to_bytes(c.L, "big") for k in ks))
        assert not inf.any()
        b = bytes(xy)
        for i, k in enumerate(ks):
            self.cache[k] = (int.from_bytes(b[2 * i * c.L:(2 * i + 1) * c.L], "big"), int.from_bytes(b[(2 * i + 1) * c.L:(2 * i + 2) * c.L], "big"))

    def __call__(self, k):
        if k not in self.cache:
            self.cache[k] = sign_model.mul_g(self.c, k)
        return self.cache[k]


# ---- ECDSA ------------------------------------------------------------------------------------------------------------------------

def named_s_targets(c):
    n = c.n
    half = 1 << (32 * words(c) - 1)
    out = [("s = 0", 0), ("s = 1", 1), ("s = 2", 2), ("s = n - 1", n - 1), ("s = n - 2", n - 2),
           ("s = (n - 1) / 2 - 1", (n - 1) // 2 - 1), ("s = (n - 1) / 2", (n - 1) // 2),
           ("s = (n + 1) / 2", (n + 1) // 2), ("s = (n + 1) / 2 + 1", (n + 1) // 2 + 1)]
    out += [("s = 2^(32 N - 1) %+d" % dl, half + dl) for dl in (-1, 0, 1) if half + dl < n]
    return out


def sum_targets(c):
    """(label, the integer z + r d), and the labels that do not exist on this set"""
    n = c.n
    W = 1 << (32 * words(c))
    out = [("n - 1", n - 1), ("n", n), ("n + 1", n + 1), ("2n - 2", 2 * n - 2)]
    gone = []
    for label, t in (("2^(32 N) - 1", W - 1), ("2^(32 N)", W), ("2^(32 N) + 1", W + 1)):
        if t <= 2 * n - 2:
            out.append((label, t))
        else:
            gone.append(label)
    return out, gone


_ecdsa_cache = {}


def ecdsa_vectors(name, oracle=None):
    """-> (vectors, missing, thinned): missing = [(family, what, why)], thinned = {family part: (taken, of)}"""
    if name in _ecdsa_cache:
        return _ecdsa_cache[name]
    c = pyec.CURVES[name]
    n, L = c.n, c.L
    wire = 1 << (8 * L)
    rng = random.Random("sign-vectors-ecdsa-" + name)
    key = lambda: rng.randrange(1, n)
    inv = lambda v: pow(v, -1, n)
    pts = Points(c, oracle)
    vec, missing, thinned = [], [], {}

    k0 = key()
    operands = field_vectors.n_operands(name)
    pairs = [(a, b) for a, b in zip(*field_vectors.family_n(name)[40][:2]) if a % n]
    inv_l, inv_t = modinv_vectors.family_l(name, "n"), modinv_vectors.family_t(name, "n")
    inv_s = modinv_vectors.family_s(name, "n")
    t_ops, t_pairs, t_l, t_t = thin(operands, CAP_OPERANDS), thin(pairs, CAP_PAIRS), thin(inv_l, CAP_INV_L), thin(inv_t, CAP_INV_T)
    thinned = {"S operands": (len(t_ops), len(operands)), "M pairs": (len(t_pairs), len(pairs)),
               "I family_l": (len(t_l), len(inv_l)), "I family_t": (len(t_t), len(inv_t)), "I family_s": (len(inv_s), len(inv_s))}
    nonces = [k for k in dict.fromkeys(t_l + t_t + inv_s) if 1 <= k < n]
    pts.prefetch([k0] + [inv(a) for a, _ in t_pairs] + nonces)

    # S and its twins
    R0 = pts(k0)
    r0 = R0[0] % n
    assert r0
    twins = 0
    for label, s in named_s_targets(c):
        d = key()
        z = (s * k0 - r0 * d) % n
        vec.append(Vec("S", label, s, d, k0, z, s))
        js = []
        if z + n < wire:
            js = [1]
            if name == "p521":
                js = sorted({1, 2, 127, (wire - 1 - z) // n})
        for j in js:
            assert z + j * n < wire
            vec.append(Vec("S+n", "%s | z + %d n" % (label, j), s, d, k0, z + j * n, s))
            twins += 1
    if not twins:
        missing.append(("S+n", "z + n", "no constructed z leaves room below 2^(8 L)"))
    for s in t_ops:
        d = key()
        vec.append(Vec("S", "s = operand %#x" % s, s, d, k0, (s * k0 - r0 * d) % n, s))

    # A: the integer z + v, v = r d
    targets, gone = sum_targets(c)
    for label in gone:
        missing.append(("A", "z + r d = " + label, "above 2n - 2"))
    for label, t in targets:
        lo, hi = max(0, t - (n - 1)), min(n - 1, t - 1)
        assert lo <= hi
        for z in dict.fromkeys([lo, hi, rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)]):
            v = t - z
            assert 1 <= v < n and 0 <= z < n
            d = v * inv(r0) % n
            vec.append(Vec("A", "z + r d = %s, z = %#x" % (label, z), t, d, k0, z, inv(k0) * (t % n) % n))

    # M: kinv = a, sum = b
    for a, b in t_pairs:
        k = inv(a)
        r = pts(k)[0] % n
        d = key()
        vec.append(Vec("M", "kinv = %#x, sum = %#x" % (a, b), (a, b), d, k, (b - r * d) % n, a * b % n))

    # I: the nonce is the inversion's input
    for k in nonces:
        r = pts(k)[0] % n
        d, z = key(), rng.getrandbits(8 * L)
        vec.append(Vec("I", "k = %#x" % k, k, d, k, z, inv(k) * (z % n + r * d) % n))

    # Z: reduce_wire on the multiples of n (the only set whose wire holds more than 2n)
    if name == "p521":
        for j in (1, 2, 64, 127, 128):
            for dl in (-1, 0, 1):
                z = j * n + dl
                if z < wire:
                    d = key()
                    vec.append(Vec("Z", "z = %d n %+d" % (j, dl), z, d, k0, z, inv(k0) * (z % n + r0 * d) % n))
                else:
                    missing.append(("Z", "z = %d n %+d" % (j, dl), "does not fit 66 bytes"))
        z = wire - 1
        vec.append(Vec("Z", "z = 2^528 - 1", z, 5, k0, z, inv(k0) * (z % n + r0 * 5) % n))
        # ... and beside r d = n - 1, the largest: a prehash left at n + 1 or above would carry the sum to 2n and beyond
        d = (n - 1) * inv(r0) % n
        for label, z in (("z = 128 n +1", 128 * n + 1), ("z = 128 n +2", 128 * n + 2), ("z = 2^528 - 1", wire - 1)):
            vec.append(Vec("Z", label + ", r d = n - 1", z, d, k0, z, inv(k0) * (z % n + n - 1) % n))

    assert len({(v.family, v.label) for v in vec}) == len(vec), name
    _ecdsa_cache[name] = (vec, missing, thinned)
    return _ecdsa_cache[name]


def expect_ecdsa(c, s, R, normalize_s, usable=True):
    """the record the construction gives: s as constructed (None / 0: fails), R the affine point (x may be forged), -> (sig, recid, ok)"""
    n = c.n
    r = R[0] % n
    if not usable or s is None or s == 0 or r == 0:
        return (bytes(2 * c.L), 0, 0)
    recid = (R[1] & 1) | (2 if R[0] >= n else 0)
    if normalize_s and s > (n - 1) // 2:
        s, recid = n - s, recid ^ 1
    return (r.to_bytes(c.L, "big") + s.to_bytes(c.L, "big"), recid, 1)


def ecdsa_expected(name, vec, normalize_s, oracle=None):
    """[(sig, recid, ok)] for ecdsa_vectors / position vectors"""
    c = pyec.CURVES[name]
    pts = Points(c, oracle)
    pts.prefetch([v.k for v in vec if 1 <= v.k < c.n])
    return [expect_ecdsa(c, v.s, pts(v.k) if 1 <= v.k < c.n else (1, 0), normalize_s, v.s is not None) for v in vec]


def ecdsa_failures(name):
    """the failing vectors of family P: s = 0 and the range failures of d and k"""
    c = pyec.CURVES[name]
    n = c.n
    rng = random.Random("sign-vectors-fail-" + name)
    key = lambda: rng.randrange(1, n)
    k, d = key(), key()
    r = sign_model.mul_g(c, k)[0] % n
    out = [Vec("P", "s = 0", 0, d, k, (-r * d) % n, 0)]
    for v, what in ((0, "0"), (n, "n"), ((1 << (8 * c.L)) - 1, "2^(8 L) - 1")):
        out.append(Vec("P", "d = " + what, v, v, key(), rng.getrandbits(8 * c.L), None))
        out.append(Vec("P", "k = " + what, v, key(), v, rng.getrandbits(8 * c.L), None))
    return out


def position_batches(name):
    """-> (good, fails, layouts): good = BATCH ordinary vectors (family "P", s by the model's formula); layouts = one list of
    (position, index into fails) per batch, every failing vector at every one of POSITIONS over the batches"""
    c = pyec.CURVES[name]
    n = c.n
    rng = random.Random("sign-vectors-pos-" + name)
    fails = ecdsa_failures(name)
    ks = [rng.randrange(1, n) for _ in range(8)]                  # eight nonces shared by the neighbours: eight points to compute
    good = []
    for i in range(BATCH):
        k, d, z = ks[i % 8], rng.randrange(1, n), rng.getrandbits(8 * c.L)
        good.append((d, k, z))
    rs = {k: sign_model.mul_g(c, k)[0] % n for k in ks}
    good = [Vec("P", "neighbour %d" % i, None, d, k, z, pow(k, -1, n) * (z % n + rs[k] * d) % n) for i, (d, k, z) in enumerate(good)]
    layouts = [[(p, (i + j) % len(fails)) for i, p in enumerate(POSITIONS)] for j in range(len(fails))]
    for f in range(len(fails)):
        assert sorted(p for lay in layouts for p, g in lay if g == f) == sorted(POSITIONS)
    return good, fails, layouts


def placed(good, fails, layout):
    out = list(good)
    for p, f in layout:
        out[p] = fails[f]
    return out


# ---- SM2DSA -----------------------------------------------------------------------------------------------------------------------

_sm2_cache = {}


def sm2_vectors(oracle=None):
    """-> (vectors, missing, thinned)"""
    if "v" in _sm2_cache:
        return _sm2_cache["v"]
    c, n = pyec.SM2, pyec.SM2.n
    rng = random.Random("sign-vectors-sm2")
    inv = lambda v: pow(v, -1, n)
    pts = Points(c, oracle)
    vec, missing = [], []
    k0 = rng.randrange(2, n - 1)
    x0 = pts(k0)[0] % n

    def built(family, label, target, a, b, k=k0, x=x0):
        """d = a^-1 - 1, r = (k - b) / d, e = r - x(R): s = a b"""
        assert a % n not in (0, 1)
        d = (inv(a) - 1) % n
        r = (k - b) * inv(d) % n
        assert r != 0 and (r + k) % n != 0, label
        s = a * b % n
        return Sm2Vec(family, label, target, d, k, (r - x) % n, r, s, s != 0)

    def free_a():
        return rng.randrange(2, n)

    for label, s in named_s_targets(c):
        a = free_a()
        vec.append(built("S", label, s, a, s * inv(a) % n))
    operands = field_vectors.n_operands("sm2")
    t_ops = thin(operands, CAP_OPERANDS)
    for s in t_ops:
        a = free_a()
        vec.append(built("S", "s = operand %#x" % s, s, a, s * inv(a) % n))
    pairs = [(a, b) for a, b in zip(*field_vectors.family_n("sm2")[40][:2]) if a % n not in (0, 1) and b != k0]
    t_pairs = thin(pairs, CAP_PAIRS)
    for a, b in t_pairs:
        vec.append(built("M", "(1 + d)^-1 = %#x, k - r d = %#x" % (a, b), (a, b), a, b))
    # the two sides of sm2_sub_mod's borrow: k - r d = 0 (fails: s = 0), 1, n - 1 with k small and large
    for kk, what in ((k0, "k0"), (1, "1"), (n - 1, "n - 1")):
        xk = pts(kk)[0] % n
        for b in (0, 1, n - 1):
            if b == kk:                                            # r = 0: not this family's failure
                continue
            vec.append(built("B", "k - r d = %s, k = %s" % ({0: "0", 1: "1"}.get(b, "n - 1"), what), b, free_a(), b, kk, xk))
    # r chosen directly
    for label, r in (("r = 1", 1), ("r = n - 1", n - 1), ("r = n - k", n - k0), ("r = n - k - 1", n - k0 - 1), ("r = n - k + 1", n - k0 + 1)):
        d = rng.randrange(1, n - 1)
        s = inv(1 + d) * (k0 - r * d) % n
        ok = (r + k0) % n != 0 and s != 0
        assert ok == (label != "r = n - k")
        vec.append(Sm2Vec("R", label, r, d, k0, (r - x0) % n, r, s, ok))
    # e + n twins: r = x(R) + j makes e = j, which leaves room below 2^256 for j < 2^256 - n
    room = (1 << 256) - n
    assert room > 2
    for j in (0, 1, room // 2, room - 1):
        r = (x0 + j) % n
        d = rng.randrange(1, n - 1)
        s = inv(1 + d) * (k0 - r * d) % n
        assert r and (r + k0) % n and s
        vec.append(Sm2Vec("E+n", "e = %#x" % j, j, d, k0, j, r, s, True))
        vec.append(Sm2Vec("E+n", "e = %#x + n" % j, j + n, d, k0, j + n, r, s, True))
    assert len({(v.family, v.label) for v in vec}) == len(vec)
    thinned = {"S operands": (len(t_ops), len(operands)), "M pairs": (len(t_pairs), len(pairs))}
    _sm2_cache["v"] = (vec, missing, thinned)
    return _sm2_cache["v"]


def expect_sm2(v):
    if not v.ok:
        return sm2sign_model.ZERO
    return (v.r.to_bytes(32, "big") + v.s.to_bytes(32, "big"), 1)


def sm2_failures():
    """the failing vectors of the position family: s = 0, r = 0, r + k = 0 and the range failures of d and k"""
    n = pyec.SM2.n
    rng = random.Random("sign-vectors-sm2-fail")
    rnd = lambda: rng.randrange(2, n - 1)
    x_of = lambda k: sign_model.mul_g(pyec.SM2, k)[0]
    out = []
    k, d = rnd(), rnd()
    r = k * pow(d, -1, n) % n
    out.append(Sm2Vec("P", "s = 0", 0, d, k, (r - x_of(k)) % n, r, 0, False))
    k = rnd()
    out.append(Sm2Vec("P", "r = 0", 0, rnd(), k, (-x_of(k)) % n, 0, None, False))
    k = rnd()
    out.append(Sm2Vec("P", "r + k = 0", 0, rnd(), k, (-k - x_of(k)) % n, n - k, None, False))
    for v, what in ((0, "0"), (n - 1, "n - 1"), (n, "n"), (2 ** 256 - 1, "2^256 - 1")):
        out.append(Sm2Vec("P", "d = " + what, v, v, rnd(), rnd(), None, None, False))
    for v, what in ((0, "0"), (n, "n"), (2 ** 256 - 1, "2^256 - 1")):
        out.append(Sm2Vec("P", "k = " + what, v, rnd(), v, rnd(), None, None, False))
    return out


def sm2_position_batches():
    """as position_batches; the neighbours' records are sm2sign_model.sign's"""
    c, n = pyec.SM2, pyec.SM2.n
    rng = random.Random("sign-vectors-sm2-pos")
    fails = sm2_failures()
    ks = [rng.randrange(1, n) for _ in range(8)]
    xs = {k: sign_model.mul_g(c, k) for k in ks}
    good = []
    for i in range(BATCH):
        k, d, e = ks[i % 8], rng.randrange(1, n - 1), rng.getrandbits(256)
        sig, ok = sm2sign_model.sign(d, k, e, R=xs[k])
        assert ok
        good.append(Sm2Vec("P", "neighbour %d" % i, None, d, k, e, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big"), True))
    layouts = [[(p, (i + j) % len(fails)) for i, p in enumerate(POSITIONS)] for j in range(len(fails))]
    for f in range(len(fails)):
        assert sorted(p for lay in layouts for p, g in lay if g == f) == sorted(POSITIONS)
    return good, fails, layouts


# ---- the hook: stages no pipeline input produces ---------------------------------------------------------------------------------

def hook_ecdsa(name):
    """forged x(R) at n (r = 0: a zero record), n + 1, p - 1 (where n < p) and n - 1, crossed with the named s targets, y odd and
    even; the identity flag; a cleared nonce flag beside a valid k.  -> (vectors, missing)"""
    c = pyec.CURVES[name]
    n, p = c.n, c.p
    rng = random.Random("sign-vectors-hook-" + name)
    key = lambda: rng.randrange(1, n)
    vec, missing = [], []
    xs = [("x = n", n), ("x = n + 1", n + 1), ("x = p - 1", p - 1), ("x = n - 1", n - 1)]
    for xl, x in xs:
        if not x < p:
            missing.append(("H", xl, "p <= n"))
            continue
        r = x % n
        for i, (sl, s) in enumerate(named_s_targets(c)):
            d, k = key(), key()
            y = rng.randrange(2, p) & ~1 | (i & 1)
            vec.append(HookVec("H", "%s, %s, y %s" % (xl, sl, "odd" if y & 1 else "even"), (x, s), d, k, 1, (s * k - r * d) % n, x, y, 0,
                               s if r else 0))
    d, k, z = key(), key(), rng.getrandbits(8 * c.L)
    R = sign_model.mul_g(c, k)
    s = pow(k, -1, n) * (z % n + R[0] % n * d) % n
    vec.append(HookVec("H", "honest stages", None, d, k, 1, z, R[0], R[1], 0, s))
    vec.append(HookVec("H", "r_inf = 1", None, d, k, 1, z, R[0], R[1], 1, None))
    vec.append(HookVec("H", "flag = 0, k valid", None, d, k, 0, z, R[0], R[1], 0, None))
    return vec, missing


def hook_ecdsa_expected(name, vec, normalize_s):
    c = pyec.CURVES[name]
    return [expect_ecdsa(c, v.s, (v.x, v.y), normalize_s, bool(v.flag) and not v.r_inf) for v in vec]


def hook_sm2():
    """x(R) in [n, p) and at n (reduced once: r = e), the identity flag, a cleared flag -> [(row for sm2sign_model.finish, label)]"""
    n, p = pyec.SM2.n, pyec.SM2.p
    rng = random.Random("sign-vectors-hook-sm2")
    rnd = lambda: rng.randrange(2, n - 1)
    rows = []
    for label, x in (("x = n", n), ("x = n + 1", n + 1), ("x = p - 1", p - 1), ("x = n - 1", n - 1)):
        for e in (0, 1, n - 1, rnd()):
            rows.append(("%s, e = %#x" % (label, e), (rnd(), rnd(), 1, e, x, 0)))
    rows.append(("r_inf = 1", (rnd(), rnd(), 1, rnd(), rnd(), 1)))
    rows.append(("flag = 0, k valid", (rnd(), rnd(), 0, rnd(), rnd(), 0)))
    return rows


def schnorr_challenge(x, px, msg):
    return int.from_bytes(sign_model.tagged_hash(b"BIP0340/challenge", x.to_bytes(32, "big") + px.to_bytes(32, "big") + msg), "big") % pyec.K256.n


def hook_schnorr():
    """k_schnorr_sign_finish: s = k' + e d' with k' = n - k when y(R) is odd and e from the model's challenge hash.  The integer
    k' + e d' at n - 1, n (s = 0: ok = 0), n + 1, 2^256 - 1, 2^256, 2^256 + 1, each with y(R) odd and even and with d' from a key
    whose y(P) is odd and one whose y(P) is even; the identity flag; a cleared flag."""
    c = pyec.K256
    n = c.n
    rng = random.Random("sign-vectors-hook-schnorr")
    keys = {}
    while len(keys) < 2:                                          # one key of each parity of y(P)
        d = rng.randrange(1, n)
        P = sign_model.mul_g(c, d)
        keys.setdefault(P[1] & 1, (n - d if P[1] & 1 else d, P[0]))
    vec = []
    targets = [("n - 1", n - 1), ("n", n), ("n + 1", n + 1), ("2^256 - 1", 2 ** 256 - 1), ("2^256", 2 ** 256), ("2^256 + 1", 2 ** 256 + 1)]
    for py_odd, (dd, px) in sorted(keys.items()):
        for ry_odd in (0, 1):
            for label, t in targets:
                while True:                                       # a forged R: any x, the parity of y is all the step reads
                    x, msg = rng.randrange(1, c.p), bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 32, 45))))
                    ed = schnorr_challenge(x, px, msg) * dd % n
                    if 1 <= t - ed < n:
                        break
                kp = t - ed                                       # the k the sum sees
                k = n - kp if ry_odd else kp
                y = rng.randrange(2, c.p) & ~1 | ry_odd
                vec.append(SchnorrHookVec("H", "k' + e d' = %s, y(R) %s, y(P) %s" % (label, "odd" if ry_odd else "even", "odd" if py_odd else "even"),
                                          t, dd, px, k, 1, x, y, 0, msg, t % n))
    dd, px = keys[0]
    x, y, k, msg = rng.randrange(1, c.p), rng.randrange(1, c.p), rng.randrange(1, n), b"m"
    vec.append(SchnorrHookVec("H", "r_inf = 1", None, dd, px, k, 1, x, y, 1, msg, None))
    vec.append(SchnorrHookVec("H", "flag = 0, k valid", None, dd, px, k, 0, x, y, 0, msg, None))
    return vec


def expect_schnorr(v):
    if v.s is None or v.s == 0:
        return (bytes(64), 0)
    return (v.x.to_bytes(32, "big") + v.s.to_bytes(32, "big"), 1)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------

def counts(vec):
    return Counter(v.family for v in vec)


def report(oracle=None):
    """vectors per set and family, what was thinned, what could not be built"""
    lines = []
    for name in sign_model.ECDSA_SETS:
        vec, missing, thinned = ecdsa_vectors(name, oracle)
        cnt = counts(vec)
        hv, hmiss = hook_ecdsa(name)
        lines.append("ecdsa %-8s %4d vectors: %s; P %d failing x %d positions in %d batches of %d; hook %d" % (
            name, len(vec), ", ".join("%s %d" % (f, cnt[f]) for f in ECDSA_FAMILIES), len(ecdsa_failures(name)), len(POSITIONS),
            len(ecdsa_failures(name)), BATCH, len(hv)))
        lines.append("    taken of the shared lists: " + ", ".join("%s %d / %d" % (k, a, b) for k, (a, b) in thinned.items()))
        for fam, what, why in missing + hmiss:
            lines.append("    not built: %s, %s (%s)" % (fam, what, why))
    vec, missing, thinned = sm2_vectors(oracle)
    cnt = counts(vec)
    lines.append("sm2dsa         %4d vectors: %s; P %d failing x %d positions; hook %d" % (
        len(vec), ", ".join("%s %d" % (f, cnt[f]) for f in SM2_FAMILIES), len(sm2_failures()), len(POSITIONS), len(hook_sm2())))
    lines.append("    taken of the shared lists: " + ", ".join("%s %d / %d" % (k, a, b) for k, (a, b) in thinned.items()))
    lines.append("bip340         no steered vector through the entry point (the challenge hashes x(R) and x(P)); hook %d" % len(hook_schnorr()))
    return "\n".join(lines)


def first_mismatch(name, what, vec, got, want):
    """None, or a message naming the set, the family, the label and the first differing element"""
    assert len(got) == len(want) == len(vec), (name, what, len(got), len(want), len(vec))
    if list(got) == list(want):
        return None
    i = next(j for j in range(len(want)) if got[j] != want[j])
    bad = sum(1 for g, w in zip(got, want) if g != w)
    show = lambda rec: tuple(x.hex() if isinstance(x, (bytes, bytearray)) else x for x in rec)
    return "%s %s: %d of %d differ, first at element %d: family %s, %s: got %r, want %r" % (
        name, what, bad, len(want), i, vec[i].family, vec[i].label, show(got[i]), show(want[i]))


if __name__ == "__main__":
    import oracle_lib
    oracle_lib.build()
    print(report(oracle_lib))
