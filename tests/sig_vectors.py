"""Adversarial signatures for every verification scheme: R first, the key derived from it (test infrastructure, no GPU, no oracle).

gpu_common's *_cases sign with a random nonce, so x(R), u1, u2 and the key are all random and nothing structured ever reaches
`ecgpu_verify.h`.  Here the point R the verifier will arrive at is CHOSEN, with r, s and the digest, and the public key follows:
    ECDSA                     Q = u2^-1 (R - u1 G)        u1 = z / s, u2 = r / s
    SM2DSA                    Q = t^-1 (R - s G)          t = r + s
    bign                      Q = b^-1 (R - a G)          a = S1 + H, b = S0 + 2^128, S0 = belt-hash(OID || x(R) || H)[:16]
    BIP340, challenge given   P = (-e)^-1 (R - s G)
    recovery                  nothing to derive: the key is r^-1 (s R - z G)
No nonce is known and none is needed.  Every vector is (family, label, inputs, expected); the expected verdict is what the
construction says (the ranges of the scheme, the key's encoding, x(R) against r), never the answer of a verifier —
tests/test_sig_vectors.py holds it against pyec's models, the oracle and the CPU build of the kernels' code, and
tests/test_gpu_sig_vectors.py runs the same vectors on the device.  Inputs are Python integers and may exceed the field or the
order (x + p, r + n, ...); a value the curve's wire width cannot hold is left out and counted in `skipped(scheme, curve)`.

What the construction cannot reach: a scheme whose hash covers the key.  `schnorr_verify_raw` hashes P into e and the SM2DSA
message path hashes Q into Z, so neither can be given a chosen R; the raw BIP340 vectors below are signed with a known key and
carry only the key-side and range families.  For the same reason a key with a chosen encoding (a small x, so that x + p fits)
cannot be paired with a FIXED digest — that would be a forgery — so the message-level ECDSA vectors carry x + p / y + p only on
the curves where the derived key happens to fit (p521 always, Brainpool about every second key) and bign takes the one key whose
x + p fits and whose logarithm is known: its generator (0, y).  S0 = 1 cannot be reached by a valid bign signature (a 128-bit
preimage); it is fed as a rejected one, and the reachable extremes of S0 (top bit set, top byte zero) are searched over H.

Vectors are memoised per (scheme, curve): the CPU and the GPU tests share them and p521 costs seconds.  `GEN_SECONDS` keeps the
time each (scheme, curve) took to generate."""
import functools
import hashlib
import random
import time
from collections import Counter, namedtuple

import pyec

INF = pyec.INF
ECDSA_CURVES = ["k256", "p256", "p384", "p224", "p192", "p521", "bp256", "bp384", "bp256t1", "bp384t1"]
DIGEST = {"k256": "sha256", "p256": "sha256", "p384": "sha384", "p224": "sha224", "p521": "sha512", "bp256": "sha256", "bp384": "sha384",
          "bp256t1": "sha256", "bp384t1": "sha384"}                  # p192 has no digest in the reference: no message entry
MSG_CURVES = [c for c in ECDSA_CURVES if c in DIGEST]
MSG_LENS = (11, 150)                                                 # one block, and more than one block of every digest

Ecdsa = namedtuple("Ecdsa", "family label z r s qx qy exp exp_hs")            # exp_hs: under reject_high_s
EcdsaMsg = namedtuple("EcdsaMsg", "family label msg r s qx qy exp exp_hs")
Recover = namedtuple("Recover", "family label z r s recid exp exp_hs")         # exp: the key (x, y) or None
Schnorr = namedtuple("Schnorr", "family label e r s px py exp")               # exp None: the reference decides (odd-y keys)
SchnorrRaw = namedtuple("SchnorrRaw", "family label pkx msg r s exp")
Sm2dsa = namedtuple("Sm2dsa", "family label e r s qx qy exp")
Bign = namedtuple("Bign", "family label h s0 s1 qx qy exp")                   # h: the 32 hash bytes as a little-endian integer
BignMsg = namedtuple("BignMsg", "family label msg s0 s1 qx qy exp")

GEN_SECONDS = {}
_SKIPPED = {}


def skipped(scheme, curve):
    """Counter family -> cases left out because the wire width of the curve cannot hold one of their values."""
    return _SKIPPED.get((scheme, curve), Counter())


def counts(vectors):
    return Counter(v.family for v in vectors)


def _rng(scheme, curve):
    return random.Random("sig_vectors/%s/%s" % (scheme, curve))


def _timed(scheme):
    def deco(fn):
        @functools.lru_cache(maxsize=None)
        def wrapper(curve):
            t0 = time.perf_counter()
            _SKIPPED[(scheme, curve)] = Counter()
            out = tuple(fn(curve))
            GEN_SECONDS[(scheme, curve)] = time.perf_counter() - t0
            return out
        return functools.wraps(fn)(wrapper)
    return deco


def point_at(c, x, odd=None, step=1):
    """The curve point at the first x at or beyond `x` (below it with step = -1) that has one; y of the requested parity."""
    while 0 <= x < c.p:
        P = pyec.lift_x(c, x, 0 if odd is None else odd)
        if P is not None:
            return P
        x += step
    raise ValueError("no point")


def sub(c, P, Q):
    return pyec.add(c, P, pyec.neg(c, Q))


def fits(c, *vals):
    return all(0 <= v < 1 << (8 * c.L) for v in vals)


def _inv(a, n):
    return pow(a % n, -1, n)


def ecdsa_key(c, R, z, r, s):
    """Q = u2^-1 (R - u1 G): the key under which (r, s) on z makes the verifier arrive at R"""
    w = _inv(s, c.n)
    return pyec.mul(c, _inv(r * w, c.n), sub(c, R, pyec.mul(c, z * w % c.n, pyec.G(c))))


def ecdsa_verdicts(c, R, r, s, key_ok):
    ok = 1 <= r < c.n and 1 <= s < c.n and key_ok and R is not INF and R[0] % c.n == r
    return ok, ok and s <= (c.n - 1) // 2


# ---- ECDSA on the prehash ---------------------------------------------------------------------------------------------------
@_timed("ecdsa")
def ecdsa_vectors(curve):
    c = pyec.CURVES[curve]
    rng, n, p, G = _rng("ecdsa", curve), c.n, c.p, pyec.G(c)
    top = (1 << (8 * c.L)) - 1
    out = []
    assert p > n
    rz = lambda: rng.randrange(top + 1)
    rs = lambda: rng.randrange(1, n)

    def put(family, label, R, z, r, s, Q=None, key_ok=True, enc=None):
        """Q: the key as the verifier should understand it (derived when None); enc: its coordinates on the wire when they differ"""
        if Q is None:
            Q = ecdsa_key(c, R, z, r, s)
        assert Q is not INF and pyec.on_curve(c, Q)
        qx, qy = enc or Q
        if not fits(c, z, r, s, qx, qy):
            _SKIPPED[("ecdsa", curve)][family] += 1
            return Q
        out.append(Ecdsa(family, label, z, r, s, qx, qy, *ecdsa_verdicts(c, R, r, s, key_ok)))
        return Q

    # x(R) in [n, p): r = x - n
    x = n + 1
    def next_R():
        nonlocal x
        R = point_at(c, x, rng.randrange(2))
        x = R[0] + 1
        return R
    for label, s in (("s = 1", 1), ("s = n - 1", n - 1), ("s = (n - 1) / 2", (n - 1) // 2), ("s = (n + 1) / 2", (n + 1) // 2), ("s random", rs())):
        R = next_R()
        put("x_ge_n", label, R, rz(), R[0] - n, s)
    for label, z in (("z = 0", 0), ("z = n - 1", n - 1), ("z = n", n), ("z all ones", top), ("z random", rz()),
                     ("z = the largest multiple of n", top // n * n)):
        R = next_R()
        put("x_ge_n", label, R, z, R[0] - n, rs())
    R, z, s = next_R(), rz(), rs()
    Q = put("x_ge_n", "r = x - n, the twin of the next", R, z, R[0] - n, s)
    put("x_ge_n", "r = x(R) itself, which is >= n", R, z, R[0], s, Q)

    # the ends of the x axis
    R = point_at(c, 1, rng.randrange(2))
    put("edge_x", "the smallest x with a point", R, rz(), R[0], rs())
    R = point_at(c, p - 1, rng.randrange(2), step=-1)
    assert R[0] >= n
    put("edge_x", "the largest x below p", R, rz(), R[0] - n, rs())
    R = pyec.lift_x(c, 0, rng.randrange(2))
    if R is not None:                                              # x(R) = 0 gives r = 0: no key is derived from u2 = 0
        put("edge_x_zero", "x(R) = 0: r = 0", R, rz(), 0, rs(), pyec.mul(c, rs(), G))

    # non-canonical encodings, each beside its canonical twin
    K = point_at(c, rng.randrange(1, 1 << 16), rng.randrange(2))
    u1, u2 = rs(), rs()
    R = pyec.add(c, pyec.mul(c, u1, G), pyec.mul(c, u2, K))
    r = R[0] % n
    s = r * _inv(u2, n) % n
    z = u1 * s % n
    put("noncanonical", "key with a small x", R, z, r, s, K)
    put("noncanonical", "key (x + p, y)", R, z, r, s, K, key_ok=False, enc=(K[0] + p, K[1]))
    if top + 1 - p > p >> 16:                                      # y + p fits for a fair share of the keys: a handful of multiples of G
        Q, d = G, 1
        while Q[1] + p > top:
            Q, d = pyec.add(c, Q, G), d + 1
            assert d < 64
        z, k = rz(), rs()
        r, s = pyec.ecdsa_sign(c, d, z, k)
        R = pyec.mul(c, k, G)
        put("noncanonical", "key %d G" % d, R, z, r, s, Q)
        put("noncanonical", "key (x, y + p)", R, z, r, s, Q, key_ok=False, enc=(Q[0], Q[1] + p))
    else:
        _SKIPPED[("ecdsa", curve)]["noncanonical"] += 1
    R, z, s = next_R(), rz(), rs()
    Q = put("noncanonical", "r = x - n", R, z, R[0] - n, s)
    put("noncanonical", "r + n", R, z, R[0], s, Q)
    R, z, s = point_at(c, rng.randrange(n), rng.randrange(2)), rz(), rng.randrange(1, min(n, top + 1 - n))
    Q = put("noncanonical", "s small", R, z, R[0], s)
    put("noncanonical", "s + n", R, z, R[0], s + n, Q)

    # range failures beside a valid twin; the equation holds for every one of them once r and s are reduced
    R, z, s = point_at(c, rng.randrange(n), rng.randrange(2)), rz(), rs()
    Q = put("range", "valid", R, z, R[0], s)
    put("range", "s = 0", R, z, R[0], 0, Q)
    put("range", "s = n", R, z, R[0], n, Q)
    put("range", "r = 0", R, z, 0, s, Q)
    put("range", "r = n", R, z, n, s, Q)

    # exceptional sums in u1 G + u2 Q; z is small so that z + n fits every curve
    def both(label, R, z, r, s, Q):
        put("exceptional", label, R, z, r, s, Q)
        put("exceptional", label + ", z + n", R, z + n, r, s, Q)
    rzs = lambda: rng.randrange(1, 1 << 64)
    z, s = rzs(), rs()
    t = z * _inv(s, n) % n
    R = pyec.mul(c, 2 * t, G)
    r = R[0] % n
    both("u1 G = u2 Q: the sum is a doubling", R, z, r, s, pyec.mul(c, z * _inv(r, n), G))
    z, s, r = rzs(), rs(), rs()
    both("u1 G = -u2 Q: R = O", INF, z, r, s, pyec.mul(c, -z * _inv(r, n), G))
    k, s = rs(), rs()
    R = pyec.mul(c, k, G)
    r = R[0] % n
    both("u1 = 0", R, 0, r, s, pyec.mul(c, s * k * _inv(r, n), G))
    for sign in (1, -1):
        k, z = rs(), rzs()
        R = pyec.mul(c, k, G)
        r = R[0] % n
        both("Q = %sG" % ("" if sign > 0 else "-"), R, z, r, (z + sign * r) * _inv(k, n) % n, G if sign > 0 else pyec.neg(c, G))
    for sign in (1, -1):
        k, z = rs(), rzs()
        R = pyec.mul(c, k, G)
        r = R[0] % n
        s = z * _inv(k - sign, n) % n
        both("u2 Q = %sG" % ("" if sign > 0 else "-"), R, z, r, s, pyec.mul(c, sign * s * _inv(r, n), G))
    k, z = rs(), rzs()
    R = pyec.mul(c, k, G)
    r = R[0] % n
    both("u2 = 1", R, z, r, r, pyec.mul(c, k - z * _inv(r, n), G))
    k, z = rs(), rzs()
    R = pyec.mul(c, k, G)
    r = R[0] % n
    both("u2 = n - 1", R, z, r, n - r, pyec.mul(c, -(k + z * _inv(r, n)), G))
    return out


# ---- ECDSA from messages ----------------------------------------------------------------------------------------------------
def digest_z(c, msg):
    d = hashlib.new(DIGEST[c.name], msg).digest()
    return int.from_bytes(d[: c.L] if len(d) >= c.L else d, "big")               # bits2field: the leftmost L bytes, or left-padded


@_timed("ecdsa_msg")
def ecdsa_msg_vectors(curve):
    c = pyec.CURVES[curve]
    rng, n, p = _rng("ecdsa_msg", curve), c.n, c.p
    top = (1 << (8 * c.L)) - 1
    out = []
    rs = lambda: rng.randrange(1, n)
    x = n + 1 + rng.randrange(1 << 20)

    def next_R():
        nonlocal x
        R = point_at(c, x, rng.randrange(2))
        x = R[0] + 1
        return R

    def put(family, label, msg, R, r, s, Q=None, key_ok=True, enc=None):
        if Q is None:
            Q = ecdsa_key(c, R, digest_z(c, msg), r, s)
        assert Q is not INF
        qx, qy = enc or Q
        if not fits(c, r, s, qx, qy):
            _SKIPPED[("ecdsa_msg", curve)][family] += 1
            return Q
        out.append(EcdsaMsg(family, label, msg, r, s, qx, qy, *ecdsa_verdicts(c, R, r, s, key_ok)))
        return Q

    for ln in MSG_LENS:
        rm = lambda: bytes(rng.randrange(256) for _ in range(ln))
        for label, s in (("s random", rs()), ("s = (n - 1) / 2", (n - 1) // 2), ("s = (n + 1) / 2", (n + 1) // 2)):
            R = next_R()
            put("x_ge_n", label, rm(), R, R[0] - n, s)
        R, m, s = next_R(), rm(), rs()
        Q = put("x_ge_n", "r = x - n, the twin of the next", m, R, R[0] - n, s)
        put("x_ge_n", "r = x(R) itself, which is >= n", m, R, R[0], s, Q)
        R, m, s = point_at(c, rng.randrange(n), rng.randrange(2)), rm(), rng.randrange(1, min(n, top + 1 - n))
        Q = put("noncanonical", "s small", m, R, R[0], s)
        put("noncanonical", "s + n", m, R, R[0], s + n, Q)
        # a key cannot be chosen under a fixed digest: take derived keys until a coordinate leaves room for p
        if top + 1 - p > p >> 16:
            for coord in (0, 1):
                for _ in range(64):
                    R, m, s = point_at(c, rng.randrange(n), rng.randrange(2)), rm(), rs()
                    Q = ecdsa_key(c, R, digest_z(c, m), R[0], s)
                    if Q[coord] + p <= top:
                        break
                else:
                    raise AssertionError("no derived key leaves room for p")
                put("noncanonical", "derived key with room in %s" % "xy"[coord], m, R, R[0], s, Q)
                put("noncanonical", "key (x + p, y)" if coord == 0 else "key (x, y + p)", m, R, R[0], s, Q, key_ok=False,
                    enc=(Q[0] + p, Q[1]) if coord == 0 else (Q[0], Q[1] + p))
        else:
            _SKIPPED[("ecdsa_msg", curve)]["noncanonical"] += 2
    return out


# ---- public-key recovery ----------------------------------------------------------------------------------------------------
def recover_key(c, R, z, r, s):
    """r^-1 (s R - z G), or None for the identity"""
    if R is None:
        return None
    Q = pyec.mul(c, _inv(r, c.n), sub(c, pyec.mul(c, s, R), pyec.mul(c, z, pyec.G(c))))
    return None if Q is INF else Q


@_timed("recover")
def recover_vectors(curve):
    c = pyec.CURVES[curve]
    rng, n, p = _rng("recover", curve), c.n, c.p
    top = (1 << (8 * c.L)) - 1
    out = []
    rz = lambda: rng.randrange(top + 1)
    rs = lambda: rng.randrange(1, n)

    def put(family, label, z, r, s, recid):
        """the candidate x is r, or r + n with bit 1 of the id; it has to fit the words, lie below p and have a point"""
        ok = recid <= 3 and 1 <= r < n and 1 <= s < n
        xc = r + (n if recid & 2 else 0)
        R = pyec.lift_x(c, xc, recid & 1) if ok and xc <= top else None
        Q = recover_key(c, R, z, r, s)
        out.append(Recover(family, label, z, r, s, recid, Q, Q if s <= (n - 1) // 2 else None))
        return Q

    if 2 * n > top:                                               # every curve but p521, whose 66 bytes hold r + n
        for recid in (2, 3):
            x0 = point_at(c, rng.randrange(1, 1 << 16))[0]
            r = top + 1 - n + x0                                  # r + n = 2^(8L) + x0: a sum that drops the carry lands on x0
            assert r < n
            assert put("carry_trap", "r + n = 2^(8L) + x0, id %d" % recid, rz(), r, rs(), recid) is None
            put("carry_trap", "the same r, id %d" % (recid & 1), rz(), r, rs(), recid & 1)
    for recid in (0, 1, 2, 3):
        put("largest_r", "r = n - 1, id %d" % recid, rz(), n - 1, rs(), recid)
    x = n + 1
    for odd in (0, 1):
        R = point_at(c, x, odd)
        x = R[0] + 1
        z, s = rz(), rs()
        assert put("below_p", "x(R) >= n, id %d" % (2 | odd), z, R[0] - n, s, 2 | odd) is not None
        put("below_p", "the same with bit 1 cleared, id %d" % odd, z, R[0] - n, s, odd)
    for label, s in (("s = (n - 1) / 2", (n - 1) // 2), ("s = (n + 1) / 2", (n + 1) // 2)):
        R = point_at(c, rng.randrange(n), rng.randrange(2))
        assert put("high_s", label, rz(), R[0], s, R[1] & 1) is not None
    R, z = point_at(c, rng.randrange(n), rng.randrange(2)), rz()
    for label, r, s, recid in (("s = 1", R[0], 1, R[1] & 1), ("s = n - 1", R[0], n - 1, R[1] & 1), ("s = 0", R[0], 0, R[1] & 1),
                               ("s = n", R[0], n, R[1] & 1), ("r = 0", 0, rs(), 0), ("r = n", n, rs(), 1), ("id 4", R[0], rs(), 4 | (R[1] & 1))):
        put("range", label, z, r, s, recid)
    return out


# ---- BIP340 -----------------------------------------------------------------------------------------------------------------
def _tagged(tag, data):
    t = hashlib.sha256(tag).digest()
    return hashlib.sha256(t + t + data).digest()


@_timed("schnorr")
def schnorr_vectors(curve="k256"):
    c = pyec.CURVES[curve]
    rng, n, p, G = _rng("schnorr", curve), c.n, c.p, pyec.G(c)
    top = (1 << 256) - 1
    out = []
    rs = lambda: rng.randrange(1, n)
    re = lambda: rng.randrange(top + 1)

    def key(R, e, s):
        return pyec.mul(c, _inv(-e, n), sub(c, R, pyec.mul(c, s, G)))

    def put(family, label, R, e, r, s, P=None, key_ok=True, reference_decides=False):
        """R: where s G - e P arrives for the key P (derived when None)"""
        if P is None:
            P = key(R, e, s)
        assert P is not INF
        ok = r < p and 0 < s < n and key_ok and R is not INF and R[1] % 2 == 0 and R[0] == r
        out.append(Schnorr(family, label, e, r, s, P[0], P[1], None if reference_decides else ok))
        return P

    x = n + 1
    for odd in (0, 1):
        R = point_at(c, x, odd)
        x = R[0] + 1
        put("x_ge_n", "y(R) %s, r = x(R) >= n" % ("odd" if odd else "even"), R, re(), R[0], rs())
    e, s = re(), rs()
    put("identity", "R = O", INF, e, point_at(c, rng.randrange(p), 0)[0], s, pyec.mul(c, s * _inv(e, n), G))
    R = point_at(c, rng.randrange(1, 1 << 16), 0)
    e, s = re(), rs()
    P = put("r_range", "r = x0", R, e, R[0], s)
    put("r_range", "r = x0 + p", R, e, R[0] + p, s, P)
    for label, e in (("e = 0", 0), ("e = 1", 1), ("e = n - 1", n - 1), ("e = n", n), ("e = n + 1", n + 1), ("e all ones", top)):
        s = rs()
        if e % n == 0:                                             # R = s G whatever the key is
            R = pyec.mul(c, s, G)
            if R[1] & 1:
                s, R = n - s, pyec.neg(c, R)
            put("challenge", label, R, e, R[0], s, pyec.mul(c, rs(), G))
        else:
            R = point_at(c, rng.randrange(p), 0)
            put("challenge", label, R, e, R[0], s)
    for label, s_key, s in (("s = 1", 1, 1), ("s = n - 1", n - 1, n - 1), ("s = 0", 0, 0), ("s = n", 0, n)):
        R, e = point_at(c, rng.randrange(p), 0), re()
        put("s_range", label, R, e, R[0], s, key(R, e, s_key))
    for i in range(2):                                             # the equation holds; the reference's keys have even y
        while True:
            R, e, s = point_at(c, rng.randrange(p), 0), re(), rs()
            P = key(R, e, s)
            if P[1] & 1:
                break
        put("odd_key", "key with odd y #%d" % i, R, e, R[0], s, P, reference_decides=True)
    return out


@_timed("schnorr_raw")
def schnorr_raw_vectors(curve="k256"):
    """Signed with a known key (e hashes P: no R can be chosen); the key-side and the range families only."""
    c = pyec.CURVES[curve]
    rng, n, p, G = _rng("schnorr_raw", curve), c.n, c.p, pyec.G(c)
    top = (1 << 256) - 1
    out = []
    for ln in (32, 45):
        d = rng.randrange(1, n)
        P = pyec.mul(c, d, G)
        if P[1] & 1:
            d = n - d
        k = rng.randrange(1, n)
        R = pyec.mul(c, k, G)
        if R[1] & 1:
            k = n - k
        msg = bytes(rng.randrange(256) for _ in range(ln))
        e = int.from_bytes(_tagged(b"BIP0340/challenge", R[0].to_bytes(32, "big") + P[0].to_bytes(32, "big") + msg), "big")
        s = (k + e * d) % n
        x0 = point_at(c, rng.randrange(1, 1 << 16))[0]
        xn = next(v for v in range(x0 + 1, x0 + 64) if pyec.lift_x(c, v, 0) is None)
        put = lambda family, label, pkx, m, r_, s_, exp: out.append(SchnorrRaw(family, label, pkx, m, r_, s_, exp))
        put("range", "valid", P[0], msg, R[0], s, True)
        put("range", "another message", P[0], bytes([msg[0] ^ 1]) + msg[1:], R[0], s, False)
        put("range", "s = 0", P[0], msg, R[0], 0, False)
        put("range", "s = n", P[0], msg, R[0], n, False)
        put("range", "r = p", P[0], msg, p, s, False)
        put("range", "r all ones", P[0], msg, top, s, False)
        put("key", "key = p", p, msg, R[0], s, False)
        put("key", "key all ones", top, msg, R[0], s, False)
        put("key", "key = x0 + p", x0 + p, msg, R[0], s, False)
        put("key", "key with no point", xn, msg, R[0], s, False)
        if s + n <= top:
            put("range", "s + n", P[0], msg, R[0], s + n, False)
        else:
            _SKIPPED[("schnorr_raw", curve)]["range"] += 1
    return out


# ---- SM2DSA on the prehash --------------------------------------------------------------------------------------------------
@_timed("sm2dsa")
def sm2dsa_vectors(curve="sm2"):
    c = pyec.CURVES[curve]
    rng, n, p, G = _rng("sm2dsa", curve), c.n, c.p, pyec.G(c)
    top = (1 << 256) - 1
    out = []
    rs = lambda: rng.randrange(1, n)
    re = lambda: rng.randrange(top + 1)
    rR = lambda: point_at(c, rng.randrange(n), rng.randrange(2))

    def put(family, label, R, e, r, s, Q=None, key_ok=True, enc=None):
        """R: where s G + t Q arrives, t = r + s; x1 = 0 for the identity, as the reference takes it"""
        t = (r + s) % n
        if Q is None:
            Q = pyec.mul(c, _inv(t, n), sub(c, R, pyec.mul(c, s, G)))
        assert Q is not INF and pyec.on_curve(c, Q)
        x1 = 0 if R is INF else R[0]
        ok = 1 <= r < n and 1 <= s < n and t != 0 and key_ok and (e % n + x1) % n == r
        qx, qy = enc or Q
        assert fits(c, e, r, s, qx, qy)
        out.append(Sm2dsa(family, label, e, r, s, qx, qy, ok))
        return Q

    e, s = re(), rs()
    r = e % n
    put("identity", "R = O, r = e mod n", INF, e, r, s, pyec.mul(c, -s * _inv(r + s, n), G))
    x = n + 1
    for i in range(2):
        R = point_at(c, x, i)
        x = R[0] + 1
        e = re()
        put("x_ge_n", "x1 in [n, p) #%d" % i, R, e, (e + R[0]) % n, rs())
    R = rR()
    e = rng.randrange(n - R[0], n)                                # (e mod n) + (x1 mod n) >= n
    put("sum_wraps", "e + x1 >= n", R, e, (e + R[0]) % n, rs())
    R = point_at(c, n - (1 << 200), rng.randrange(2))              # x1 just below n: a small e wraps the sum, and e + n fits the words
    e = rng.randrange(n - R[0], top + 1 - n)
    put("sum_wraps", "e + x1 >= n with e + n on the wire", R, e + n, (e + R[0]) % n, rs())
    R = rR()
    put("sum_wraps", "e + x1 = n: r = 0", R, n - R[0], 0, rs())
    for label, e in (("e = 0", 0), ("e = n - 1", n - 1), ("e = n", n), ("e all ones", top)):
        R = rR()
        put("digest", label, R, e, (e + R[0]) % n, rs())
    R = rR()
    put("t_carry", "r = s = n - 1: r + s exceeds the words", R, (n - 1 - R[0]) % n, n - 1, n - 1)
    R = rR()
    e = re()
    r = (e + R[0]) % n
    put("t_zero", "r + s = n", R, e, r, n - r, pyec.mul(c, rs(), G))
    K = point_at(c, rng.randrange(1, 1 << 16), rng.randrange(2))
    s, t = rs(), rs()
    R = pyec.add(c, pyec.mul(c, s, G), pyec.mul(c, t, K))
    r = (t - s) % n
    e = (r - R[0]) % n
    put("noncanonical", "key with a small x", R, e, r, s, K)
    put("noncanonical", "key (x + p, y)", R, e, r, s, K, key_ok=False, enc=(K[0] + p, K[1]))
    R, e, s = rR(), re(), rs()
    r = (e + R[0]) % n
    Q = put("range", "valid", R, e, r, s)
    put("range", "s = 0", R, e, r, 0, Q)
    put("range", "s = n", R, e, r, n, Q)
    put("range", "r = n", R, e, n, s, Q)
    if r + n <= top:
        put("range", "r + n", R, e, r + n, s, Q)
    return out


# ---- bign -------------------------------------------------------------------------------------------------------------------
def bign_s0(R, h):
    """belt-hash(OID || x(R) || H)[:16] as a little-endian integer; h: the hash as a little-endian integer"""
    return int.from_bytes(pyec.belt_hash(pyec.BELT_OID + R[0].to_bytes(32, "little") + h.to_bytes(32, "little"))[:16], "little")


def _bign_put(c, out, cls, family, label, R, hm, s0, s1, Q=None, key_ok=True, enc=None):
    """R: where a G + b Q arrives; hm: the hash as an integer (Bign) or the message (BignMsg)"""
    n = c.n
    h = hm if cls is Bign else int.from_bytes(pyec.belt_hash(hm), "little")
    a, b = (s1 + h) % n, s0 + (1 << 128)
    if Q is None:
        Q = pyec.mul(c, _inv(b, n), sub(c, R, pyec.mul(c, a, pyec.G(c))))
    assert Q is not INF and pyec.on_curve(c, Q)
    ok = s0 != 0 and 0 < s1 < n and key_ok and R is not INF and bign_s0(R, h) == s0
    qx, qy = enc or Q
    assert fits(c, h, s1, qx, qy) and s0 < 1 << 128
    out.append(cls(family, label, hm, s0, s1, qx, qy, ok))
    return Q


def _bign_generator_key(c, rng, out, cls, hm):
    """the one key whose x + p fits the words and whose logarithm is known: +-G = (0, +-y), signed by the model"""
    h = hm if cls is Bign else int.from_bytes(pyec.belt_hash(hm), "little")
    for d, Q in ((1, pyec.G(c)), (c.n - 1, pyec.neg(c, pyec.G(c)))):
        k = rng.randrange(1, c.n)
        sig = pyec.bign_sign(c, d, h.to_bytes(32, "little"), k)
        s0, s1 = int.from_bytes(sig[:16], "little"), int.from_bytes(sig[16:], "little")
        R = pyec.mul(c, k, pyec.G(c))
        name = "G" if d == 1 else "-G"
        _bign_put(c, out, cls, "noncanonical", "key %s = (0, y)" % name, R, hm, s0, s1, Q)
        _bign_put(c, out, cls, "noncanonical", "key %s as (p, y)" % name, R, hm, s0, s1, Q, key_ok=False, enc=(c.p, Q[1]))


@_timed("bign")
def bign_vectors(curve="bign256"):
    c = pyec.CURVES[curve]
    rng, n, p = _rng("bign", curve), c.n, c.p
    top = (1 << 256) - 1
    out = []
    rs = lambda: rng.randrange(1, n)
    rh = lambda: rng.randrange(top + 1)
    rR = lambda: point_at(c, rng.randrange(p), rng.randrange(2))
    put = lambda *a, **k: _bign_put(c, out, Bign, *a, **k)
    for label, h in (("H random", rh()), ("H random, another", rh()), ("H >= q", rng.randrange(n, top + 1))):
        R = rR()
        put("chosen_R", label, R, h, bign_s0(R, h), rs())
    for label, h in (("H = q - 1", n - 1), ("H = q", n), ("H all ones", top)):
        R = rR()
        put("s1_carry", "S1 = q - 1, " + label, R, h, bign_s0(R, h), n - 1)
    R, h = rR(), rng.randrange(1, n)
    put("a_zero", "S1 + H = q", R, h, bign_s0(R, h), n - h)
    R, h = rR(), rng.randrange(n + 1, top + 1)
    put("a_zero", "S1 + (H mod q) = q, H >= q", R, h, bign_s0(R, h), 2 * n - h)
    R, h = point_at(c, rng.randrange(1, 1 << 16), rng.randrange(2)), rh()
    put("small_x", "x(R) below 2^16: zero bytes in the hashed x", R, h, bign_s0(R, h), rs())
    R = rR()
    h = next(h for h in iter(rh, None) if bign_s0(R, h) >> 127)
    put("s0_extremes", "S0 with its top bit set", R, h, bign_s0(R, h), rs())
    h = next(h for h in iter(rh, None) if bign_s0(R, h) >> 120 == 0)
    put("s0_extremes", "S0 with a zero top byte", R, h, bign_s0(R, h), rs())
    put("s0_extremes", "S0 = 1, which no hash reaches", R, h, 1, rs())
    put("s0_extremes", "S0 = 0", R, h, 0, rs())
    _bign_generator_key(c, rng, out, Bign, rh())
    R, h = rR(), rh()
    s0 = bign_s0(R, h)
    Q = put("range", "valid", R, h, s0, rs())
    Q0 = pyec.mul(c, _inv(s0 + (1 << 128), n), sub(c, R, pyec.mul(c, h, pyec.G(c))))     # the key for S1 = 0 mod q
    put("range", "S1 = 0", R, h, s0, 0, Q0)
    put("range", "S1 = q", R, h, s0, n, Q0)
    return out


@_timed("bign_msg")
def bign_msg_vectors(curve="bign256"):
    c = pyec.CURVES[curve]
    rng, n, p = _rng("bign_msg", curve), c.n, c.p
    out = []
    rs = lambda: rng.randrange(1, n)
    put = lambda *a, **k: _bign_put(c, out, BignMsg, *a, **k)
    for ln in (13, 70):
        rm = lambda: bytes(rng.randrange(256) for _ in range(ln))
        hv = lambda m: int.from_bytes(pyec.belt_hash(m), "little")
        R, m = point_at(c, rng.randrange(p), rng.randrange(2)), rm()
        put("chosen_R", "%d bytes" % ln, R, m, bign_s0(R, hv(m)), rs())
        R, m = point_at(c, rng.randrange(p), rng.randrange(2)), rm()
        put("chosen_R", "%d bytes, S1 = q - 1" % ln, R, m, bign_s0(R, hv(m)), n - 1)
        R, m = point_at(c, rng.randrange(p), rng.randrange(2)), rm()
        put("a_zero", "%d bytes, S1 + (H mod q) = q" % ln, R, m, bign_s0(R, hv(m)), n - hv(m) % n)
        R, m = point_at(c, rng.randrange(1, 1 << 16), rng.randrange(2)), rm()
        put("small_x", "%d bytes" % ln, R, m, bign_s0(R, hv(m)), rs())
        _bign_generator_key(c, rng, out, BignMsg, rm())
    return out


# ---- wire encodings ---------------------------------------------------------------------------------------------------------
def _be(vals, L):
    return b"".join(v.to_bytes(L, "big") for v in vals)


def pack_ecdsa(c, vec):
    """-> z, r, s, q bytes, expected verdicts (policy off), expected verdicts (reject_high_s)"""
    return (_be((v.z for v in vec), c.L), _be((v.r for v in vec), c.L), _be((v.s for v in vec), c.L),
            b"".join(v.qx.to_bytes(c.L, "big") + v.qy.to_bytes(c.L, "big") for v in vec),
            bytes(int(v.exp) for v in vec), bytes(int(v.exp_hs) for v in vec))


def pack_ecdsa_msg(c, vec):
    """one message length -> q, msgs, sigs (r || s), expected, expected under reject_high_s"""
    return (b"".join(v.qx.to_bytes(c.L, "big") + v.qy.to_bytes(c.L, "big") for v in vec), b"".join(v.msg for v in vec),
            b"".join(v.r.to_bytes(c.L, "big") + v.s.to_bytes(c.L, "big") for v in vec),
            bytes(int(v.exp) for v in vec), bytes(int(v.exp_hs) for v in vec))


def pack_recover(c, vec):
    """-> z, r, s, recid bytes, then (keys, ok) with the policy off and (keys, ok) under reject_high_s"""
    def keys(attr):
        ks = [getattr(v, attr) for v in vec]
        return (b"".join(bytes(2 * c.L) if k is None else k[0].to_bytes(c.L, "big") + k[1].to_bytes(c.L, "big") for k in ks),
                bytes(int(k is not None) for k in ks))
    return (_be((v.z for v in vec), c.L), _be((v.r for v in vec), c.L), _be((v.s for v in vec), c.L), bytes(v.recid for v in vec),
            keys("exp"), keys("exp_hs"))


def pack_schnorr(vec):
    """-> e, r, s, p_xy, expected (2 where the reference decides)"""
    return (_be((v.e for v in vec), 32), _be((v.r for v in vec), 32), _be((v.s for v in vec), 32),
            b"".join(v.px.to_bytes(32, "big") + v.py.to_bytes(32, "big") for v in vec), bytes(2 if v.exp is None else int(v.exp) for v in vec))


def pack_schnorr_raw(vec):
    """one message length -> pk_x, msgs, sigs, expected"""
    return (_be((v.pkx for v in vec), 32), b"".join(v.msg for v in vec), b"".join(v.r.to_bytes(32, "big") + v.s.to_bytes(32, "big") for v in vec),
            bytes(int(v.exp) for v in vec))


def pack_sm2dsa(vec):
    return (_be((v.e for v in vec), 32), _be((v.r for v in vec), 32), _be((v.s for v in vec), 32),
            b"".join(v.qx.to_bytes(32, "big") + v.qy.to_bytes(32, "big") for v in vec), bytes(int(v.exp) for v in vec))


def _bign_sig_key(vec):
    return (b"".join(v.s0.to_bytes(16, "little") + v.s1.to_bytes(32, "little") for v in vec),
            b"".join(v.qx.to_bytes(32, "little") + v.qy.to_bytes(32, "little") for v in vec))


def pack_bign(vec):
    """-> h, sigs, q, expected (all little-endian)"""
    sg, q = _bign_sig_key(vec)
    return b"".join(v.h.to_bytes(32, "little") for v in vec), sg, q, bytes(int(v.exp) for v in vec)


def pack_bign_msg(vec):
    """one message length -> q, msgs, sigs, expected"""
    sg, q = _bign_sig_key(vec)
    return q, b"".join(v.msg for v in vec), sg, bytes(int(v.exp) for v in vec)


def by_len(vec):
    """vectors with a .msg grouped by message length, order kept: {len: [vectors]}"""
    out = {}
    for v in vec:
        out.setdefault(len(v.msg), []).append(v)
    return out


# the families every curve has to carry; those that exist only where the curve allows are listed in the test beside the reason
FAMILIES = {
    "ecdsa": ("x_ge_n", "edge_x", "noncanonical", "range", "exceptional"),
    "ecdsa_msg": ("x_ge_n", "noncanonical"),
    "recover": ("largest_r", "below_p", "high_s", "range"),
    "schnorr": ("x_ge_n", "identity", "r_range", "challenge", "s_range", "odd_key"),
    "schnorr_raw": ("range", "key"),
    "sm2dsa": ("identity", "x_ge_n", "sum_wraps", "digest", "t_carry", "t_zero", "noncanonical", "range"),
    "bign": ("chosen_R", "s1_carry", "a_zero", "small_x", "s0_extremes", "noncanonical", "range"),
    "bign_msg": ("chosen_R", "a_zero", "small_x", "noncanonical"),
}


def report():
    """Per (scheme, curve): the case count of every family, what was left out, the seconds generation took (generates everything)."""
    lines = []
    jobs = ([("ecdsa", ecdsa_vectors, ECDSA_CURVES), ("ecdsa_msg", ecdsa_msg_vectors, MSG_CURVES), ("recover", recover_vectors, ECDSA_CURVES),
             ("schnorr", schnorr_vectors, ["k256"]), ("schnorr_raw", schnorr_raw_vectors, ["k256"]), ("sm2dsa", sm2dsa_vectors, ["sm2"]),
             ("bign", bign_vectors, ["bign256"]), ("bign_msg", bign_msg_vectors, ["bign256"])])
    for scheme, fn, curves in jobs:
        for curve in curves:
            cnt = counts(fn(curve))
            sk = skipped(scheme, curve)
            lines.append("%-11s %-8s %3d cases  %s%s  %.2f s" % (
                scheme, curve, sum(cnt.values()), "  ".join("%s %d" % kv for kv in sorted(cnt.items())),
                ("  (left out: %s)" % ", ".join("%s %d" % kv for kv in sorted(sk.items()))) if sk else "", GEN_SECONDS[(scheme, curve)]))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
