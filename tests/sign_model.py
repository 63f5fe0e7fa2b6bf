"""Independent model of the signing entry points (test infrastructure): hmac / hashlib and Python integers.

ECDSA as `ecdsa::hazmat::sign_prehashed` computes it (SEC1 v2 4.1.3) with the recovery id and the low-S rule of `NORMALIZE_S`, the
nonce of RFC 6979 section 3.2 over the curve's `DigestAlgorithm`, and BIP340 `sign_raw` with the key fix-up.  Shares nothing with the
HIP kernels; the group arithmetic is pyec's curve constants with a Jacobian ladder of its own (pyec.mul inverts at every step and is
ten times slower; tests/test_sign_model.py holds the two against each other).
"""
import hashlib
import hmac

import pyec

# the reference's `DigestAlgorithm` per curve (k256/src/ecdsa.rs:117-119, p256/src/ecdsa.rs:72-74, p384/src/ecdsa.rs:69-71,
# p224/src/ecdsa.rs:69-71, p521/src/ecdsa.rs:69-71, bp256 / bp384 likewise); p192 has none
DIGEST = {"k256": "sha256", "p256": "sha256", "bp256": "sha256", "bp256t1": "sha256", "p384": "sha384", "bp384": "sha384",
          "bp384t1": "sha384", "p224": "sha224", "p521": "sha512"}
ECDSA_SETS = ("k256", "p256", "p384", "p224", "p192", "p521", "bp256", "bp384", "bp256t1", "bp384t1")
RFC6979_SETS = tuple(s for s in ECDSA_SETS if s in DIGEST)
NORMALIZE_S = {"k256": True}          # k256/src/ecdsa.rs:104-106; false everywhere else
MAX_CANDIDATES = 128


# ---- generator multiples: Jacobian double-and-add, one inversion at the end -------------------------------------------------
def _jdbl(c, P):
    X, Y, Z = P
    if Y == 0 or Z == 0:
        return (1, 1, 0)
    p = c.p
    S = 4 * X * Y * Y % p
    M = (3 * X * X + c.a * pow(Z, 4, p)) % p
    X3 = (M * M - 2 * S) % p
    Y3 = (M * (S - X3) - 8 * pow(Y, 4, p)) % p
    return (X3, Y3, 2 * Y * Z % p)


def _jadd_affine(c, P, Q):
    X1, Y1, Z1 = P
    if Z1 == 0:
        return (Q[0], Q[1], 1)
    p = c.p
    Z1Z1 = Z1 * Z1 % p
    U2 = Q[0] * Z1Z1 % p
    S2 = Q[1] * Z1 * Z1Z1 % p
    H = (U2 - X1) % p
    R = (S2 - Y1) % p
    if H == 0:
        return _jdbl(c, P) if R == 0 else (1, 1, 0)
    HH = H * H % p
    HHH = H * HH % p
    V = X1 * HH % p
    X3 = (R * R - HHH - 2 * V) % p
    Y3 = (R * (V - X3) - Y1 * HHH) % p
    return (X3, Y3, Z1 * H % p)


def mul_g(c, k):
    """k * G as an affine pair, or None for the identity."""
    k %= c.n
    G = (c.gx, c.gy)
    R = (1, 1, 0)
    for bit in bin(k)[2:] if k else "":
        R = _jdbl(c, R)
        if bit == "1":
            R = _jadd_affine(c, R, G)
    if R[2] == 0:
        return None
    zi = pow(R[2], -1, c.p)
    return (R[0] * zi * zi % c.p, R[1] * zi * zi * zi % c.p)


# ---- ECDSA ------------------------------------------------------------------------------------------------------------------
def bits2field(c, digest):
    """ecdsa `hazmat::bits2field`: the leftmost L bytes of the digest (all of a shorter one) as an integer."""
    return int.from_bytes(digest[: c.L], "big")


def ecdsa_sign(c, d, k, z, normalize_s, R=None):
    """-> (sig = r || s as 2L bytes, recid, ok) for key d, nonce k and prehash integer z (any L-byte values).
    R: k G where the caller has it already (large batches take it from the oracle's C code), else computed here."""
    zero = (bytes(2 * c.L), 0, 0)
    if not (1 <= d < c.n and 1 <= k < c.n):
        return zero
    R = mul_g(c, k) if R is None else R
    r = R[0] % c.n
    s = pow(k, -1, c.n) * (z % c.n + r * d) % c.n
    if r == 0 or s == 0:
        return zero
    recid = (R[1] & 1) | (2 if R[0] >= c.n else 0)
    if normalize_s and s > (c.n - 1) // 2:
        s = c.n - s
        recid ^= 1
    return (r.to_bytes(c.L, "big") + s.to_bytes(c.L, "big"), recid, 1)


def rfc6979_nonce(c, d, z, cap=MAX_CANDIDATES):
    """RFC 6979 section 3.2 with x = d as L bytes, h1 = (z mod n) as L bytes, no additional data.
    -> (k, rejected): the first candidate in [1, n) and how many were rejected before it; k = None after `cap` candidates."""
    h = DIGEST[c.name]
    hlen = hashlib.new(h).digest_size
    shift = 8 * c.L - c.n.bit_length()
    x = (d % (1 << (8 * c.L))).to_bytes(c.L, "big")
    h1 = (z % c.n).to_bytes(c.L, "big")
    V = b"\x01" * hlen
    K = b"\x00" * hlen
    K = hmac.new(K, V + b"\x00" + x + h1, h).digest()
    V = hmac.new(K, V, h).digest()
    K = hmac.new(K, V + b"\x01" + x + h1, h).digest()
    V = hmac.new(K, V, h).digest()
    for rejected in range(cap):
        T = b""
        while len(T) < c.L:
            V = hmac.new(K, V, h).digest()
            T += V
        k = int.from_bytes(T[: c.L], "big") >> shift
        if 1 <= k < c.n:
            return k, rejected
        K = hmac.new(K, V + b"\x00", h).digest()
        V = hmac.new(K, V, h).digest()
    return None, cap


def ecdsa_sign_rfc6979(c, d, z, normalize_s, cap=MAX_CANDIDATES):
    """`PrehashSigner::sign_prehash` on the prehash integer z -> (sig, recid, ok)."""
    k, _ = rfc6979_nonce(c, d, z, cap)
    if k is None:
        return (bytes(2 * c.L), 0, 0)
    return ecdsa_sign(c, d, k, z, normalize_s)


def ecdsa_sign_msg(c, d, msg, normalize_s):
    """`Signer::sign(msg)`: the curve's digest, bits2field, the RFC 6979 form."""
    return ecdsa_sign_rfc6979(c, d, bits2field(c, hashlib.new(DIGEST[c.name], msg).digest()), normalize_s)


# ---- BIP340 -----------------------------------------------------------------------------------------------------------------
def tagged_hash(tag, data):
    t = hashlib.sha256(tag).digest()
    return hashlib.sha256(t + t + data).digest()


def sha256_midstate(tag):
    """The SHA-256 chaining value after the block SHA256(tag) || SHA256(tag), as eight words (ecgpu_sign.h, ecgpu_sha256.h)."""
    K = [int((q ** (1 / 3) % 1) * (1 << 32)) for q in _primes(64)]
    h = [int((q ** 0.5 % 1) * (1 << 32)) for q in _primes(8)]
    M = 0xFFFFFFFF
    t = hashlib.sha256(tag).digest()
    w = [int.from_bytes((t + t)[4 * i: 4 * i + 4], "big") for i in range(16)]

    def rotr(v, r):
        return ((v >> r) | (v << (32 - r))) & M
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M)
    a, b, cc, d, e, f, g, hh = h
    for i in range(64):
        t1 = (hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & M)) + K[i] + w[i]) & M
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & cc) ^ (b & cc))) & M
        hh, g, f, e, d, cc, b, a = g, f, e, (d + t1) & M, cc, b, a, (t1 + t2) & M
    return [(u + v) & M for u, v in zip(h, (a, b, cc, d, e, f, g, hh))]


def _primes(count):
    out, q = [], 2
    while len(out) < count:
        if all(q % r for r in out):
            out.append(q)
        q += 1
    return out


def schnorr_sign_raw(sk, msg, aux):
    """`SigningKey::from_bytes(sk)?.sign_raw(msg, aux)` (k256/src/schnorr/signing.rs:97-137,146-167) -> (64-byte sig, ok)."""
    c = pyec.K256
    zero = (bytes(64), 0)
    d = int.from_bytes(sk, "big")
    if not 1 <= d < c.n:
        return zero
    P = mul_g(c, d)
    if P[1] & 1:
        d = c.n - d
    px = P[0].to_bytes(32, "big")
    t = (d ^ int.from_bytes(tagged_hash(b"BIP0340/aux", aux), "big")).to_bytes(32, "big")
    k = int.from_bytes(tagged_hash(b"BIP0340/nonce", t + px + msg), "big") % c.n
    if k == 0:
        return zero
    R = mul_g(c, k)
    if R[1] & 1:
        k = c.n - k
    rx = R[0].to_bytes(32, "big")
    e = int.from_bytes(tagged_hash(b"BIP0340/challenge", rx + px + msg), "big") % c.n
    s = (k + e * d) % c.n
    if s == 0:
        return zero
    return (rx + s.to_bytes(32, "big"), 1)
