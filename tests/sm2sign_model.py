"""Independent model of the SM2DSA signing entry points (test infrastructure): hmac / hashlib (SM3) and Python integers.

`sm2::dsa::SigningKey::sign_prehash_rfc6979` (sm2/src/dsa/signing.rs:213-258) as GB/T 32918.2 section 6.1 states it, the one
candidate of RFC 6979 section 3.2 over HMAC-SM3, and `Signer::sign` with e = SM3(Z || M).  Shares nothing with the HIP kernels.
The generator is sign_model.rfc6979_nonce — the function that reproduces the reference's RFC 6979 vectors — with the hash swapped
and cap = 1: it is not restated here.
"""
import hashlib

import pyec
import sign_model

C = pyec.SM2
N = C.n
ZERO = (bytes(64), 0)

sign_model.DIGEST.setdefault("sm2", "sm3")       # the digest SM2DSA binds to the curve (sm2/src/dsa.rs: `Sm3`)


def rfc6979_candidate(d, e):
    """The generator's first candidate for x = d (32 bytes as read) and h1 = e mod n, and whether it is in [1, n).
    The reference calls `fill_next_k` once: a rejected candidate is an error, not a reason to go on."""
    k, rejected = sign_model.rfc6979_nonce(C, d, e, cap=1)
    return k, rejected == 0 and k is not None


def finish(d, k, k_ok, e, x, r_inf=False):
    """A5-A7 from x = x(R), any value below p -> (sig = r || s as 64 bytes, ok).  k_ok: the nonce's verdict so far (the
    generator's accepted flag); r_inf: R is the identity (no k in [1, n) gives it)."""
    if not (k_ok and not r_inf and 1 <= d < N and d != N - 1 and 1 <= k < N):
        return ZERO
    r = (e % N + x % N) % N
    if r == 0 or (r + k) % N == 0:
        return ZERO
    s = pow(1 + d, -1, N) * (k - r * d) % N
    if s == 0:
        return ZERO
    return (r.to_bytes(32, "big") + s.to_bytes(32, "big"), 1)


def sign(d, k, e, R=None):
    """A3-A7 with the caller's nonce -> (sig, ok); d, k, e any 256-bit integers.
    R: k G where the caller has it already, else computed here."""
    if not 1 <= k < N:
        return ZERO
    R = sign_model.mul_g(C, k) if R is None else R
    return finish(d, k, True, e, R[0])


def edge_cases(rng):
    """(label, d, k, e) for the form with the caller's nonce: the three failures that have to be constructed (the prehash is chosen
    after the nonce), every key, nonce and prehash at the ends of its range, and sums that cross n and 2^256.  What each gives is
    the model's to say (`sign`); `fails` in the label marks the ones that must end with ok = 0."""
    rnd = lambda: rng.randrange(2, N - 1)
    x_of = lambda k: sign_model.mul_g(C, k)[0]
    out = []
    k = rnd()
    out.append(("fails: r = 0", rnd(), k, (-x_of(k)) % N))
    k = rnd()
    out.append(("fails: r + k = 0", rnd(), k, (-k - x_of(k)) % N))
    k, d = rnd(), rnd()
    r = k * pow(d, -1, N) % N
    out.append(("fails: s = 0", d, k, (r - x_of(k)) % N))
    for d in (0, N - 1, N, 2 ** 256 - 1):
        out.append(("fails: d = %x" % d, d, rnd(), rnd()))
    for k in (0, N):
        out.append(("fails: k = %x" % k, rnd(), k, rnd()))
    for k in (N - 1, 1):
        out.append(("k = %x" % k, rnd(), k, rnd()))
    for e in (0, N - 1, N, N + 1, 2 ** 256 - 1):
        out.append(("e = %x" % e, rnd(), rnd(), e))
    k = rnd()
    x = x_of(k) % N
    out.append(("e + x(R) = n + 5", rnd(), k, (N + 5 - x) % N))               # the sum crosses n
    while x <= 2 ** 256 - N:                                                  # (one x in 2^32 is that small)
        k = rnd()
        x = x_of(k) % N
    out.append(("e + x(R) >= 2^256", rnd(), k, N - 1))                         # and the word size: the carry out of the top limb
    return out


def sign_rfc6979(d, e):
    """`PrehashSigner::sign_prehash` on the prehash integer e -> (sig, ok)."""
    k, ok = rfc6979_candidate(d, e)
    if not ok:
        return ZERO
    return sign(d, k, e)


def public_key(d):
    return sign_model.mul_g(C, d)


def message_hash(distid, PA, msg):
    """e = SM3(Z || M) with Z = hash_z(distid, PA), as an integer"""
    return int.from_bytes(hashlib.new("sm3", pyec.sm2_za(C, distid, PA) + msg).digest(), "big")


def sign_msg(distid, d, msg):
    """`SigningKey::new(distid, sk)?.sign(msg)` -> (sig, ok)"""
    if not 1 <= d < N:
        return ZERO
    return sign_rfc6979(d, message_hash(distid, public_key(d), msg))
