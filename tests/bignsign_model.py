"""Independent model of the bign signing entry points (test infrastructure): pyec's belt-block / belt-hash and Python integers.

`bignp256::ecdsa::SigningKey::sign_prehash` (bignp256/src/ecdsa/signing.rs:110-161) with the nonce generator of STB 34.101.45
section 6.3.3 (the un-vendored `bign_genk::KGenerator<BeltBlock>`), restated here for l = 128 and pinned by the reference's own
signature vector (bignp256/tests/ecdsa.rs:20-33): that vector is the deterministic signature.  Shares nothing with the HIP kernels.
All byte strings as they lie, all integers little-endian.
"""
import pyec

C = pyec.BIGN256
Q = C.n
ZERO = (bytes(48), 0)
TWO128 = 1 << 128
MAX_ROUNDS = 4096                   # a guard for the model's loop only: with the real q the first candidate (round 4) is accepted


def le(v, n=32):
    return v.to_bytes(n, "little")


def theta(d_bytes):
    """theta = belt-hash(OID(h) || <d>_256 || t), t empty; d as its 32 bytes lie"""
    return pyec.belt_hash(pyec.BELT_OID + d_bytes)


def genk(d_bytes, h_bytes, bound=Q, max_rounds=MAX_ROUNDS):
    """The generator on the 32 bytes it is given -> (k, rounds); k = None if no candidate up to max_rounds is in (0, bound).
    d_bytes: the key as 32 bytes; h_bytes: r1 || r2 (the REDUCED prehash in the signer)."""
    th = theta(d_bytes)
    r1, r2 = h_bytes[:16], h_bytes[16:]
    for i in range(1, max_rounds + 1):
        s = r1
        r1 = pyec._bxor(pyec._bxor(pyec.belt_block(s, th), r2), le(i, 16))
        r2 = s
        if i % 4 == 0:
            k = int.from_bytes(r1 + r2, "little")
            if 0 < k < bound:
                return k, i
    return None, max_rounds


def nonce(d, h_raw, reduce_h=True):
    """the signer's nonce: the generator is fed the prehash REDUCED mod q (signing.rs:117-123).  reduce_h = False is the other
    reading (raw bytes), kept so that a test can tell the two apart."""
    hb = le(int.from_bytes(h_raw, "little") % Q) if reduce_h else h_raw
    return genk(le(d), hb)[0]


def finish(d, k, k_ok, h_raw, s0):
    """S1 and the verdict from S0 (16 bytes, any value) -> (sig, ok)"""
    s0i = int.from_bytes(s0, "little")
    if not (k_ok and 1 <= d < Q and 1 <= k < Q and s0i != 0):
        return ZERO
    s1 = (k - int.from_bytes(h_raw, "little") - (s0i + TWO128) * d) % Q
    if s1 == 0:
        return ZERO
    return (s0 + le(s1), 1)


def s0_of(k, h_raw):
    """S0 = belt-hash(OID || <x(R)>_256 || raw prehash)[..16], R = k G"""
    R = pyec.mul(C, k, pyec.G(C))
    return pyec.belt_hash(pyec.BELT_OID + le(R[0]) + h_raw)[:16]


def sign(d, k, h_raw):
    """steps 3-7 with the caller's nonce -> (sig, ok); d, k any 256-bit integers, h_raw 32 bytes"""
    if not (1 <= k < Q and 1 <= d < Q):
        return ZERO
    sig = pyec.bign_sign(C, d, h_raw, k)
    out = finish(d, k, True, h_raw, sig[:16])
    assert out == ZERO or out[0] == sig
    return out


def sign_prehash(d, h_raw, reduce_h=True):
    """`PrehashSigner::sign_prehash` -> (sig, ok)"""
    if not 1 <= d < Q:
        return ZERO
    return sign(d, nonce(d, h_raw, reduce_h), h_raw)


def sign_msg(d, msg):
    """`Signer::try_sign` -> (sig, ok)"""
    return sign_prehash(d, pyec.belt_hash(msg))


def public_key(d):
    return pyec.mul(C, d, pyec.G(C))


PREHASH_GE_Q = [b"\xff" * 32, le(Q), le(Q + 1)]


def s1_zero_case(rng):
    """(d, k, h_raw) with S1 = 0: fix k and H, compute S0, solve d = (k - H)(S0 + 2^128)^-1"""
    while True:
        k, h_raw = rng.randrange(1, Q), le(rng.getrandbits(256))
        s0 = int.from_bytes(s0_of(k, h_raw), "little")
        d = (k - int.from_bytes(h_raw, "little")) * pow(s0 + TWO128, -1, Q) % Q
        if d:
            return d, k, h_raw


def refusals(rng):
    """(label, d, k, h_raw) for the caller's-nonce form, each refused (S0 = 0 cannot be constructed: it is handed to the finish
    step directly)"""
    rnd = lambda: rng.randrange(1, Q)
    rh = lambda: le(rng.getrandbits(256))
    out = [("d = 0", 0, rnd(), rh()), ("d = q", Q, rnd(), rh()), ("d = q - 1 + 1 (wire: q)", Q - 1 + 1, rnd(), rh()),
           ("d = 2^256 - 1", 2 ** 256 - 1, rnd(), rh()), ("k = 0", rnd(), 0, rh()), ("k = q", rnd(), Q, rh())]
    d, k, h = s1_zero_case(rng)
    out.append(("S1 = 0", d, k, h))
    return out
