"""X448 as the reference computes it, in Python integers: the clamp (x448/src/lib.rs:122-126), the ladder of
`&MontgomeryPoint * &EdwardsScalar` with its step `differential_add_and_double` (ed448-goldilocks/src/montgomery.rs:83-110,168-204),
`to_affine` with invert(0) = 0 (:216-219) and the byte-wise low-order rule of `x448()` (lib.rs:152-156).  Records are 56 bytes,
little-endian.  The model of tests/test_x448_model.py, of the g++ twin (tests/test_hostcheck_x448.py) and of the GPU tests."""

P = 2 ** 448 - 2 ** 224 - 1
A24 = 39082                                   # A_PLUS_TWO_OVER_FOUR, A = 156326
A = 156326
BASE_U = 5
ZERO = bytes(56)
LOW_ORDER = (bytes(56), (1).to_bytes(56, "little"), (P - 1).to_bytes(56, "little"))


def le(v):
    return int(v).to_bytes(56, "little")


def clamp(scalar):
    b = bytearray(scalar)
    assert len(b) == 56
    b[0] &= 252
    b[55] |= 128
    return int.from_bytes(b, "little")


def step(p, q, u):
    (pu, pw), (qu, qw) = p, q
    t0, t1, t2, t3 = pu + pw, pu - pw, qu + qw, qu - qw
    t4, t5 = t0 * t0 % P, t1 * t1 % P
    t6 = t4 - t5
    t7, t8 = t0 * t3 % P, t1 * t2 % P
    t9, t10 = t7 + t8, t7 - t8
    t13 = A24 * t6
    return (t4 * t5 % P, t6 * (t13 + t5) % P), (t9 * t9 % P, u * t10 * t10 % P)


def ladder(k, u):
    """k: the 448-bit integer as it is used; u: any integer (taken mod p) -> the canonical result"""
    u %= P
    x0, x1, swap = (1, 0), (u, 1), 0
    for s in range(447, -1, -1):
        bit = (k >> s) & 1
        if swap ^ bit:
            x0, x1 = x1, x0
        x0, x1 = step(x0, x1, u)
        swap = bit
    # no final swap: bit 0 of a clamped scalar is 0
    return x0[0] * pow(x0[1], P - 2, P) % P


def x448_unchecked(scalar, point):
    return le(ladder(clamp(scalar), int.from_bytes(point, "little")))


def x448(scalar, point):
    """-> (record, ok): refused exactly when the point's bytes are one of the three low-order records"""
    if bytes(point) in LOW_ORDER:
        return ZERO, 0
    return x448_unchecked(scalar, point), 1


def public_key(scalar):
    return x448_unchecked(scalar, le(BASE_U))


def on_curve(u):
    """whether u is the coordinate of a point of Curve448 (not of its twist): u^3 + A u^2 + u is a square"""
    v = (u * u * u + A * u * u + u) % P
    return v == 0 or pow(v, (P - 1) // 2, P) == 1


# u records every layer is asked about: label -> bytes
SPECIAL_U = {
    "0": le(0), "1": le(1), "p-1": le(P - 1), "p": le(P), "p+1": le(P + 1), "2^224-1": le(2 ** 224 - 1), "2^224": le(2 ** 224),
    "2^224+1": le(2 ** 224 + 1), "2^448-1": le(2 ** 448 - 1), "5": le(5), "2": le(2), "p-2": le(P - 2),
}
# the five inputs whose product is the zero record; the first three are the ones `x448()` refuses
ZERO_PRODUCT = ("0", "1", "p-1", "p", "p+1")


def twist_u(rng):
    while True:
        u = rng.randrange(2, P)
        if not on_curve(u):
            return le(u)
