"""SM2 public-key encryption (GB/T 32918.4, the reference's `sm2::pke`) in plain Python: hashlib's SM3 and tests/pyec.py.  The model the
CPU twin (tests/hostcheck_pke) and the device (tests/test_gpu_pke.py) are compared with.

    encrypt(P, k, M) -> (C1, C2, C3) or None      C1 = k G as (x, y), C2 = M ^ KDF(x2 || y2, len M), C3 = SM3(x2 || M || y2) with
                                                  (x2, y2) = k P; None where the entry point gives ok = 0
    decrypt(d, C1, C2, C3) -> M or None
"""
import hashlib

import pyec

C = pyec.SM2
LENGTHS = [1, 31, 32, 33, 55, 56, 63, 64, 65, 96, 97, 119, 120, 128, 1000]     # KDF chunk edges, SM3 padding edges of 64 + len
ZERO_KEYSTREAM_NONCES = (115, 251, 284)      # for the reference vector's key: the first keystream byte is zero


def sm3(data):
    return hashlib.new("sm3", data).digest()


def kdf(x2, y2, length):
    """t = SM3(x2 || y2 || 1) || SM3(x2 || y2 || 2) || ... cut to `length` bytes (sm2/src/pke.rs:349-381)"""
    out = b""
    j = 1
    while len(out) < length:
        out += sm3(x2 + y2 + j.to_bytes(4, "big"))
        j += 1
    return out[:length]


def _xor(a, b):
    return bytes(p ^ q for p, q in zip(a, b))


def point_ok(P):
    return P is not None and 0 <= P[0] < C.p and 0 <= P[1] < C.p and pyec.on_curve(C, P)


def shared(k, P):
    S = pyec.mul(C, k, P)
    return S[0].to_bytes(32, "big"), S[1].to_bytes(32, "big")


def encrypt(P, k, M):
    if not (1 <= k < C.n) or not point_ok(P) or len(M) == 0:
        return None
    x2, y2 = shared(k, P)
    t = kdf(x2, y2, len(M))
    if not any(t):
        return None
    return pyec.mul(C, k, pyec.G(C)), _xor(M, t), sm3(x2 + M + y2)


def decrypt(d, C1, C2, C3):
    if not (1 <= d < C.n) or not point_ok(C1):
        return None
    x2, y2 = shared(d, C1)
    M = _xor(C2, kdf(x2, y2, len(C2)))
    return M if sm3(x2 + M + y2) == C3 else None


def enc_xy(P):
    return P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big")


def split_cipher(ct):
    """04 || C1 || C3 || C2 (Mode::C1C3C2) -> (C1, C2, C3)"""
    assert ct[0] == 4
    return (int.from_bytes(ct[1:33], "big"), int.from_bytes(ct[33:65], "big")), ct[97:], ct[65:97]
