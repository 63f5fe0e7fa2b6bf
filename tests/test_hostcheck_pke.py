"""The SM2 public-key encryption code of csrc/ecgpu_pke.h compiled for the CPU (tests/hostcheck_pke) against tests/pke_model.py: the
lane bodies of k_pke_load / k_pke_point, k_pke_seal and k_pke_open on the reference's vectors and on 200 random elements per message
length.  The multiplications in between are the CPU build of the `_ct` algorithms (tests/hostcheck), cross-checked with pyec on a few
elements.  The same source with its own main is built with AddressSanitizer + UBSan as a stand-alone program and run once over the
vector and the boundary lengths.  CPU only."""
import ctypes
import fcntl
import json
import os
import random
import subprocess

import numpy as np
import pytest

import hostcheck_lib
import pke_model as pm
import pyec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostcheck_pke")
SRC = os.path.join(HERE, "hostcheck_pke.cpp")
LIB = os.path.join(HERE, "libhostcheck_pke.so")
PROG = os.path.join(HERE, "hostcheck_pke_san")
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("ecgpu_pke.h", "ecgpu_sm3.h", "ecgpu_hash.h", "ecgpu_sign.h", "ecgpu_verify.h",
                                                "ecgpu_scalar.h", "ecgpu_point.h", "ecgpu_field.h", "ecgpu_params.h")]
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "sm2pke.json")))
D = int(VEC["private_key"], 16)
MSG = bytes.fromhex(VEC["msg"])
SM2 = pyec.SM2.cid
_u8p = ctypes.POINTER(ctypes.c_uint8)
_lib = None


def _build(target, flags):
    def fresh():
        return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in DEPS)
    with open(target + ".lock", "w") as lock:               # pytest-xdist workers arrive together: one builds, the others wait
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            tmp = target + ".tmp.%d" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + flags + ["-o", tmp, SRC])
            os.replace(tmp, target)


def lib():
    global _lib
    if _lib is None:
        _build(LIB, ["-O2", "-fPIC", "-shared"])
        _lib = ctypes.CDLL(LIB)
    return _lib


def _a(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(4, np.uint8)


def _p(a):
    return a.ctypes.data_as(_u8p)


def _sz(v):
    return ctypes.c_size_t(v)


def twin_load(scalars, points):
    n = len(scalars) // 32
    S, P = _a(scalars), _a(points)
    so, po, flag = np.zeros(n * 32, np.uint8), np.zeros(n * 64, np.uint8), np.zeros(n, np.uint8)
    assert lib().hp_load(_p(S), _p(P), _sz(n), _p(so), _p(po), _p(flag)) == 0
    return bytes(so), bytes(po), flag


def twin_seal(x2y2, flag, msgs, msg_len, c1):
    n = len(x2y2) // 64
    X, F, M, C1 = _a(x2y2), _a(bytes(flag)), _a(msgs), _a(c1)
    c2, c3, ok = np.zeros(max(n * msg_len, 4), np.uint8), np.zeros(n * 32, np.uint8), np.zeros(n, np.uint8)
    assert lib().hp_seal(_p(X), _p(F), _p(M), _sz(msg_len), _sz(n), _p(C1), _p(c2), _p(c3), _p(ok)) == 0
    return bytes(C1), bytes(c2[:n * msg_len]), bytes(c3), ok


def twin_open(x2y2, flag, c2, msg_len, c3):
    n = len(x2y2) // 64
    X, F, C2, C3 = _a(x2y2), _a(bytes(flag)), _a(c2), _a(c3)
    out, ok = np.full(max(n * msg_len, 4), 0xEE, np.uint8), np.zeros(n, np.uint8)
    assert lib().hp_open(_p(X), _p(F), _p(C2), _sz(msg_len), _p(C3), _sz(n), _p(out), _p(ok)) == 0
    return bytes(out[:n * msg_len]), ok


def enc32(values):
    return b"".join(v.to_bytes(32, "big") for v in values)


def test_reference_cipher_through_the_twin():
    C1, C2, C3 = pm.split_cipher(bytes.fromhex(VEC["cipher"]))
    d, c1, flag = twin_load(enc32([D]), pm.enc_xy(C1))
    assert (d, c1, list(flag)) == (enc32([D]), pm.enc_xy(C1), [1])
    rc, xy, inf = hostcheck_lib.batch_mul_ct(SM2, d, c1)
    assert rc == 0 and not inf.any() and bytes(xy) == b"".join(pm.shared(D, C1))
    m, ok = twin_open(bytes(xy), flag, C2, len(C2), C3)
    assert (m, list(ok)) == (MSG, [1])
    # and back: sealing MSG under the same shared point gives the vector's C2 and C3
    _, c2, c3, ok = twin_seal(bytes(xy), flag, MSG, len(MSG), pm.enc_xy(C1))
    assert (c2, c3, list(ok)) == (C2, C3, [1])


def test_load_sanitises_scalars_and_points():
    c = pm.C
    G, Q = pyec.G(c), pyec.mul(c, D, pyec.G(c))
    ks = [0, 1, c.n - 1, c.n, 2 ** 256 - 1, 5, 5, 5, 5]
    pts = [Q] * 5 + [Q, (Q[0], Q[1] ^ 1), (c.p, Q[1]), (Q[0], c.p + 1)]
    s, p, flag = twin_load(enc32(ks), b"".join(pm.enc_xy(P) for P in pts))
    assert list(flag) == [0, 1, 1, 0, 0, 1, 0, 0, 0]
    assert s == enc32([k if 1 <= k < c.n else 1 for k in ks])
    assert p == b"".join(pm.enc_xy(P if pm.point_ok(P) else G) for P in pts)


@pytest.mark.parametrize("msg_len", pm.LENGTHS)
def test_seal_and_open_200_random_elements(msg_len):
    c = pm.C
    n = 200
    rng = random.Random("pke-twin-%d" % msg_len)
    ds = [rng.randrange(1, c.n) for _ in range(n)]
    ks = [rng.randrange(1, c.n) for _ in range(n)]
    rc, pk, inf = hostcheck_lib.batch_mul_base_ct(SM2, enc32(ds))
    assert rc == 0 and not inf.any()
    rc, xy, inf = hostcheck_lib.batch_mul_ct(SM2, enc32(ks), bytes(pk))
    assert rc == 0 and not inf.any()
    xy = bytes(xy)
    for i in (0, n - 1):                                                          # the CPU multiplications against pyec
        P = (int.from_bytes(pk[64 * i:64 * i + 32], "big"), int.from_bytes(pk[64 * i + 32:64 * i + 64], "big"))
        assert xy[64 * i:64 * i + 64] == b"".join(pm.shared(ks[i], P))
    msgs = bytes(rng.getrandbits(8) for _ in range(n * msg_len))
    flag = [1] * n
    flag[3] = flag[n - 2] = 0                                                     # an element the load step rejected
    c1_in = bytes(rng.getrandbits(8) for _ in range(n * 64))
    c1, c2, c3, ok = twin_seal(xy, flag, msgs, msg_len, c1_in)
    # (at msg_len = 1 one keystream in 256 is all zero: such an element is a rejected one too)
    flag = [int(f and any(pm.kdf(xy[64 * i:64 * i + 32], xy[64 * i + 32:64 * i + 64], msg_len))) for i, f in enumerate(flag)]
    assert list(ok) == flag and sum(flag) >= n - 8
    for i in range(n):
        x2, y2, M = xy[64 * i:64 * i + 32], xy[64 * i + 32:64 * i + 64], msgs[i * msg_len:(i + 1) * msg_len]
        got = (c1[64 * i:64 * i + 64], c2[i * msg_len:(i + 1) * msg_len], c3[32 * i:32 * i + 32])
        if flag[i]:
            t = pm.kdf(x2, y2, msg_len)
            assert got == (c1_in[64 * i:64 * i + 64], bytes(a ^ b for a, b in zip(M, t)), pm.sm3(x2 + M + y2)), i
        else:
            assert got == (bytes(64), bytes(msg_len), bytes(32)), i
    # open: good elements give the message back; one flipped bit in C2 resp. C3, and the rejected elements, give a zero record
    bad2, bad3 = bytearray(c2), bytearray(c3)
    bad2[7 * msg_len + msg_len - 1] ^= 0x80
    bad3[9 * 32 + 31] ^= 1
    for cc2, cc3, dead in ((c2, c3, set()), (bytes(bad2), c3, {7}), (c2, bytes(bad3), {9})):
        m, ok = twin_open(xy, [1] * n, cc2, msg_len, cc3)
        for i in range(n):
            alive = flag[i] and i not in dead
            assert int(ok[i]) == int(alive), i
            assert m[i * msg_len:(i + 1) * msg_len] == (msgs[i * msg_len:(i + 1) * msg_len] if alive else bytes(msg_len)), i
    m, ok = twin_open(xy, [0] * n, c2, msg_len, c3)
    assert not ok.any() and m == bytes(n * msg_len)


def test_zero_keystream_and_empty_message():
    c = pm.C
    Q = pyec.mul(c, D, pyec.G(c))
    for k in pm.ZERO_KEYSTREAM_NONCES:
        xy = b"".join(pm.shared(k, Q))
        assert pm.kdf(xy[:32], xy[32:], 1) == b"\x00"
        c1, c2, c3, ok = twin_seal(xy, [1], b"\x5a", 1, bytes(range(64)))
        assert (c1, c2, c3, list(ok)) == (bytes(64), b"\x00", bytes(32), [0])          # the caller draws another k
        m, ok = twin_open(xy, [1], b"\x5a", 1, pm.sm3(xy[:32] + b"\x5a" + xy[32:]))       # a model-built ciphertext with t = 0 opens
        assert (m, list(ok)) == (b"\x5a", [1])
        _, c2, c3, ok = twin_seal(xy, [1], b"\x5a\xa5", 2, bytes(64))
        assert list(ok) == [1] and c2[0] == 0x5a
    xy = b"".join(pm.shared(7, Q))
    m, ok = twin_open(xy, [1], b"", 0, pm.sm3(xy))
    assert list(ok) == [1]
    m, ok = twin_open(xy, [1], b"", 0, pm.sm3(xy + b"\x00"))
    assert list(ok) == [0]


def test_sanitized_standalone_program(tmp_path):
    """AddressSanitizer + UBSan on the lane bodies, every buffer exactly its record's size: the vector and the boundary lengths"""
    # (the runtimes linked into the program itself: it needs no preload and does not mind what else the process environment loads)
    _build(PROG, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                  "-DHOSTCHECK_PKE_MAIN"])
    c = pm.C
    rng = random.Random("pke-san")
    C1v, C2v, C3v = pm.split_cipher(bytes.fromhex(VEC["cipher"]))
    Q = pyec.mul(c, D, pyec.G(c))
    rows = []                                                                             # (scalar, point, message)
    rows.append((rng.randrange(1, c.n), Q, MSG))
    for msg_len in pm.LENGTHS:
        rows.append((rng.randrange(1, c.n), Q, bytes(rng.getrandbits(8) for _ in range(msg_len))))
    rows.append((0, Q, b"abc"))
    rows.append((5, (Q[0], Q[1] ^ 1), b"abcd"))
    rows.append((pm.ZERO_KEYSTREAM_NONCES[0], Q, b"\x33"))
    lines, want = [], []
    for k, P, M in rows:
        good = 1 <= k < c.n and pm.point_ok(P)
        ks, Ps = (k if 1 <= k < c.n else 1), (P if pm.point_ok(P) else pyec.G(c))
        x2, y2 = pm.shared(ks, Ps)
        lines.append("%s %s %s %s" % (k.to_bytes(32, "big").hex(), pm.enc_xy(P).hex(), (x2 + y2).hex(), M.hex() or "-"))
        t = pm.kdf(x2, y2, len(M))
        ok = good and any(t)
        hx = lambda b: b.hex() or "-"
        want.append(" s=%s p=%s flag=%02x c1=%s c2=%s c3=%s ok=%02x m=%s ok2=%02x" % (
            ks.to_bytes(32, "big").hex(), pm.enc_xy(Ps).hex(), int(good), hx(pm.enc_xy(P) if ok else bytes(64)),
            hx(bytes(a ^ b for a, b in zip(M, t)) if ok else bytes(len(M))), hx(pm.sm3(x2 + M + y2) if ok else bytes(32)), int(ok),
            hx(M if ok else bytes(len(M))), int(ok)))
    path = tmp_path / "rows.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([PROG, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == want
