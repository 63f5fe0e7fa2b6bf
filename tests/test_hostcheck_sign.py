"""The signing code of csrc/ecgpu_sign.h compiled for the CPU (tests/hostcheck_sign) against tests/sign_model.py: the RFC 6979
generator with its retries and its candidate cap, the ECDSA and BIP340 finish steps, the message hashing — on every parameter set
the entry points support.  The multiplications by the generator in between are the CPU build of fixed_base_mul_ct (tests/hostcheck),
the algorithm the signing entry points launch.  CPU only."""
import ctypes
import fcntl
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import hostcheck_lib
import pyec
import sign_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostcheck_sign")
SRC = os.path.join(HERE, "hostcheck_sign.cpp")
LIB = os.path.join(HERE, "libhostcheck_sign.so")
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")
_u8p = ctypes.POINTER(ctypes.c_uint8)
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in ("ecgpu_sign.h", "ecgpu_hash.h", "ecgpu_sha256.h", "ecgpu_scalar.h",
                                                        "ecgpu_modinv.h", "ecgpu_params.h")]

        def fresh():
            return os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps)
        with open(LIB + ".lock", "w") as lock:               # pytest-xdist workers arrive together: one builds, the others wait
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not fresh():
                tmp = LIB + ".tmp.%d" % os.getpid()
                subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                                       "-o", tmp, SRC])
                os.replace(tmp, LIB)
        _lib = ctypes.CDLL(LIB)
    return _lib


def _a(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy() if len(b) else np.zeros(1, np.uint8)


def _p(a):
    return a.ctypes.data_as(_u8p)


def twin_rfc6979(c, d, z, cap=sm.MAX_CANDIDATES):
    n = len(d) // c.L
    D, Z, k, tried = _a(d), _a(z), np.zeros(n * c.L, np.uint8), np.zeros(n, np.int32)
    assert lib().hs_rfc6979(c.cid, _p(D), _p(Z), ctypes.c_size_t(n), cap, _p(k), tried.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0
    return bytes(k), tried


def twin_nonce_load(c, k):
    n = len(k) // c.L
    K, out, flag = _a(k), np.zeros(n * c.L, np.uint8), np.zeros(n, np.uint8)
    assert lib().hs_nonce_load(c.cid, _p(K), ctypes.c_size_t(n), _p(out), _p(flag)) == 0
    return bytes(out), flag


def twin_finish(c, d, k, flag, z, rxy, rinf, normalize_s):
    n = len(d) // c.L
    sig, recid, ok = np.zeros(n * 2 * c.L, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    args = [_a(v) for v in (d, k, flag, z, rxy, rinf)]
    assert lib().hs_ecdsa_sign_finish(c.cid, *[_p(v) for v in args], ctypes.c_size_t(n), int(normalize_s), _p(sig), _p(recid), _p(ok)) == 0
    return bytes(sig), recid, ok


def twin_sign(c, d, k, flag, z, normalize_s):
    """k: sanitised nonces; the whole path of the entry points after the nonce."""
    rc, rxy, rinf = hostcheck_lib.batch_mul_base_ct(c.cid, k)
    assert rc == 0
    return twin_finish(c, d, k, flag, z, rxy, rinf, normalize_s)


def enc(c, values):
    return b"".join(v.to_bytes(c.L, "big") for v in values)


def edge_values(c):
    return [0, 1, c.n - 1, c.n, 2 ** (8 * c.L) - 1]


@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_caller_nonce_form(name):
    c = pyec.CURVES[name]
    rng = random.Random("sign-twin-" + name)
    ds = edge_values(c) + [rng.randrange(1, c.n) for _ in range(7)]
    ks = [rng.randrange(1, c.n) for _ in range(5)] + edge_values(c) + [rng.randrange(1, c.n), 5]
    zs = [0, c.n, 2 ** (8 * c.L) - 1] + [rng.getrandbits(8 * c.L) for _ in range(9)]
    d, k, z = enc(c, ds), enc(c, ks), enc(c, zs)
    ksafe, flag = twin_nonce_load(c, k)
    assert list(flag) == [int(1 <= v < c.n) for v in ks]
    assert ksafe == enc(c, [v if 1 <= v < c.n else 1 for v in ks])
    for normalize_s in (0, 1):
        sig, recid, ok = twin_sign(c, d, ksafe, flag, z, normalize_s)
        for i in range(len(ds)):
            want = sm.ecdsa_sign(c, ds[i], ks[i], zs[i], normalize_s)
            assert (sig[i * 2 * c.L:(i + 1) * 2 * c.L], int(recid[i]), int(ok[i])) == want, (name, i, normalize_s)
        assert [int(v) for v in ok] == [0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 1, 1]                  # a bad element leaves its neighbours alone


@pytest.mark.parametrize("name", sm.RFC6979_SETS)
def test_rfc6979_nonces_and_signatures(name):
    c = pyec.CURVES[name]
    rng = random.Random("rfc6979-twin-" + name)
    n = 160
    ds = [rng.randrange(1, c.n) for _ in range(n)]
    zs = [rng.getrandbits(8 * c.L) for _ in range(n)]
    ds[:3] = [1, c.n - 1, 2]
    zs[:3] = [0, c.n, 2 ** (8 * c.L) - 1]
    d, z = enc(c, ds), enc(c, zs)
    k, tried = twin_rfc6979(c, d, z)
    want = [sm.rfc6979_nonce(c, ds[i], zs[i]) for i in range(n)]
    assert k == enc(c, [w[0] for w in want])
    assert list(tried) == [w[1] + 1 for w in want]
    if name.startswith("bp"):
        # the brainpool orders sit well below 2^(8 L): these inputs must exercise the retry loop, several times in a row
        assert max(w[1] for w in want) >= 3, max(w[1] for w in want)
        assert sum(1 for w in want if w[1]) >= n // 5
    pick = list(range(12)) + [i for i in range(n) if want[i][1] >= 3][:4]
    sub = lambda b, w: b"".join(b[i * w:(i + 1) * w] for i in pick)
    for normalize_s in (0, 1):
        sig, recid, ok = twin_sign(c, sub(d, c.L), sub(k, c.L), bytes([1] * len(pick)), sub(z, c.L), normalize_s)
        for j, i in enumerate(pick):
            got = (sig[j * 2 * c.L:(j + 1) * 2 * c.L], int(recid[j]), int(ok[j]))
            assert got == sm.ecdsa_sign_rfc6979(c, ds[i], zs[i], normalize_s), (name, i)


@pytest.mark.parametrize("name", ["bp256", "bp384t1"])
def test_candidate_cap(name):
    """The 128-candidate cap through a lower one: an element that needs more candidates than the cap allows gets ok = 0 (k = 1 goes
    to the multiplication, the flag stays clear), one that needs exactly the cap is signed."""
    c = pyec.CURVES[name]
    rng = random.Random("cap-" + name)
    ds = [rng.randrange(1, c.n) for _ in range(200)]
    zs = [rng.getrandbits(8 * c.L) for _ in range(200)]
    rej = [sm.rfc6979_nonce(c, a, b)[1] for a, b in zip(ds, zs)]
    assert max(rej) >= 3
    d, z = enc(c, ds), enc(c, zs)
    for cap in (1, 2, 3, max(rej) + 1):
        k, tried = twin_rfc6979(c, d, z, cap)
        assert list(tried) == [r + 1 if r < cap else 0 for r in rej], cap
        flag = bytes(int(t != 0) for t in tried)
        for i in range(200):
            if rej[i] >= cap:
                assert k[i * c.L:(i + 1) * c.L] == (1).to_bytes(c.L, "big")
        some = [i for i in range(200) if rej[i] >= cap][:3] + [i for i in range(200) if rej[i] == cap - 1][:3]
        sub = lambda b, w: b"".join(b[i * w:(i + 1) * w] for i in some)
        sig, recid, ok = twin_sign(c, sub(d, c.L), sub(k, c.L), sub(flag, 1), sub(z, c.L), 0)
        for j, i in enumerate(some):
            assert (sig[j * 2 * c.L:(j + 1) * 2 * c.L], int(recid[j]), int(ok[j])) == sm.ecdsa_sign_rfc6979(c, ds[i], zs[i], 0, cap=cap)


@pytest.mark.parametrize("name", ["k256", "p256", "p224", "bp256", "p384"])
def test_recid_bit_1_from_a_forged_x(name):
    """x(R) >= n needs an x in [n, p), a 2^-128 event on these curves that no findable nonce reaches; the finish step is fed such an x
    directly (with any y: the step reads its parity only).  p521 and the sets with p < n have no such x at all."""
    c = pyec.CURVES[name]
    assert c.n < c.p
    rng = random.Random("recid-" + name)
    d, k, z = rng.randrange(1, c.n), rng.randrange(1, c.n), rng.getrandbits(8 * c.L)
    for x, y in ((c.n, 2), (c.n + 1, 3), (c.p - 1, 4), (c.n - 1, 5)):
        for normalize_s in (0, 1):
            sig, recid, ok = twin_finish(c, enc(c, [d]), enc(c, [k]), b"\x01", enc(c, [z]), enc(c, [x, y]), b"\x00", normalize_s)
            r = x % c.n
            s = pow(k, -1, c.n) * (z % c.n + r * d) % c.n
            rid = (y & 1) | (2 if x >= c.n else 0)
            if normalize_s and s > (c.n - 1) // 2:
                s, rid = c.n - s, rid ^ 1
            if r == 0:
                assert int(ok[0]) == 0 and sig == bytes(2 * c.L) and int(recid[0]) == 0         # x = n: r = 0
            else:
                assert (sig, int(recid[0]), int(ok[0])) == (enc(c, [r, s]), rid, 1), (name, x)


@pytest.mark.parametrize("name", sm.RFC6979_SETS)
def test_message_hash(name):
    c = pyec.CURVES[name]
    rng = random.Random("hash-" + name)
    for msg_len in (0, 1, 55, 56, 64, 111, 112, 128, 200):
        msgs = [bytes(rng.getrandbits(8) for _ in range(msg_len)) for _ in range(3)]
        M, out = _a(b"".join(msgs)), np.zeros(3 * c.L, np.uint8)
        assert lib().hs_hash_msg(c.cid, _p(M), ctypes.c_size_t(msg_len), ctypes.c_size_t(3), _p(out)) == 0
        want = b"".join(sm.bits2field(c, hashlib.new(sm.DIGEST[name], m).digest()).to_bytes(c.L, "big") for m in msgs)
        assert bytes(out) == want, msg_len


def test_unsupported_sets():
    k, t = np.zeros(32, np.uint8), np.zeros(1, np.int32)
    for cid in (pyec.P192.cid,):
        assert lib().hs_rfc6979(cid, _p(k), _p(k), ctypes.c_size_t(0), 128, _p(k), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -2
    for cid in (pyec.SM2.cid, pyec.BIGN256.cid):
        assert lib().hs_nonce_load(cid, _p(k), ctypes.c_size_t(0), _p(k), _p(k)) == -1


def twin_schnorr(sks, msgs, msg_len, auxs):
    c = pyec.K256
    n = len(sks)
    sk, aux, M = _a(b"".join(sks)), _a(b"".join(auxs)), _a(b"".join(msgs))
    dsafe, dflag = twin_nonce_load(c, bytes(sk))
    rc, pxy, pinf = hostcheck_lib.batch_mul_base_ct(0, dsafe)
    assert rc == 0 and not pinf.any()
    dp, k, flag = np.zeros(64 * n, np.uint8), np.zeros(32 * n, np.uint8), np.zeros(n, np.uint8)
    assert lib().hs_schnorr_nonce(_p(sk), _p(pxy), _p(aux), _p(M), ctypes.c_size_t(msg_len), ctypes.c_size_t(n), _p(dp), _p(k), _p(flag)) == 0
    assert list(flag) == list(dflag)
    rc, rxy, rinf = hostcheck_lib.batch_mul_base_ct(0, bytes(k))
    assert rc == 0
    sig, ok = np.zeros(64 * n, np.uint8), np.zeros(n, np.uint8)
    assert lib().hs_schnorr_sign_finish(_p(dp), _p(k), _p(flag), _p(rxy), _p(_a(bytes(rinf))), _p(M), ctypes.c_size_t(msg_len),
                                        ctypes.c_size_t(n), _p(sig), _p(ok)) == 0
    return bytes(sig), ok


@pytest.mark.parametrize("msg_len", [0, 1, 23, 32, 55, 56, 64, 100])
def test_schnorr_sign(msg_len):
    c = pyec.K256
    rng = random.Random(1000 + msg_len)
    rb = lambda m: bytes(rng.getrandbits(8) for _ in range(m))
    sks = [v.to_bytes(32, "big") for v in (0, 1, c.n - 1, c.n, 2 ** 256 - 1, 3)] + [rb(32) for _ in range(6)]
    msgs = [rb(msg_len) for _ in sks]
    auxs = [bytes(32), b"\xff" * 32] + [rb(32) for _ in sks[2:]]
    sig, ok = twin_schnorr(sks, msgs, msg_len, auxs)
    for i in range(len(sks)):
        assert (sig[64 * i:64 * i + 64], int(ok[i])) == sm.schnorr_sign_raw(sks[i], msgs[i], auxs[i]), i
    assert [int(v) for v in ok[:6]] == [0, 1, 1, 0, 0, 1]
