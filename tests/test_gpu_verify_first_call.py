"""-m gpu: every verification / recovery `_dev` entry point as the FIRST call of a fresh context.

A scheme states its own scratch reservations (csrc/ecgpu_api.hip, the scheme functions around verify_pipeline).  A buffer a scheme
forgot is invisible whenever an earlier call on the same context has already grown it, and the other suites share one engine per
module — so here each entry point gets a context of its own, and one further context runs all of them queued behind each other, in
an order in which a scheme that needs more follows one that needs less.

N = 257: one workgroup plus one element (the NB of test_gpu_timing_spans.py).  k256 for ECDSA / recovery / BIP340, the three ECDSA
forms again on p384 (48-byte records: buffers of another size than every 32-byte scheme), sm2 for SM2DSA, bign256 for bign.  The
elements are signatures by the big-integer models (pyec, sign_model) over a handful of keys, repeated; elements 0, 255 and 256 have
a bit of s flipped, element 128 has a public key that is not on the curve.  Public-key recovery takes no key and recovers SOME key
from any (z, r, s) in range, so there the flipped bit is the top one under reject_high_s (the signatures are low-S), and element 128
has an r that is no x coordinate of the curve.  Expected verdicts (and recovered keys) are the models', element by element."""
import ctypes
import functools
import hashlib
import random

import numpy as np
import pytest

import pyec
import sign_model as sm
from gpu_common import bip340_challenge, ecgpu_module

pytestmark = pytest.mark.gpu
N = 257
BAD_S, BAD_KEY = (0, 255, 256), 128
POOL = 5                              # distinct signers; element i is signer i % POOL (the model runs once per distinct element)
MSG_LEN = 40
DISTID = b"1234567812345678"
S, I = ctypes.c_size_t, ctypes.c_int


class Case:
    """fn(ctx, *lead, *inputs, n, *tail, [keys,] verdicts): inputs are the host arrays in the entry point's argument order (ctypes
    scalars pass through), exp_xy the key records of the recovery (empty: the entry point has no such output)"""
    def __init__(self, fn, inputs, exp_ok, lead=(), tail=(), exp_xy=b""):
        self.fn, self.inputs, self.lead, self.tail = fn, inputs, lead, tail
        self.exp_ok, self.exp_xy = bytes(exp_ok), bytes(exp_xy)
        assert len(self.exp_ok) == N and all(self.exp_ok[i] == 0 for i in BAD_S + (BAD_KEY,)) and sum(self.exp_ok) == N - 4


def _rng(tag):
    return random.Random("verify-first-call-" + tag)


def _flip(buf, at, bit=1):
    buf[at] ^= bit


def _off_curve_x(c, rng):
    x = rng.randrange(1, min(c.n, c.p))
    while pyec.lift_x(c, x, 0) is not None:
        x += 1
    return x


def _ints(c, rec, order="big"):
    L = len(rec) // 2
    return (int.from_bytes(rec[:L], order), int.from_bytes(rec[L:], order))


def _ecdsa_pool(c, rng, msg=False):
    """POOL x (z bytes or message, r || s, key record, recid) — low-S signatures by sign_model"""
    out = []
    while len(out) < POOL:
        d, k = rng.randrange(1, c.n), rng.randrange(1, c.n)
        m = bytes(rng.randrange(256) for _ in range(MSG_LEN if msg else c.L))
        z = sm.bits2field(c, hashlib.new(sm.DIGEST[c.name], m).digest()) if msg else int.from_bytes(m, "big")
        sig, recid, ok = sm.ecdsa_sign(c, d, k, z, True)
        if ok and recid < 2:
            out.append((m, sig, pyec.enc_point(c, sm.mul_g(c, d))[0], recid))
    return out


def _z_of(c, m, msg):
    return sm.bits2field(c, hashlib.new(sm.DIGEST[c.name], m).digest()) if msg else int.from_bytes(m, "big")


def _ecdsa_verify_case(curve, msg):
    c = pyec.CURVES[curve]
    L = c.L
    pool = _ecdsa_pool(c, _rng("ecdsa" + curve + str(msg)), msg)
    m, sig, q = (bytearray(b"".join(pool[i % POOL][k] for i in range(N))) for k in range(3))
    for i in BAD_S:
        _flip(sig, i * 2 * L + 2 * L - 1)
    _flip(q, BAD_KEY * 2 * L + 2 * L - 1)
    ml = len(pool[0][0])

    @functools.lru_cache(None)
    def model(mi, si, qi):
        return pyec.ecdsa_verify(c, _ints(c, qi), _z_of(c, mi, msg), int.from_bytes(si[:L], "big"), int.from_bytes(si[L:], "big"), True)
    exp = [int(model(bytes(m[i * ml:(i + 1) * ml]), bytes(sig[i * 2 * L:(i + 1) * 2 * L]), bytes(q[i * 2 * L:(i + 1) * 2 * L]))) for i in range(N)]
    if msg:
        return Case("ecgpu_ecdsa_verify_msg_batch_dev", [q, m, S(MSG_LEN), sig], exp, lead=(I(c.cid),), tail=(I(1),))
    sg = np.frombuffer(bytes(sig), np.uint8).reshape(N, 2 * L)
    return Case("ecgpu_ecdsa_verify_batch_dev", [m, sg[:, :L].tobytes(), sg[:, L:].tobytes(), q], exp, lead=(I(c.cid),), tail=(I(1),))


def _ecdsa_recover_case(curve):
    c = pyec.CURVES[curve]
    L = c.L
    rng = _rng("recover" + curve)
    pool = _ecdsa_pool(c, rng)
    z = bytearray(b"".join(pool[i % POOL][0] for i in range(N)))
    r = bytearray(b"".join(pool[i % POOL][1][:L] for i in range(N)))
    s = bytearray(b"".join(pool[i % POOL][1][L:] for i in range(N)))
    recid = bytes(pool[i % POOL][3] for i in range(N))
    for i in BAD_S:
        _flip(s, i * L, 0x80)
    r[BAD_KEY * L:(BAD_KEY + 1) * L] = _off_curve_x(c, rng).to_bytes(L, "big")

    @functools.lru_cache(None)
    def model(zi, ri, si, idi):
        Q = pyec.ecdsa_recover(c, int.from_bytes(zi, "big"), int.from_bytes(ri, "big"), int.from_bytes(si, "big"), idi, True)
        return (bytes(2 * L), 0) if Q is None else (pyec.enc_point(c, Q)[0], 1)
    got = [model(bytes(z[i * L:(i + 1) * L]), bytes(r[i * L:(i + 1) * L]), bytes(s[i * L:(i + 1) * L]), recid[i]) for i in range(N)]
    assert all(got[i][0] == pool[i % POOL][2] for i in range(N) if i not in BAD_S + (BAD_KEY,))       # the signers' keys come out
    return Case("ecgpu_ecdsa_recover_batch_dev", [z, r, s, recid], [g[1] for g in got], lead=(I(c.cid),), tail=(I(1),),
                exp_xy=b"".join(g[0] for g in got))


def _bip340_model(P, e, r, s):
    """BIP340 verification on the challenge: R = s G - e P; R finite, y(R) even, x(R) = r"""
    c = pyec.K256
    if P is None or not pyec.on_curve(c, P) or r >= c.p or s >= c.n:
        return False
    R = pyec.add(c, pyec.mul(c, s, pyec.G(c)), pyec.mul(c, (-e) % c.n, P))
    return R is not pyec.INF and R[1] % 2 == 0 and R[0] == r


def _schnorr_case(raw):
    c = pyec.K256
    rng = _rng("bip340" + str(raw))
    pool = []
    while len(pool) < POOL:
        sk, aux = (bytes(rng.randrange(256) for _ in range(32)) for _ in range(2))
        m = bytes(rng.randrange(256) for _ in range(MSG_LEN if raw else 32))
        sig, ok = sm.schnorr_sign_raw(sk, m, aux)
        if ok:
            pool.append((pyec.lift_x(c, sm.mul_g(c, int.from_bytes(sk, "big"))[0], 0), m, sig))
    pk = bytearray(b"".join(pool[i % POOL][0][0].to_bytes(32, "big") for i in range(N)))
    pxy = bytearray(b"".join(pyec.enc_point(c, pool[i % POOL][0])[0] for i in range(N)))
    m = b"".join(pool[i % POOL][1] for i in range(N))
    sig = bytearray(b"".join(pool[i % POOL][2] for i in range(N)))
    for i in BAD_S:
        _flip(sig, i * 64 + 63)
    _flip(pxy, BAD_KEY * 64 + 63)
    pk[BAD_KEY * 32:(BAD_KEY + 1) * 32] = _off_curve_x(c, rng).to_bytes(32, "big")
    ml = len(pool[0][1])

    @functools.lru_cache(None)
    def model(key, mi, si):
        P = pyec.lift_x(c, int.from_bytes(key, "big"), 0) if raw else _ints(c, key)
        e = int.from_bytes(bip340_challenge(si[:32], key[:32], mi), "big") % c.n
        return _bip340_model(P, e, int.from_bytes(si[:32], "big"), int.from_bytes(si[32:], "big"))
    key, kl = (pk, 32) if raw else (pxy, 64)
    exp = [int(model(bytes(key[i * kl:(i + 1) * kl]), m[i * ml:(i + 1) * ml], bytes(sig[i * 64:(i + 1) * 64]))) for i in range(N)]
    if raw:
        return Case("ecgpu_schnorr_verify_raw_batch_dev", [pk, m, S(MSG_LEN), sig], exp)
    sg = np.frombuffer(bytes(sig), np.uint8).reshape(N, 64)
    # (the challenge of an element is hashed over the x of its key record: for element 128 that is the signer's x, the record's y is off)
    e = b"".join(bip340_challenge(bytes(sig[i * 64:i * 64 + 32]), bytes(pxy[i * 64:i * 64 + 32]), m[i * 32:(i + 1) * 32]) for i in range(N))
    return Case("ecgpu_schnorr_verify_batch_dev", [e, sg[:, :32].tobytes(), sg[:, 32:].tobytes(), pxy], exp)


def _sm2dsa_case(msg):
    c = pyec.CURVES["sm2"]
    rng = _rng("sm2dsa" + str(msg))
    e_of = lambda q, m: int.from_bytes(hashlib.new("sm3", pyec.sm2_za(c, DISTID, _ints(c, q)) + m).digest() if msg else m, "big")
    pool = []
    while len(pool) < POOL:
        d = rng.randrange(1, c.n - 1)
        q = pyec.enc_point(c, sm.mul_g(c, d))[0]
        m = bytes(rng.randrange(256) for _ in range(MSG_LEN if msg else 32))
        sig = pyec.sm2dsa_sign(c, d, e_of(q, m), rng.randrange(1, c.n))
        if sig is not None:
            pool.append((m, sig[0].to_bytes(32, "big") + sig[1].to_bytes(32, "big"), q))
    m, sig, q = (bytearray(b"".join(pool[i % POOL][k] for i in range(N))) for k in range(3))
    for i in BAD_S:
        _flip(sig, i * 64 + 63)
    _flip(q, BAD_KEY * 64 + 63)
    ml = len(pool[0][0])

    @functools.lru_cache(None)
    def model(mi, si, qi):
        return pyec.sm2dsa_verify(c, _ints(c, qi), e_of(qi, mi), int.from_bytes(si[:32], "big"), int.from_bytes(si[32:], "big"))
    exp = [int(model(bytes(m[i * ml:(i + 1) * ml]), bytes(sig[i * 64:(i + 1) * 64]), bytes(q[i * 64:(i + 1) * 64]))) for i in range(N)]
    if msg:
        return Case("ecgpu_sm2dsa_verify_msg_batch_dev", [DISTID, S(len(DISTID)), q, m, S(MSG_LEN), sig], exp)
    sg = np.frombuffer(bytes(sig), np.uint8).reshape(N, 64)
    return Case("ecgpu_sm2dsa_verify_batch_dev", [m, sg[:, :32].tobytes(), sg[:, 32:].tobytes(), q], exp)


def _bign_case(msg):
    c = pyec.CURVES["bign256"]
    rng = _rng("bign" + str(msg))
    le = lambda v: v.to_bytes(32, "little")
    h_of = lambda m: pyec.belt_hash(m) if msg else m
    pool = []
    for _ in range(POOL):
        d = rng.randrange(1, c.n - 1)
        Q = sm.mul_g(c, d)
        m = bytes(rng.randrange(256) for _ in range(MSG_LEN if msg else 32))
        pool.append((m, pyec.bign_sign(c, d, h_of(m), rng.randrange(1, c.n)), le(Q[0]) + le(Q[1])))
    m, sig, q = (bytearray(b"".join(pool[i % POOL][k] for i in range(N))) for k in range(3))
    for i in BAD_S:
        _flip(sig, i * 48 + 16)                      # S1, little-endian
    _flip(q, BAD_KEY * 64)
    ml = len(pool[0][0])

    @functools.lru_cache(None)
    def model(mi, si, qi):
        return pyec.bign_verify(c, _ints(c, qi, "little"), h_of(mi), si)
    exp = [int(model(bytes(m[i * ml:(i + 1) * ml]), bytes(sig[i * 48:(i + 1) * 48]), bytes(q[i * 64:(i + 1) * 64]))) for i in range(N)]
    if msg:
        return Case("ecgpu_bign_verify_msg_batch_dev", [q, m, S(MSG_LEN), sig], exp)
    return Case("ecgpu_bign_verify_batch_dev", [m, sig, q], exp)


# in the order of the queued run: what needs more scratch follows what needs less (no inverses -> ec_r -> the batch inversion's
# buffers without ec_xy -> with it -> the front stages' buffers -> the same on 48-byte records)
BUILDERS = {
    "schnorr_verify": lambda: _schnorr_case(False),
    "bign_verify": lambda: _bign_case(False),
    "sm2dsa_verify": lambda: _sm2dsa_case(False),
    "schnorr_verify_raw": lambda: _schnorr_case(True),
    "ecdsa_recover-k256": lambda: _ecdsa_recover_case("k256"),
    "ecdsa_verify-k256": lambda: _ecdsa_verify_case("k256", False),
    "bign_verify_msg": lambda: _bign_case(True),
    "sm2dsa_verify_msg": lambda: _sm2dsa_case(True),
    "ecdsa_verify_msg-k256": lambda: _ecdsa_verify_case("k256", True),
    "ecdsa_recover-p384": lambda: _ecdsa_recover_case("p384"),
    "ecdsa_verify-p384": lambda: _ecdsa_verify_case("p384", False),
    "ecdsa_verify_msg-p384": lambda: _ecdsa_verify_case("p384", True),
}


@functools.lru_cache(None)
def case(name):
    return BUILDERS[name]()


class Run:
    """one case on an engine: its inputs uploaded, outputs in device buffers of its own"""
    def __init__(self, eng, cs):
        self.eng, self.cs = eng, cs
        self.bufs = [eng.to_device(bytes(a)) if isinstance(a, (bytes, bytearray)) else a for a in cs.inputs]
        self.d_xy = eng.dev_alloc(len(cs.exp_xy)) if cs.exp_xy else None
        self.d_ok = eng.dev_alloc(N)

    def call(self):
        ptr = lambda b: b if isinstance(b, (ctypes.c_size_t, ctypes.c_int)) else ctypes.c_void_p(b.ptr)
        args = [*self.cs.lead, *map(ptr, self.bufs), S(N), *self.cs.tail, *([ptr(self.d_xy)] if self.d_xy else []), ptr(self.d_ok)]
        rc = getattr(self.eng._lib, self.cs.fn)(self.eng._ctx, *args)
        assert rc == 0, (self.cs.fn, rc, self.eng._lib.ecgpu_last_error(self.eng._ctx))

    def check(self):
        ok = bytes(self.eng.to_host(self.d_ok, N))
        assert ok == self.cs.exp_ok, [i for i in range(N) if ok[i] != self.cs.exp_ok[i]]
        if self.d_xy:
            xy = bytes(self.eng.to_host(self.d_xy, len(self.cs.exp_xy)))
            L2 = len(xy) // N
            assert xy == self.cs.exp_xy, [i for i in range(N) if xy[i * L2:(i + 1) * L2] != self.cs.exp_xy[i * L2:(i + 1) * L2]]

    def free(self):
        for b in self.bufs + [self.d_xy, self.d_ok]:
            if hasattr(b, "free"):
                b.free()


@pytest.mark.parametrize("name", list(BUILDERS))
def test_first_call_of_a_fresh_context(name):
    eng = ecgpu_module().Engine(0)
    try:
        run = Run(eng, case(name))
        run.call()
        run.check()
        run.call()                       # the same call again on the same context: the same bytes
        run.check()
        run.free()
    finally:
        eng.close()


def test_all_queued_on_one_fresh_context():
    eng = ecgpu_module().Engine(0)
    try:
        runs = [Run(eng, case(name)) for name in BUILDERS]
        eng.set_async(True)
        for run in runs:
            run.call()
        eng.synchronize()
        eng.set_async(False)
        for run in runs:
            run.check()
            run.free()
    finally:
        eng.close()
