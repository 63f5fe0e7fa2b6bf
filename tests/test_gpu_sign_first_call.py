"""-m gpu: every signing entry point (and the two SM2 encryption calls) as the FIRST call of a fresh context.

A scheme states its own scratch reservations beside the common ones (csrc/ecgpu_api.hip, the scheme functions around sign_pipeline;
sm2_pke_dev has a frame of its own).  A buffer a scheme forgot to reserve is invisible whenever an earlier call on the same context
has already grown it, and the other suites share one engine per module — so here each entry point gets a context of its own, and one
further context runs all of them queued behind each other, in an order in which a scheme that needs more follows one that needs less.
That run is then repeated at 600 elements on the same context: every buffer grows a second time, and a pointer read before the
reservations would be stale.

N = 257: one workgroup plus one element.  ECDSA in its three forms (caller's nonce, RFC 6979, messages) through the `_dev` entry points
on k256 and p384 (32- and 48-byte records, 32- and 64-bit HMAC state words) and from messages on p521 (the largest sg_state), BIP340
through ecgpu_schnorr_sign_raw_batch_dev, SM2DSA, bign and SM2 encryption / decryption through their host-pointer forms (they have no
other).  The elements are a pool of 5 distinct signers, repeated, so that the big-integer models (sign_model, sm2sign_model,
bignsign_model, pke_model) run once per distinct element.  Planted among them: element 0 has key 0, element 255 has key n, element 256
has nonce 0 in the caller's-nonce forms and key n - 1 in the others (a valid key everywhere but in SM2DSA).  SM2 encryption has no
private key: its secret scalar is the nonce, which is 0, n and n - 1 there.  Expected bytes, recovery ids and verdicts are the models',
element by element; the models alone must refuse exactly the planted elements (checked when a case is built, before anything runs on
the device).  After every case the library's read-back hook finds the wiped scratch zero."""
import ctypes
import functools
import random

import pytest

import bignsign_model as bm
import pke_model as pm
import pyec
import sign_model as sm
import sm2sign_model as s2
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
N, N_AGAIN = 257, 600
KEY_0, KEY_N, LAST = 0, 255, 256
POOL = 5                              # distinct signers; element i is signer i % POOL
MSG_LEN = 40
DISTID = b"1234567812345678"


class Case:
    """dev: fn(eng, inputs, outputs) on device buffers (inputs uploaded, outputs allocated at the sizes of `exp`); otherwise
    fn(eng) -> the host arrays.  exp: the expected outputs in the entry point's order, the verdicts last; planted: the elements
    the models must refuse, and no others."""
    def __init__(self, n, fn, exp, planted, inputs=None):
        self.n, self.fn, self.inputs, self.exp = n, fn, inputs, tuple(bytes(e) for e in exp)
        ok = self.exp[-1]
        assert len(ok) == n and set(ok) <= {0, 1}
        assert [i for i in range(n) if not ok[i]] == sorted(planted), ([i for i in range(n) if not ok[i]], planted)
        for rec in self.exp[:-1]:
            unit = len(rec) // n
            assert len(rec) == unit * n and all(rec[unit * i:unit * i + unit] == bytes(unit) for i in planted)


def _rng(tag):
    return random.Random("sign-first-call-" + tag)


def _rand(rng, nbytes):
    return bytes(rng.randrange(256) for _ in range(nbytes))


def _elements(n, pool, edges):
    """element i is pool[i % POOL], but for the planted ones: edges maps an index to the fields it replaces"""
    out = []
    for i in range(n):
        el = list(pool[i % POOL])
        for field, value in edges.get(i, {}).items():
            el[field] = value
        out.append(tuple(el))
    return out


def _columns(rows):
    return [b"".join(col) for col in zip(*rows)]


def _edges(order, keyed_nonce):
    """the planted keys (field 0) and, in the caller's-nonce forms, the planted nonce (field 1)"""
    return {KEY_0: {0: 0}, KEY_N: {0: order}, LAST: {1: 0} if keyed_nonce else {0: order - 1}}


# ---- ECDSA: d, k, z as integers (k unused in the RFC 6979 forms), or d and a message -----------------------------------------
@functools.lru_cache(None)
def _ecdsa_model(curve, form, d, k, m):
    c = pyec.CURVES[curve]
    norm = sm.NORMALIZE_S.get(curve, False)
    if form == "nonce":
        sig, recid, ok = sm.ecdsa_sign(c, d, k, int.from_bytes(m, "big"), norm)
    elif form == "rfc6979":
        sig, recid, ok = sm.ecdsa_sign_rfc6979(c, d, int.from_bytes(m, "big"), norm)
    else:
        sig, recid, ok = sm.ecdsa_sign_msg(c, d, m, norm)
    return sig, bytes([recid]), bytes([ok])


def _ecdsa_case(curve, form, n):
    c = pyec.CURVES[curve]
    L, norm = c.L, sm.NORMALIZE_S.get(curve, False)
    rng = _rng("ecdsa" + curve + form)
    pool = [(rng.randrange(1, c.n), rng.randrange(1, c.n), _rand(rng, MSG_LEN if form == "msg" else L)) for _ in range(POOL)]
    els = _elements(n, pool, _edges(c.n, form == "nonce"))
    exp = _columns(_ecdsa_model(curve, form, *el) for el in els)
    d, k, m = _columns((el[0].to_bytes(L, "big"), el[1].to_bytes(L, "big"), el[2]) for el in els)
    if form == "nonce":
        return Case(n, lambda e, i, o: e.ecdsa_sign_dev(c.cid, i[0], i[1], i[2], n, norm, *o), exp, (KEY_0, KEY_N, LAST), [d, k, m])
    if form == "rfc6979":
        return Case(n, lambda e, i, o: e.ecdsa_sign_rfc6979_dev(c.cid, i[0], i[1], n, norm, *o), exp, (KEY_0, KEY_N), [d, m])
    return Case(n, lambda e, i, o: e.ecdsa_sign_msg_dev(c.cid, i[0], i[1], MSG_LEN, n, norm, *o), exp, (KEY_0, KEY_N), [d, m])


# ---- BIP340: key, message, aux_rand ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _schnorr_model(sk, msg, aux):
    sig, ok = sm.schnorr_sign_raw(sk.to_bytes(32, "big"), msg, aux)
    return sig, bytes([ok])


def _schnorr_case(n):
    c = pyec.K256
    rng = _rng("bip340")
    pool = [(rng.randrange(1, c.n), _rand(rng, MSG_LEN), _rand(rng, 32)) for _ in range(POOL)]
    els = _elements(n, pool, _edges(c.n, False))
    exp = _columns(_schnorr_model(*el) for el in els)
    sk, msg, aux = _columns((el[0].to_bytes(32, "big"), el[1], el[2]) for el in els)
    return Case(n, lambda e, i, o: e.schnorr_sign_raw_dev(i[0], i[1], MSG_LEN, i[2], n, *o), exp, (KEY_0, KEY_N), [sk, msg, aux])


# ---- SM2DSA: d, k, e as integers, or d and a message; key n - 1 is refused (1 + d has no inverse) -----------------------------------
@functools.lru_cache(None)
def _sm2dsa_model(form, d, k, m):
    if form == "nonce":
        sig, ok = s2.sign(d, k, int.from_bytes(m, "big"))
    elif form == "rfc6979":
        sig, ok = s2.sign_rfc6979(d, int.from_bytes(m, "big"))
    else:
        sig, ok = s2.sign_msg(DISTID, d, m)
    return sig, bytes([ok])


def _sm2dsa_case(form, n):
    rng = _rng("sm2dsa" + form)
    pool = [(rng.randrange(1, s2.N - 1), rng.randrange(1, s2.N), _rand(rng, MSG_LEN if form == "msg" else 32)) for _ in range(POOL)]
    els = _elements(n, pool, _edges(s2.N, form == "nonce"))
    exp = _columns(_sm2dsa_model(form, *el) for el in els)
    d, k, m = _columns((el[0].to_bytes(32, "big"), el[1].to_bytes(32, "big"), el[2]) for el in els)
    if form == "nonce":
        return Case(n, lambda e: e.sm2dsa_sign(d, k, m), exp, (KEY_0, KEY_N, LAST))
    if form == "rfc6979":
        return Case(n, lambda e: e.sm2dsa_sign_rfc6979(d, m), exp, (KEY_0, KEY_N, LAST))
    return Case(n, lambda e: e.sm2dsa_sign_msg(DISTID, d, m, MSG_LEN), exp, (KEY_0, KEY_N, LAST))


# ---- bign: d, k as integers, h the raw prehash bytes, or d and a message; every record little-endian --------------------------------
@functools.lru_cache(None)
def _bign_model(form, d, k, m):
    sig, ok = bm.sign(d, k, m) if form == "nonce" else bm.sign_prehash(d, m) if form == "prehash" else bm.sign_msg(d, m)
    return sig, bytes([ok])


def _bign_case(form, n):
    rng = _rng("bign" + form)
    pool = [(rng.randrange(1, bm.Q), rng.randrange(1, bm.Q), _rand(rng, MSG_LEN if form == "msg" else 32)) for _ in range(POOL)]
    els = _elements(n, pool, _edges(bm.Q, form == "nonce"))
    exp = _columns(_bign_model(form, *el) for el in els)
    d, k, m = _columns((bm.le(el[0]), bm.le(el[1]), el[2]) for el in els)
    if form == "nonce":
        return Case(n, lambda e: e.bign_sign(d, k, m), exp, (KEY_0, KEY_N, LAST))
    if form == "prehash":
        return Case(n, lambda e: e.bign_sign_prehash(d, m), exp, (KEY_0, KEY_N))
    return Case(n, lambda e: e.bign_sign_msg(d, m, MSG_LEN), exp, (KEY_0, KEY_N))


# ---- SM2 encryption: the recipient's key d (P = d G), the nonce k, the message -------------------------------------------------------
@functools.lru_cache(None)
def _public(d):
    return pm.enc_xy(sm.mul_g(pm.C, d))


@functools.lru_cache(None)
def _seal_model(d, k, msg):
    P = sm.mul_g(pm.C, d)
    got = pm.encrypt(P, k, msg)
    if got is None:
        return bytes(64), bytes(len(msg)), bytes(32), b"\x00"
    return pm.enc_xy(got[0]), got[1], got[2], b"\x01"


@functools.lru_cache(None)
def _open_model(d, c1, c2, c3):
    got = pm.decrypt(d, (int.from_bytes(c1[:32], "big"), int.from_bytes(c1[32:], "big")), c2, c3)
    return (bytes(len(c2)), b"\x00") if got is None else (got, b"\x01")


def _pke_pool():
    rng = _rng("pke")
    return [(rng.randrange(1, pm.C.n), rng.randrange(1, pm.C.n), _rand(rng, MSG_LEN)) for _ in range(POOL)]


def _pke_encrypt_case(n):
    order = pm.C.n
    els = _elements(n, _pke_pool(), {KEY_0: {1: 0}, KEY_N: {1: order}, LAST: {1: order - 1}})
    exp = _columns(_seal_model(*el) for el in els)
    pk, k, msg = _columns((_public(el[0]), el[1].to_bytes(32, "big"), el[2]) for el in els)
    return Case(n, lambda e: e.sm2_pke_encrypt(pk, k, msg, MSG_LEN), exp, (KEY_0, KEY_N))


def _pke_decrypt_case(n):
    """the ciphertexts are the model's, sealed to the pool's keys; element 256 is sealed to (n - 1) G and opens"""
    order = pm.C.n
    rows = []
    for i, (d, k, msg) in enumerate(_elements(n, _pke_pool(), {LAST: {0: order - 1}})):
        c1, c2, c3, ok = _seal_model(d, k, msg)
        assert ok == b"\x01"
        rows.append(({KEY_0: 0, KEY_N: order}.get(i, d), c1, c2, c3))
    exp = _columns(_open_model(*row) for row in rows)
    d, c1, c2, c3 = _columns((row[0].to_bytes(32, "big"),) + row[1:] for row in rows)
    return Case(n, lambda e: e.sm2_pke_decrypt(d, c1, c2, MSG_LEN, c3), exp, (KEY_0, KEY_N))


# in the order of the queued run: what needs more scratch follows what needs less (the common list alone -> sg_dp at 16 bytes ->
# sg_state -> sg_dp at 64 bytes -> vtab -> ec_e -> 48-byte records -> the largest sg_state)
BUILDERS = {
    "sm2dsa_sign": lambda n: _sm2dsa_case("nonce", n),
    "sm2dsa_sign_rfc6979": lambda n: _sm2dsa_case("rfc6979", n),
    "bign_sign": lambda n: _bign_case("nonce", n),
    "bign_sign_prehash": lambda n: _bign_case("prehash", n),
    "schnorr_sign": _schnorr_case,
    "sm2_pke_decrypt": _pke_decrypt_case,
    "sm2_pke_encrypt": _pke_encrypt_case,
    "ecdsa_sign-k256": lambda n: _ecdsa_case("k256", "nonce", n),
    "ecdsa_sign_rfc6979-k256": lambda n: _ecdsa_case("k256", "rfc6979", n),
    "sm2dsa_sign_msg": lambda n: _sm2dsa_case("msg", n),
    "bign_sign_msg": lambda n: _bign_case("msg", n),
    "ecdsa_sign_msg-k256": lambda n: _ecdsa_case("k256", "msg", n),
    "ecdsa_sign-p384": lambda n: _ecdsa_case("p384", "nonce", n),
    "ecdsa_sign_rfc6979-p384": lambda n: _ecdsa_case("p384", "rfc6979", n),
    "ecdsa_sign_msg-p384": lambda n: _ecdsa_case("p384", "msg", n),
    "ecdsa_sign_msg-p521": lambda n: _ecdsa_case("p521", "msg", n),
}


@functools.lru_cache(None)
def case(name, n=N):
    return BUILDERS[name](n)


class Run:
    """one case on an engine: a `_dev` form gets its inputs uploaded and outputs in device buffers of its own"""
    def __init__(self, eng, cs):
        self.eng, self.cs, self.got, self.bufs = eng, cs, None, []
        if cs.inputs is not None:
            self.ins = [eng.to_device(a) for a in cs.inputs]
            self.outs = [eng.dev_alloc(len(e)) for e in cs.exp]
            self.bufs = self.ins + self.outs

    def call(self):
        if self.cs.inputs is None:
            self.got = self.cs.fn(self.eng)
        else:
            self.cs.fn(self.eng, self.ins, self.outs)

    def check(self):
        if self.cs.inputs is not None:
            self.got = [self.eng.to_host(b, len(e)) for b, e in zip(self.outs, self.cs.exp)]
        assert len(self.got) == len(self.cs.exp)
        ok = bytes(self.got[-1])
        assert ok == self.cs.exp[-1], [i for i in range(self.cs.n) if ok[i] != self.cs.exp[-1][i]]
        for got, exp in zip(self.got[:-1], self.cs.exp[:-1]):
            got, unit = bytes(got), len(exp) // self.cs.n
            assert got == exp, [i for i in range(self.cs.n) if got[unit * i:unit * i + unit] != exp[unit * i:unit * i + unit]]
            assert all(got[unit * i:unit * i + unit] == bytes(unit) for i in range(self.cs.n) if not ok[i])    # refused: a zero record

    def free(self):
        for b in self.bufs:
            b.free()


def _wiped(eng):
    hook = eng._lib.ecgpu_testhook_wiped_scratch_nonzero
    hook.restype = ctypes.c_longlong
    return hook(eng._ctx)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_first_call_of_a_fresh_context(name):
    cs = case(name)
    eng = ecgpu_module().Engine(0)
    try:
        run = Run(eng, cs)
        run.call()
        run.check()
        assert _wiped(eng) == 0
        run.call()                       # the same call again on the same context: the same bytes
        run.check()
        assert _wiped(eng) == 0
        run.free()
    finally:
        eng.close()


def test_all_queued_on_one_fresh_context_then_again_at_600():
    cases = [[case(name, n) for name in BUILDERS] for n in (N, N_AGAIN)]
    eng = ecgpu_module().Engine(0)
    try:
        for batch in cases:
            runs = [Run(eng, cs) for cs in batch]
            eng.set_async(True)
            for run in runs:
                run.call()
            eng.synchronize()
            eng.set_async(False)
            assert _wiped(eng) == 0
            for run in runs:
                run.check()
                run.free()
    finally:
        eng.close()
