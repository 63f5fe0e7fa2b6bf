"""Batch SM2DSA signing on the device (ecgpu_sm2dsa_sign_batch / _sign_rfc6979_batch / _sign_msg_batch; host-pointer forms only)
against tests/sm2sign_model.py: the standard's known answer, random batches on a workgroup and a normalisation-chain boundary, the
padding boundaries of Z and of Z || M, the failures that have to be constructed planted among good elements, an asynchronous
context, the argument errors, the pipelined path from 2^19 elements on, the wipe and the C example.

One reference batch of 1,000 elements is computed once (the model's arithmetic, with R = k G and PA = d G from the oracle's C
code: the model's own ladder takes a millisecond each) and every batch size is a prefix of it: elements are independent."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib
import pyec
import sm2sign_model as m
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
ERR_ARG = -7
C = m.C
SM2 = C.cid
N = m.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "sm2dsa_sign.json")))
SIZES = [1, 255, 256, 257, 1000]
NREF, MSG_LEN, DISTID = 1000, 40, b"1234567812345678"


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def enc32(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "big") if n else b""


def points(ks):
    """k G for ks in [1, n) from the oracle's C code -> [(x, y)]"""
    xy, inf = oracle_lib.batch_mul_base(SM2, enc32(ks))
    assert not inf.any()
    xy = bytes(xy)
    return [(int.from_bytes(xy[64 * i:64 * i + 32], "big"), int.from_bytes(xy[64 * i + 32:64 * i + 64], "big")) for i in range(len(ks))]


def model_rfc6979(ds, es):
    """sign_rfc6979 for a batch, the multiplications batched"""
    cands = [m.rfc6979_candidate(d, e) for d, e in zip(ds, es)]
    Rs = points([k if ok else 1 for k, ok in cands])
    return [m.finish(d, k, ok, e, R[0]) if ok else m.ZERO for d, e, (k, ok), R in zip(ds, es, cands, Rs)]


def pack(out):
    return b"".join(s for s, _ in out), bytes(ok for _, ok in out)


def dev(got):
    return bytes(got[0]), bytes(got[1])


@pytest.fixture(scope="module")
def ref():
    rng = random.Random("gpu-sm2sign-ref")
    r = {"ds": [rng.randrange(1, N - 1) for _ in range(NREF)], "ks": [rng.randrange(1, N) for _ in range(NREF)],
         "es": [rng.getrandbits(256) for _ in range(NREF)], "msgs": rand_bytes(rng, NREF * MSG_LEN)}
    r["pa"] = points(r["ds"])
    r["nonce"] = pack([m.sign(d, k, e, R) for d, k, e, R in zip(r["ds"], r["ks"], r["es"], points(r["ks"]))])
    r["rfc"] = pack(model_rfc6979(r["ds"], r["es"]))
    me = [m.message_hash(DISTID, Q, r["msgs"][i * MSG_LEN:(i + 1) * MSG_LEN]) for i, Q in enumerate(r["pa"])]
    r["me"] = me
    r["msg"] = pack(model_rfc6979(r["ds"], me))
    for f in ("nonce", "rfc", "msg"):
        assert r[f][1] == b"\x01" * NREF                  # (no random element fails: the failures are constructed below)
    return r


def test_the_standards_vector(eng):
    d, k, e = (int(VEC[t], 16) for t in ("d", "k", "e"))
    sig, ok = dev(eng.sm2dsa_sign(enc32([d]), enc32([k]), enc32([e])))
    assert (sig.hex().upper(), ok) == (VEC["r"] + VEC["s"], b"\x01")
    distid, msg = VEC["distid"].encode(), VEC["msg"].encode()
    want = m.sign_msg(distid, d, msg)
    assert want == m.sign(d, int(VEC["rfc6979_candidate"], 16), e)                        # the pinned candidate of the model
    assert dev(eng.sm2dsa_sign_msg(distid, enc32([d]), msg, len(msg))) == (want[0], b"\x01")
    assert dev(eng.sm2dsa_sign_rfc6979(enc32([d]), enc32([e]))) == (want[0], b"\x01")


@pytest.mark.parametrize("n", SIZES)
def test_random_batches(eng, ref, n):
    ds, ks, es, msgs = enc32(ref["ds"][:n]), enc32(ref["ks"][:n]), enc32(ref["es"][:n]), ref["msgs"][:n * MSG_LEN]
    got = {"nonce": dev(eng.sm2dsa_sign(ds, ks, es)), "rfc": dev(eng.sm2dsa_sign_rfc6979(ds, es)),
           "msg": dev(eng.sm2dsa_sign_msg(DISTID, ds, msgs, MSG_LEN))}
    for f, (sig, ok) in got.items():
        assert ok == ref[f][1][:n], f
        assert sig == ref[f][0][:64 * n], f
    # every signature verifies on the device ...
    q = b"".join(pyec.enc_point(C, Q)[0] for Q in ref["pa"][:n])
    r_of = lambda s: b"".join(s[64 * i:64 * i + 32] for i in range(n))
    s_of = lambda s: b"".join(s[64 * i + 32:64 * i + 64] for i in range(n))
    for f in ("nonce", "rfc"):
        assert bytes(eng.sm2dsa_verify(es, r_of(got[f][0]), s_of(got[f][0]), q)) == b"\x01" * n, f
    assert bytes(eng.sm2dsa_verify_msg(DISTID, q, msgs, MSG_LEN, got["msg"][0])) == b"\x01" * n
    # ... and a sample of 64 under the oracle
    pick = sorted(random.Random(n).sample(range(n), min(n, 64)))
    sub = lambda b, unit: b"".join(b[unit * i:unit * (i + 1)] for i in pick)
    for f in ("nonce", "rfc"):
        sg = sub(got[f][0], 64)
        rr, ss = b"".join(sg[64 * i:64 * i + 32] for i in range(len(pick))), b"".join(sg[64 * i + 32:64 * i + 64] for i in range(len(pick)))
        assert bytes(oracle_lib.sm2dsa_verify(sub(es, 32), rr, ss, sub(q, 64))) == b"\x01" * len(pick), f
    assert bytes(oracle_lib.sm2dsa_verify_msg(DISTID, sub(q, 64), sub(msgs, MSG_LEN), MSG_LEN, sub(got["msg"][0], 64))) == b"\x01" * len(pick)


@pytest.mark.parametrize("distid_len", [0, 16, 53, 54, 61, 62, 8191])
def test_padding_boundaries_of_the_message_form(eng, ref, distid_len):
    """Z's input is 194 + distid_len bytes (55 / 56 mod 64 at 53 / 54, 63 / 64 at 61 / 62); Z || M is 55 / 56 bytes at msg_len 23 / 24"""
    rng = random.Random("gpu-sm2sign-pad-%d" % distid_len)
    distid = rand_bytes(rng, distid_len)
    n = 5
    ds, pa = ref["ds"][:n], ref["pa"][:n]
    for msg_len in (0, 1, 23, 24, 31, 32, 87, 88, 200):
        msgs = rand_bytes(rng, n * msg_len)
        es = [m.message_hash(distid, Q, msgs[i * msg_len:(i + 1) * msg_len]) for i, Q in enumerate(pa)]
        want = pack(model_rfc6979(ds, es))
        assert dev(eng.sm2dsa_sign_msg(distid, enc32(ds), msgs, msg_len)) == want, msg_len
        assert want[1] == b"\x01" * n


FAILS = [c[0] for c in m.edge_cases(random.Random("gpu-sm2sign-edges")) if c[0].startswith("fails")]


@pytest.mark.parametrize("label", FAILS)
def test_constructed_failure_at_the_first_middle_and_last_position(eng, ref, label):
    n = 257
    case = [c for c in m.edge_cases(random.Random("gpu-sm2sign-edges")) if c[0] == label]
    assert len(case) == 1
    _, d, k, e = case[0]
    assert m.sign(d, k, e) == m.ZERO
    base_sig, base_ok = ref["nonce"][0][:64 * n], ref["nonce"][1][:n]
    for pos in (0, n // 2, n - 1):
        ds, ks, es = list(ref["ds"][:n]), list(ref["ks"][:n]), list(ref["es"][:n])
        ds[pos], ks[pos], es[pos] = d, k, e
        sig, ok = dev(eng.sm2dsa_sign(enc32(ds), enc32(ks), enc32(es)))
        assert ok == base_ok[:pos] + b"\x00" + base_ok[pos + 1:], (label, pos)
        assert sig == base_sig[:64 * pos] + bytes(64) + base_sig[64 * (pos + 1):], (label, pos)


def test_range_ends_and_unusable_keys_in_the_other_forms(eng, ref):
    cases = m.edge_cases(random.Random("gpu-sm2sign-ends"))
    ds, ks, es = ([c[j] for c in cases] for j in (1, 2, 3))
    Rs = points([k if 1 <= k < N else 1 for k in ks])
    want = pack([m.sign(d, k, e, R) for d, k, e, R in zip(ds, ks, es, Rs)])
    assert dev(eng.sm2dsa_sign(enc32(ds), enc32(ks), enc32(es))) == want
    assert want[1] == bytes(0 if c[0].startswith("fails") else 1 for c in cases)
    # the key's range in the forms that draw the nonce themselves: 0, n - 1, n and 2^256 - 1 among good ones
    bad = [0, N - 1, N, 2 ** 256 - 1]
    ds = ref["ds"][:3] + bad + ref["ds"][3:6]
    es = ref["es"][:10]
    sig, ok = dev(eng.sm2dsa_sign_rfc6979(enc32(ds), enc32(es)))
    assert ok == b"\x01" * 3 + b"\x00" * 4 + b"\x01" * 3
    assert sig == ref["rfc"][0][:192] + bytes(256) + pack(model_rfc6979(ds[7:], es[7:]))[0]
    msgs = ref["msgs"][:10 * MSG_LEN]
    sig, ok = dev(eng.sm2dsa_sign_msg(DISTID, enc32(ds), msgs, MSG_LEN))
    assert ok == b"\x01" * 3 + b"\x00" * 4 + b"\x01" * 3
    tail = [m.sign_msg(DISTID, d, msgs[i * MSG_LEN:(i + 1) * MSG_LEN]) for i, d in zip(range(7, 10), ds[7:])]
    assert sig == ref["msg"][0][:192] + bytes(256) + pack(tail)[0]


def test_asynchronous_context(eng, ref):
    """the calls have host-pointer forms only: on an asynchronous context each waits for the queued work, runs synchronously and
    leaves the mode as it found it"""
    n = 257
    ds, ks, es, msgs = enc32(ref["ds"][:n]), enc32(ref["ks"][:n]), enc32(ref["es"][:n]), ref["msgs"][:n * MSG_LEN]
    d_k, d_xy, d_inf = eng.to_device(ks), eng.dev_alloc(n * 64 + 16), eng.dev_alloc(n + 16)
    eng.set_async(True)
    try:
        eng.mul_by_generator_dev(SM2, d_k, n, d_xy, d_inf)                                # queued work in front of the calls
        got = {"nonce": dev(eng.sm2dsa_sign(ds, ks, es)), "rfc": dev(eng.sm2dsa_sign_rfc6979(ds, es)),
               "msg": dev(eng.sm2dsa_sign_msg(DISTID, ds, msgs, MSG_LEN))}
        eng.mul_by_generator_dev(SM2, d_k, n, d_xy, d_inf)                                # the context still queues
        eng.synchronize()
    finally:
        eng.set_async(False)
    for f in got:
        assert got[f] == (ref[f][0][:64 * n], ref[f][1][:n]), f
    assert bytes(eng.to_host(d_xy, 64 * n)) == b"".join(pyec.enc_point(C, R)[0] for R in points(ref["ks"][:n]))
    # an empty identifier and empty messages: both pointers may be NULL
    sig, ok = dev(eng.sm2dsa_sign_msg(b"", ds[:32 * 4], b"", 0))
    assert (sig, ok) == pack([m.sign_msg(b"", d, b"") for d in ref["ds"][:4]])
    assert eng.last_timing("total") >= eng.last_timing("main") > 0


def test_arguments_are_checked_before_anything_is_queued(eng):
    mod = ecgpu_module()
    lib = eng._lib
    arr = lambda size, fill: np.full(size, fill, np.uint8)
    p = lambda a: a.ctypes.data_as(mod._u8p)
    d, k, e, msgs, ident = arr(128, 5), arr(128, 5), arr(128, 5), arr(64, 7), arr(8192, 9)
    sig, ok = arr(256, 0xAB), arr(4, 0xCD)
    sz = ctypes.c_size_t
    bad = [lambda: lib.ecgpu_sm2dsa_sign_batch(eng._ctx, None, p(k), p(e), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_batch(eng._ctx, p(d), None, p(e), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_batch(eng._ctx, p(d), p(k), None, sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_batch(eng._ctx, p(d), p(k), p(e), sz(4), None, p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_batch(eng._ctx, p(d), p(k), p(e), sz(4), p(sig), None),
           lambda: lib.ecgpu_sm2dsa_sign_rfc6979_batch(eng._ctx, None, p(e), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_rfc6979_batch(eng._ctx, p(d), None, sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_rfc6979_batch(eng._ctx, p(d), p(e), sz(4), None, p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, p(ident), sz(8192), p(d), p(msgs), sz(16), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, p(ident), sz(8192), None, None, sz(0), sz(0), None, None),   # (checked before n)
           lambda: lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, None, sz(16), p(d), p(msgs), sz(16), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, p(ident), sz(16), None, p(msgs), sz(16), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, p(ident), sz(16), p(d), None, sz(16), sz(4), p(sig), p(ok)),
           lambda: lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, p(ident), sz(16), p(d), p(msgs), sz(16), sz(4), p(sig), None)]
    for i, call in enumerate(bad):
        assert call() == ERR_ARG, i
        assert b"ecgpu_sm2dsa_sign" in lib.ecgpu_last_error(eng._ctx), i
    assert bytes(sig) == b"\xab" * 256 and bytes(ok) == b"\xcd" * 4                       # nothing was written
    with pytest.raises(mod.EcgpuError) as err:
        eng.sm2dsa_sign_msg(bytes(8192), bytes(32), b"", 0)
    assert err.value.code == ERR_ARG
    # no elements: nothing to do, and no pointer is looked at
    for got in (eng.sm2dsa_sign(b"", b"", b""), eng.sm2dsa_sign_rfc6979(b"", b""), eng.sm2dsa_sign_msg(b"id", b"", b"", 7)):
        assert len(got[0]) == 0 and len(got[1]) == 0
    assert lib.ecgpu_sm2dsa_sign_batch(eng._ctx, None, None, None, sz(0), None, None) == 0
    # the longest identifier goes through
    assert lib.ecgpu_sm2dsa_sign_msg_batch(eng._ctx, p(ident), sz(8191), p(d), p(msgs), sz(16), sz(4), p(sig), p(ok)) == 0
    assert bytes(ok) == b"\x01" * 4


def test_pipelined_path(eng):
    """from 2^19 elements on a host-pointer call is cut into pieces that run under the transfers of their neighbours: every
    signature verifies on the device, and the elements at the ends and around the middle are the model's, byte for byte"""
    n = (1 << 19) + 3
    rng = np.random.default_rng(0x5325)
    ds = rng.integers(0, 256, n * 32, dtype=np.uint8)
    ds.reshape(n, 32)[:, 0] &= 0x7F                                                       # below n, and not zero in 2^19 draws
    es = rng.integers(0, 256, n * 32, dtype=np.uint8)
    sig, ok = eng.sm2dsa_sign_rfc6979(ds, es)
    assert bytes(ok) == b"\x01" * n
    q, inf = eng.mul_by_generator(SM2, ds)
    assert not inf.any()
    sg = sig.reshape(n, 64)
    v = eng.sm2dsa_verify(es, np.ascontiguousarray(sg[:, :32]).reshape(-1), np.ascontiguousarray(sg[:, 32:]).reshape(-1), q)
    assert bytes(v) == b"\x01" * n
    pick = list(range(4)) + list(range(n // 2 - 2, n // 2 + 2)) + list(range((1 << 19) - 2, n))
    geti = lambda a, i: int.from_bytes(bytes(a[32 * i:32 * i + 32]), "big")
    want = model_rfc6979([geti(ds, i) for i in pick], [geti(es, i) for i in pick])
    assert [(bytes(sg[i]), 1) for i in pick] == want


def test_caller_supplied_output_arrays(eng, ref):
    """Engine's out / ok: the same two arrays from call to call; an array that is too short is refused before the call"""
    n = 300
    ds, ks, es, msgs = enc32(ref["ds"][:n]), enc32(ref["ks"][:n]), enc32(ref["es"][:n]), ref["msgs"][:n * MSG_LEN]
    out, ok = np.full(n * 64, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    for f, call in (("nonce", lambda **kw: eng.sm2dsa_sign(ds, ks, es, **kw)), ("rfc", lambda **kw: eng.sm2dsa_sign_rfc6979(ds, es, **kw)),
                    ("msg", lambda **kw: eng.sm2dsa_sign_msg(DISTID, ds, msgs, MSG_LEN, **kw))):
        got = call(out=out, ok=ok)
        assert got[0] is out and got[1] is ok
        assert (bytes(out), bytes(ok)) == (ref[f][0][:64 * n], ref[f][1][:n]), f
        with pytest.raises(ecgpu_module().EcgpuError) as err:
            call(out=out[:-1], ok=ok)
        assert err.value.code == ERR_ARG


def test_wipe_and_a_following_unrelated_call(eng, ref):
    n = 64
    scal = enc32(ref["ks"][:n])
    before = eng.mul_by_generator(SM2, scal)
    eng.sm2dsa_sign_msg(DISTID, enc32(ref["ds"][:n]), ref["msgs"][:n * MSG_LEN], MSG_LEN)
    eng.wipe()
    after = eng.mul_by_generator(SM2, scal)
    assert bytes(after[0]) == bytes(before[0]) and bytes(after[1]) == bytes(before[1])
    want = b"".join(pyec.enc_point(C, R)[0] for R in points(ref["ks"][:n]))
    assert bytes(after[0]) == want
    assert dev(eng.sm2dsa_sign_rfc6979(enc32(ref["ds"][:n]), enc32(ref["es"][:n]))) == (ref["rfc"][0][:64 * n], b"\x01" * n)


def test_c_sm2dsa_sign_example_runs():
    """examples/sm2dsa_sign.c: the standard's known answer, a message signed and verified, the prehash form, a refused key"""
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["make", "-s", "-C", ex, "sm2dsa_sign"])
    out = subprocess.run([os.path.join(ex, "sm2dsa_sign")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": yes") == 4 and "NO" not in out.stdout
