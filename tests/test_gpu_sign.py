"""-m gpu: the signing entry points through the C ABI — ecgpu_ecdsa_sign_batch, ecgpu_ecdsa_sign_rfc6979_batch,
ecgpu_ecdsa_sign_msg_batch, ecgpu_schnorr_sign_raw_batch and their _dev forms — against the reference's vectors
(tests/golden), tests/sign_model.py, and the device's own verifiers and key recovery.

Recovery id bit 1 (x(R) >= n) is not reachable with findable inputs on these curves (an x in [n, p) is a 2^-128 event or
rarer); tests/test_hostcheck_sign.py::test_recid_bit_1_from_a_forged_x covers it by feeding the finish step such an x directly."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import oracle_lib
import pyec
import sign_model as sm
from gpu_common import ecgpu_module, load_golden

pytestmark = pytest.mark.gpu
ERR_CURVE, ERR_ARG = -1, -7
SIZES = (0, 1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def signing_golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "signing.json")) as f:
        return json.load(f)


def enc(c, values):
    return np.frombuffer(b"".join(int(v).to_bytes(c.L, "big") for v in values), np.uint8).copy()


def ints(c, arr):
    b = bytes(arr)
    return [int.from_bytes(b[i:i + c.L], "big") for i in range(0, len(b), c.L)]


def rand_bytes(rng, n):
    return np.frombuffer(rng.getrandbits(8 * n).to_bytes(n, "big") if n else b"", np.uint8).copy()


def rand_keys(c, rng, n):
    return [rng.randrange(1, c.n) for _ in range(n)]


def oracle_points(c, ks):
    """k G for valid k through the oracle's C code (None elsewhere): the model's R for the large batches"""
    safe = [k if 1 <= k < c.n else 1 for k in ks]
    xy, inf = oracle_lib.batch_mul_base(c.cid, enc(c, safe))
    assert not inf.any()
    b = bytes(xy)
    return [(int.from_bytes(b[i * 2 * c.L:i * 2 * c.L + c.L], "big"), int.from_bytes(b[i * 2 * c.L + c.L:(i + 1) * 2 * c.L], "big"))
            for i in range(len(ks))]


def model_batch(c, ds, ks, zs, normalize_s):
    """ks: nonces, None where the generator gave up"""
    Rs = oracle_points(c, [k or 0 for k in ks])
    sig, recid, ok = [], [], []
    for d, k, z, R in zip(ds, ks, zs, Rs):
        s_, r_, o_ = (bytes(2 * c.L), 0, 0) if k is None else sm.ecdsa_sign(c, d, k, z, normalize_s, R=R)
        sig.append(s_); recid.append(r_); ok.append(o_)
    return b"".join(sig), recid, ok


def same(got, want, what):
    sig, recid, ok = got
    assert [int(v) for v in ok] == list(want[2]), what
    assert [int(v) for v in recid] == list(want[1]), what
    assert bytes(sig) == want[0], what


def round_trip(eng, c, ds, zs, got, normalize_s):
    """every ok signature verifies on the device under reject_high_s = normalize_s, and its recovery id leads back to d G"""
    sig, recid, ok = got
    n = len(ds)
    if n == 0:
        return
    L = c.L
    safe = enc(c, [d if 1 <= d < c.n else 1 for d in ds])
    q, qinf = eng.mul_by_generator(c.cid, safe)
    assert not qinf.any()
    sg = np.asarray(sig).reshape(n, 2 * L)
    r, s = sg[:, :L].copy().reshape(-1), sg[:, L:].copy().reshape(-1)
    z = enc(c, zs)
    ver = eng.ecdsa_verify(c.cid, z, r, s, q, reject_high_s=bool(normalize_s))
    assert [int(v) for v in ver] == [int(v) for v in ok]
    keys, rok = eng.ecdsa_recover(c.cid, z, r, s, np.asarray(recid, np.uint8), reject_high_s=bool(normalize_s))
    assert [int(v) for v in rok] == [int(v) for v in ok]
    keys, q = np.asarray(keys).reshape(n, 2 * L), np.asarray(q).reshape(n, 2 * L)
    for i in range(n):
        if ok[i]:
            assert bytes(keys[i]) == bytes(q[i]), i


# ---- golden vectors -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k256", "p256", "p384", "p224", "p192", "p521"])
def test_golden_ecdsa_records(eng, name):
    c = pyec.CURVES[name]
    vec = load_golden(name)["ecdsa"]
    assert vec
    d, k, z = (enc(c, [int(v[f], 16) for v in vec]) for f in ("d", "k", "m"))
    sig, recid, ok = eng.ecdsa_sign(c.cid, d, k, z, normalize_s=False)
    assert all(int(v) == 1 for v in ok)
    assert bytes(sig).hex() == "".join(v["r"].rjust(2 * c.L, "0") + v["s"].rjust(2 * c.L, "0") for v in vec)
    for i, v in enumerate(vec):                     # the recovery id leads back to the record's key
        Q = pyec.ecdsa_recover(c, int(v["m"], 16), int(v["r"], 16), int(v["s"], 16), int(recid[i]))
        assert Q == (int(v["q_x"], 16), int(v["q_y"], 16)), i


@pytest.mark.parametrize("name", ["p224", "p256", "p384", "p521"])
def test_golden_rfc6979(eng, name):
    c = pyec.CURVES[name]
    for v in signing_golden()["rfc6979"][name]:
        msg = v["msg"].encode()
        d = enc(c, [int(v["d"], 16)])
        sig, recid, ok = eng.ecdsa_sign_msg(c.cid, d, msg, len(msg), normalize_s=False)
        assert int(ok[0]) == 1 and bytes(sig).hex() == v["sig"], v["msg"]
        z = sm.bits2field(c, hashlib.new(sm.DIGEST[name], msg).digest())
        sig2, recid2, ok2 = eng.ecdsa_sign_rfc6979(c.cid, d, enc(c, [z]), normalize_s=False)
        assert int(ok2[0]) == 1 and bytes(sig2).hex() == v["sig"] and int(recid2[0]) == int(recid[0])
        assert int(recid[0]) == sm.ecdsa_sign_msg(c, int(v["d"], 16), msg, False)[1]


@pytest.mark.parametrize("name", ["p256", "p384"])
def test_golden_prehash_longer_and_shorter_than_the_field(eng, name):
    c = pyec.CURVES[name]
    v = signing_golden()["prehash"][name]
    digest = hashlib.new(v["hash"], v["msg"].encode()).digest()
    assert len(digest) != c.L
    z = sm.bits2field(c, digest)
    sig, recid, ok = eng.ecdsa_sign_rfc6979(c.cid, enc(c, [int(v["d"], 16)]), enc(c, [z]), normalize_s=False)
    assert int(ok[0]) == 1 and bytes(sig).hex() == v["sig"]
    assert int(recid[0]) == sm.ecdsa_sign_rfc6979(c, int(v["d"], 16), z, False)[1]


def test_golden_ethereum_with_recovery_id(eng):
    v = [r for r in load_golden("k256")["recovery"] if "secret_key" in r][0]
    c = pyec.K256
    z = pyec.keccak256(bytes.fromhex(v["msg_hex"]))
    sig, recid, ok = eng.ecdsa_sign_rfc6979(c.cid, bytes.fromhex(v["secret_key"]), z, normalize_s=True)
    assert int(ok[0]) == 1 and bytes(sig).hex() == v["sig"] and int(recid[0]) == v["recid"]


def test_golden_bip340_sign_vectors(eng):
    vec = signing_golden()["bip340_sign"]
    assert [v["index"] for v in vec] == [0, 1, 2, 3]
    sk, msg, aux = (b"".join(bytes.fromhex(v[f]) for v in vec) for f in ("secret_key", "message", "aux_rand"))
    sig, ok = eng.schnorr_sign_raw(sk, msg, 32, aux)
    assert [int(v) for v in ok] == [1] * 4
    assert bytes(sig).hex() == "".join(v["signature"] for v in vec)
    pk = b"".join(bytes.fromhex(v["public_key"]) for v in vec)
    assert [int(v) for v in eng.schnorr_verify_raw(pk, msg, 32, sig)] == [1] * 4


# ---- random batches against the model, with the round trip on the device ---------------------------------------------------

@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_random_batches_caller_nonce(eng, name):
    c = pyec.CURVES[name]
    rng = random.Random("gpu-sign-" + name)
    for n in SIZES:
        ds, ks = rand_keys(c, rng, n), rand_keys(c, rng, n)
        zs = [rng.getrandbits(8 * c.L) for _ in range(n)]
        for normalize_s in (0, 1):
            got = eng.ecdsa_sign(c.cid, enc(c, ds), enc(c, ks), enc(c, zs), normalize_s=normalize_s)
            same(got, model_batch(c, ds, ks, zs, normalize_s), (name, n, normalize_s))
            round_trip(eng, c, ds, zs, got, normalize_s)


@pytest.mark.parametrize("name", sm.RFC6979_SETS)
def test_random_batches_rfc6979_and_messages(eng, name):
    c = pyec.CURVES[name]
    rng = random.Random("gpu-sign-rfc-" + name)
    rejected = 0
    for n in SIZES:
        ds = rand_keys(c, rng, n)
        zs = [rng.getrandbits(8 * c.L) for _ in range(n)]
        nonces = [sm.rfc6979_nonce(c, d, z) for d, z in zip(ds, zs)]
        rejected = max([rejected] + [r for _, r in nonces])
        msg_len = (0, 1, 31, 64, 119, 200)[SIZES.index(n)]
        msgs = rand_bytes(rng, n * msg_len)
        mz = [sm.bits2field(c, hashlib.new(sm.DIGEST[name], bytes(msgs[i * msg_len:(i + 1) * msg_len])).digest()) for i in range(n)]
        mk = [sm.rfc6979_nonce(c, d, z)[0] for d, z in zip(ds, mz)]
        for normalize_s in (0, 1):
            got = eng.ecdsa_sign_rfc6979(c.cid, enc(c, ds), enc(c, zs), normalize_s=normalize_s)
            same(got, model_batch(c, ds, [k for k, _ in nonces], zs, normalize_s), (name, n, normalize_s))
            round_trip(eng, c, ds, zs, got, normalize_s)
            got = eng.ecdsa_sign_msg(c.cid, enc(c, ds), msgs, msg_len, normalize_s=normalize_s)
            same(got, model_batch(c, ds, mk, mz, normalize_s), (name, n, normalize_s, "msg"))
            round_trip(eng, c, ds, mz, got, normalize_s)
            if n:                                      # the same through the verifier that hashes the messages itself
                q, _ = eng.mul_by_generator(c.cid, enc(c, ds))
                ver = eng.ecdsa_verify_msg(c.cid, q, msgs, msg_len, got[0], reject_high_s=bool(normalize_s))
                assert all(int(v) == 1 for v in ver), (name, n, normalize_s)
    if name.startswith("bp"):
        assert rejected >= 3          # the retry kernel has run several rounds for some lane of these batches


@pytest.mark.parametrize("name", sm.RFC6979_SETS)
def test_empty_messages(eng, name):
    """msg_len = 0 with n > 0: every key signs the digest of the empty string (no message array at all)"""
    c = pyec.CURVES[name]
    rng = random.Random("gpu-sign-empty-" + name)
    n = 67
    ds = rand_keys(c, rng, n)
    z = sm.bits2field(c, hashlib.new(sm.DIGEST[name], b"").digest())
    ks = [sm.rfc6979_nonce(c, d, z)[0] for d in ds]
    for normalize_s in (0, 1):
        got = eng.ecdsa_sign_msg(c.cid, enc(c, ds), b"", 0, normalize_s=normalize_s)
        same(got, model_batch(c, ds, ks, [z] * n, normalize_s), (name, normalize_s))
        round_trip(eng, c, ds, [z] * n, got, normalize_s)
    d_d = eng.to_device(enc(c, ds))
    outs = (eng.dev_alloc(n * 2 * c.L + 16), eng.dev_alloc(n + 16), eng.dev_alloc(n + 16))
    eng.ecdsa_sign_msg_dev(c.cid, d_d, None, 0, n, 1, *outs)
    assert bytes(eng.to_host(outs[0], n * 2 * c.L)) == bytes(got[0]) and bytes(eng.to_host(outs[2], n)) == bytes(got[2])


def test_arguments_are_checked_before_anything_is_queued(eng):
    mod = ecgpu_module()
    c = pyec.P256
    d_d, d_m = eng.to_device(enc(c, [5] * 4)), eng.to_device(np.zeros(64, np.uint8))
    sig, rid, ok = eng.dev_alloc(4 * 64 + 16), eng.dev_alloc(32), eng.dev_alloc(32)
    for args in ((None, d_m, 16, 4, 0, sig, rid, ok), (d_d, None, 16, 4, 0, sig, rid, ok), (d_d, d_m, 16, 4, 0, None, rid, ok),
                 (d_d, d_m, 16, 4, 0, sig, None, ok), (d_d, d_m, 16, 4, 0, sig, rid, None), (d_d.at(4), d_m, 16, 4, 0, sig, rid, ok)):
        with pytest.raises(mod.EcgpuError) as e:
            eng.ecdsa_sign_msg_dev(c.cid, *args)
        assert e.value.code == ERR_ARG
    eng.ecdsa_sign_msg_dev(c.cid, d_d, d_m, 16, 4, 0, sig, rid, ok)
    assert bytes(eng.to_host(ok, 4)) == b"\x01" * 4
    assert eng.last_timing("total") >= eng.last_timing("main") > 0


def test_rfc6979_candidate_cap(eng):
    """the 128-candidate cap, through the library's test hook for a lower one"""
    c = pyec.BP256
    rng = random.Random("gpu-cap")
    n = 300
    ds = rand_keys(c, rng, n)
    zs = [rng.getrandbits(256) for _ in range(n)]
    rej = [sm.rfc6979_nonce(c, d, z)[1] for d, z in zip(ds, zs)]
    assert max(rej) >= 3
    lib_hook = eng._lib.ecgpu_testhook_rfc6979_max_candidates
    lib_hook.restype = None
    hook = lambda cap: lib_hook(eng._ctx, cap)          # the cap of THIS context; other contexts keep 128
    other = ecgpu_module().Engine(0)
    try:
        for cap in (1, 3):
            hook(ctypes.c_int(cap))
            assert all(int(v) == 1 for v in other.ecdsa_sign_rfc6979(c.cid, enc(c, ds), enc(c, zs))[2])
            got = eng.ecdsa_sign_rfc6979(c.cid, enc(c, ds), enc(c, zs))
            ks = [sm.rfc6979_nonce(c, d, z, cap)[0] for d, z in zip(ds, zs)]
            assert [int(v) for v in got[2]] == [int(r < cap) for r in rej]
            same(got, model_batch(c, ds, ks, zs, 0), cap)
    finally:
        hook(ctypes.c_int(128))
        other.close()
    got = eng.ecdsa_sign_rfc6979(c.cid, enc(c, ds), enc(c, zs))
    assert all(int(v) == 1 for v in got[2])


@pytest.mark.parametrize("msg_len", [0, 32, 77])
def test_random_batches_schnorr(eng, msg_len):
    c = pyec.K256
    rng = random.Random(4000 + msg_len)
    for n in SIZES:
        sk, aux, msgs = enc(c, rand_keys(c, rng, n)), rand_bytes(rng, 32 * n), rand_bytes(rng, msg_len * n)
        sig, ok = eng.schnorr_sign_raw(sk, msgs, msg_len, aux)
        assert all(int(v) == 1 for v in ok)
        check = range(n) if n <= 65 else range(0, n, 16)
        for i in check:
            want = sm.schnorr_sign_raw(bytes(sk[32 * i:32 * i + 32]), bytes(msgs[msg_len * i:msg_len * (i + 1)]), bytes(aux[32 * i:32 * i + 32]))
            assert (bytes(sig[64 * i:64 * i + 64]), 1) == want, (n, i)
        if n:
            pk, pinf = eng.mul_by_generator(c.cid, sk)
            pkx = np.asarray(pk).reshape(n, 64)[:, :32].copy().reshape(-1)
            assert all(int(v) == 1 for v in eng.schnorr_verify_raw(pkx, msgs, msg_len, sig))


# ---- edges ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_edges(eng, name):
    c = pyec.CURVES[name]
    rng = random.Random("gpu-sign-edge-" + name)
    edge = [0, 1, c.n - 1, c.n, 2 ** (8 * c.L) - 1]
    good = lambda: rng.randrange(1, c.n)
    ds, ks, zs = [], [], []
    for v in edge:                                   # a bad element between good ones
        ds += [good(), v, good()]; ks += [good(), good(), good()]; zs += [rng.getrandbits(8 * c.L)] * 3
    for v in edge:
        ds += [good(), good(), good()]; ks += [good(), v, good()]; zs += [rng.getrandbits(8 * c.L)] * 3
    for v in (0, c.n, 2 ** (8 * c.L) - 1):
        ds += [good(), good()]; ks += [good(), good()]; zs += [v, v]
    for normalize_s in (0, 1):
        got = eng.ecdsa_sign(c.cid, enc(c, ds), enc(c, ks), enc(c, zs), normalize_s=normalize_s)      # returns ECGPU_OK: no exception
        want = [sm.ecdsa_sign(c, d, k, z, normalize_s) for d, k, z in zip(ds, ks, zs)]
        same(got, (b"".join(w[0] for w in want), [w[1] for w in want], [w[2] for w in want]), (name, normalize_s))
        assert [int(v) for v in got[2][:15]] == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1]
        assert [int(v) for v in got[2][15:30]] == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1]
        round_trip(eng, c, ds, zs, got, normalize_s)
        if name in sm.RFC6979_SETS:
            got = eng.ecdsa_sign_rfc6979(c.cid, enc(c, ds), enc(c, zs), normalize_s=normalize_s)
            want = [sm.ecdsa_sign_rfc6979(c, d, z, normalize_s) if 1 <= d < c.n else (bytes(2 * c.L), 0, 0) for d, z in zip(ds, zs)]
            same(got, (b"".join(w[0] for w in want), [w[1] for w in want], [w[2] for w in want]), (name, normalize_s, "rfc6979"))


def test_schnorr_edges(eng):
    c = pyec.K256
    rng = random.Random("gpu-schnorr-edge")
    sks = []
    for v in (0, 1, c.n - 1, c.n, 2 ** 256 - 1):
        sks += [rng.randrange(1, c.n), v, rng.randrange(1, c.n)]
    sk, aux, msgs = enc(c, sks), rand_bytes(rng, 32 * len(sks)), rand_bytes(rng, 32 * len(sks))
    sig, ok = eng.schnorr_sign_raw(sk, msgs, 32, aux)
    assert [int(v) for v in ok] == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1]
    for i in range(len(sks)):
        want = sm.schnorr_sign_raw(bytes(sk[32 * i:32 * i + 32]), bytes(msgs[32 * i:32 * i + 32]), bytes(aux[32 * i:32 * i + 32]))
        assert (bytes(sig[64 * i:64 * i + 64]), int(ok[i])) == want, i


# ---- call forms ---------------------------------------------------------------------------------------------------------------

def test_curve_errors(eng):
    mod = ecgpu_module()
    b32 = np.zeros(32, np.uint8)
    for cid in (mod.SM2, mod.BIGN256):
        for call in (lambda: eng.ecdsa_sign(cid, b32, b32, b32), lambda: eng.ecdsa_sign_rfc6979(cid, b32, b32),
                     lambda: eng.ecdsa_sign_msg(cid, b32, b32, 32)):
            with pytest.raises(mod.EcgpuError) as e:
                call()
            assert e.value.code == ERR_CURVE
    b24 = np.ones(24, np.uint8)
    for call in (lambda: eng.ecdsa_sign_rfc6979(mod.P192, b24, b24), lambda: eng.ecdsa_sign_msg(mod.P192, b24, b24, 24)):
        with pytest.raises(mod.EcgpuError) as e:
            call()
        assert e.value.code == ERR_CURVE
    assert int(eng.ecdsa_sign(mod.P192, b24, b24, b24)[2][0]) == 1          # the caller's nonce: p192 signs
    with pytest.raises(mod.EcgpuError) as e:
        eng.ecdsa_sign(99, b32, b32, b32)
    assert e.value.code == ERR_CURVE


@pytest.mark.parametrize("name", ["k256", "p384", "p521", "p224"])
def test_device_pointer_and_async_forms(eng, name):
    c = pyec.CURVES[name]
    rng = random.Random("gpu-sign-dev-" + name)
    n, L = 130, c.L
    ds, ks = rand_keys(c, rng, n), rand_keys(c, rng, n)
    zs = [rng.getrandbits(8 * L) for _ in range(n)]
    ks[7], ds[9] = 0, c.n
    msgs = rand_bytes(rng, n * 40)
    host = {"nonce": eng.ecdsa_sign(c.cid, enc(c, ds), enc(c, ks), enc(c, zs), normalize_s=True),
            "rfc": eng.ecdsa_sign_rfc6979(c.cid, enc(c, ds), enc(c, zs), normalize_s=True),
            "msg": eng.ecdsa_sign_msg(c.cid, enc(c, ds), msgs, 40, normalize_s=True)}
    d_d, d_k, d_z, d_m = (eng.to_device(a) for a in (enc(c, ds), enc(c, ks), enc(c, zs), msgs))
    outs = {f: (eng.dev_alloc(n * 2 * L + 16), eng.dev_alloc(n + 16), eng.dev_alloc(n + 16)) for f in host}

    def run():
        eng.ecdsa_sign_dev(c.cid, d_d, d_k, d_z, n, True, *outs["nonce"])
        eng.ecdsa_sign_rfc6979_dev(c.cid, d_d, d_z, n, True, *outs["rfc"])
        eng.ecdsa_sign_msg_dev(c.cid, d_d, d_m, 40, n, True, *outs["msg"])

    def check(what):
        for f in host:
            got = (eng.to_host(outs[f][0], n * 2 * L), eng.to_host(outs[f][1], n), eng.to_host(outs[f][2], n))
            for a, b in zip(got, host[f]):
                assert bytes(a) == bytes(b), (what, f)

    run()
    check("sync")
    zero = np.zeros(n * 2 * L + 16, np.uint8)
    for f in host:
        eng.to_device(zero, outs[f][0])
    eng.set_async(True)
    try:
        run()
        eng.synchronize()                            # a bad element is no deferred error either
    finally:
        eng.set_async(False)
    check("async")
    eng.wipe()


def test_schnorr_device_pointer_form(eng):
    c = pyec.K256
    rng = random.Random("gpu-schnorr-dev")
    n = 100
    sk, aux, msgs = enc(c, rand_keys(c, rng, n)), rand_bytes(rng, 32 * n), rand_bytes(rng, 48 * n)
    sig, ok = eng.schnorr_sign_raw(sk, msgs, 48, aux)
    d_sk, d_aux, d_m = eng.to_device(sk), eng.to_device(aux), eng.to_device(msgs)
    d_sig, d_ok = eng.dev_alloc(64 * n), eng.dev_alloc(n + 16)
    eng.set_async(True)
    try:
        eng.schnorr_sign_raw_dev(d_sk, d_m, 48, d_aux, n, d_sig, d_ok)
        eng.synchronize()
    finally:
        eng.set_async(False)
    assert bytes(eng.to_host(d_sig, 64 * n)) == bytes(sig) and bytes(eng.to_host(d_ok, n)) == bytes(ok)


def test_c_sign_and_verify_example_runs():
    """examples/sign_and_verify.c: `Signer::sign` on p256 (RFC 6979 A.2.5) and BIP340 vector 1 from plain C"""
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.run([os.path.join(ex, "sign_and_verify")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": yes") == 4 and "NO" not in out.stdout and "ok" in out.stdout


# ---- full size ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k256", "p256"])
def test_full_size_rfc6979(eng, name):
    """2^20 signatures through the host-pointer form (the pipelined staging path): every one accepted by the device verifier, a
    2^12 stride against the model"""
    c = pyec.CURVES[name]
    n, L = 1 << 20, c.L
    normalize_s = name == "k256"
    rs = np.random.default_rng(0x5160 + c.cid)
    d = oracle_lib.scalar_reduce(c.cid, rs.integers(0, 256, n * L, dtype=np.uint8))
    d.reshape(n, L)[:, L - 1] |= 1                    # no zero key
    z = rs.integers(0, 256, n * L, dtype=np.uint8)
    sig, recid, ok = eng.ecdsa_sign_rfc6979(c.cid, d, z, normalize_s=normalize_s)
    assert int(ok.sum()) == n
    q, qinf = eng.mul_by_generator(c.cid, d)
    sg = sig.reshape(n, 2 * L)
    ver = eng.ecdsa_verify(c.cid, z, sg[:, :L].copy().reshape(-1), sg[:, L:].copy().reshape(-1), q, reject_high_s=normalize_s)
    assert int(ver.sum()) == n
    for i in range(0, n, 1 << 12):
        want = sm.ecdsa_sign_rfc6979(c, int.from_bytes(bytes(d[i * L:(i + 1) * L]), "big"), int.from_bytes(bytes(z[i * L:(i + 1) * L]), "big"),
                                     normalize_s)
        assert (bytes(sg[i]), int(recid[i]), 1) == want, i
