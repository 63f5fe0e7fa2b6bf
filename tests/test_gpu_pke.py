"""Batch SM2 public-key encryption and decryption on the device (ecgpu_sm2_pke_encrypt_batch / ecgpu_sm2_pke_decrypt_batch) against
tests/pke_model.py: the reference's vectors, the message lengths the KDF's and SM3's edges sit at, bad elements at every position
among good ones, the argument errors, the pipelined path from 2^19 elements on and the wipe behind the calls.

The model is pke_model.encrypt / decrypt (hashlib's SM3 + pyec).  For the batches of several hundred elements the two
multiplications of the model come from the oracle's C code (pyec takes 14 ms each) and the KDF, the XOR and C3 from pke_model."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import oracle_lib
import pke_model as pm
import pyec
from gpu_common import ecgpu_module
from test_pke_model import der_four_fields

pytestmark = pytest.mark.gpu
ERR_ARG = -7
C = pm.C
SM2 = C.cid
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "sm2pke.json")))
D = int(VEC["private_key"], 16)
MSG = bytes.fromhex(VEC["msg"])


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


@pytest.fixture(scope="module")
def Q():
    return pyec.mul(C, D, pyec.G(C))


def enc32(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "big") if n else b""


def model_encrypt_batch(pk, ks, msgs, msg_len):
    """(c1, c2, c3, ok) for valid keys and nonces in [1, n): the oracle's multiplications, pke_model's hashing"""
    n = len(ks)
    c1, inf = oracle_lib.batch_mul_base(SM2, enc32(ks))
    xy, inf2 = oracle_lib.batch_mul(SM2, enc32(ks), pk)
    assert not inf.any() and not inf2.any()
    c1, xy = bytearray(bytes(c1)), bytes(xy)
    c2, c3, ok = bytearray(), bytearray(), []
    for i in range(n):
        x2, y2, M = xy[64 * i:64 * i + 32], xy[64 * i + 32:64 * i + 64], msgs[i * msg_len:(i + 1) * msg_len]
        t = pm.kdf(x2, y2, msg_len)
        if any(t):
            c2 += bytes(a ^ b for a, b in zip(M, t))
            c3 += pm.sm3(x2 + M + y2)
        else:
            c1[64 * i:64 * i + 64] = bytes(64)
            c2 += bytes(msg_len)
            c3 += bytes(32)
        ok.append(int(any(t)))
    return bytes(c1), bytes(c2), bytes(c3), ok


def device_encrypt(eng, pk, k, msgs, msg_len):
    c1, c2, c3, ok = eng.sm2_pke_encrypt(pk, k, msgs, msg_len)
    return bytes(c1), bytes(c2), bytes(c3), [int(v) for v in ok]


def device_decrypt(eng, d, c1, c2, msg_len, c3):
    m, ok = eng.sm2_pke_decrypt(d, c1, c2, msg_len, c3)
    return bytes(m), [int(v) for v in ok]


# ---- the reference's vectors -----------------------------------------------------------------------------------------------
def test_decrypts_the_reference_cipher(eng):
    C1, C2, C3 = pm.split_cipher(bytes.fromhex(VEC["cipher"]))
    assert device_decrypt(eng, enc32([D]), pm.enc_xy(C1), C2, len(C2), C3) == (MSG, [1])


def test_decrypts_the_reference_asn1_cipher(eng):
    x, y, c3, c2 = der_four_fields(bytes.fromhex(VEC["asn1_cipher"]))
    assert device_decrypt(eng, enc32([D]), pm.enc_xy((x, y)), c2, len(c2), c3) == (MSG, [1])


def test_encrypts_the_reference_message_with_a_fixed_nonce(eng, Q):
    k = 0x59276E27D506861A16680F3AD9C02DCCEF3CC1FA3CDBE4CE6D54B80DEAC1BC21
    C1, C2, C3 = pm.encrypt(Q, k, MSG)
    got = device_encrypt(eng, pm.enc_xy(Q), enc32([k]), MSG, len(MSG))
    assert got == (pm.enc_xy(C1), C2, C3, [1])
    assert device_decrypt(eng, enc32([D]), got[0], got[1], len(MSG), got[2]) == (MSG, [1])
    assert pm.decrypt(D, C1, got[1], got[2]) == MSG


# ---- lengths and shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msg_len", pm.LENGTHS)
def test_lengths_and_batch_shapes(eng, msg_len):
    """n = 1, 2, 257 (one lane, two lanes, one workgroup and one element): encrypt equals the model on every element, the device's
    decrypt of the device's encrypt gives the messages back.  An odd msg_len puts the message bases on all four byte alignments."""
    rng = random.Random("gpu-pke-%d" % msg_len)
    for n in (1, 2, 257):
        ds = [rng.randrange(1, C.n) for _ in range(n)]
        ks = [rng.randrange(1, C.n) for _ in range(n)]
        pk, inf = oracle_lib.batch_mul_base(SM2, enc32(ds))
        msgs = rand_bytes(rng, n * msg_len)
        want = model_encrypt_batch(pk, ks, msgs, msg_len)
        got = device_encrypt(eng, pk, enc32(ks), msgs, msg_len)
        assert got == want, (msg_len, n)
        assert sum(want[3]) >= n - 4                      # (msg_len = 1: one keystream in 256 is all zero, a legal ok = 0)
        m, ok = device_decrypt(eng, enc32(ds), got[0], got[1], msg_len, got[2])
        assert ok == want[3]
        for i in range(n):
            assert m[i * msg_len:(i + 1) * msg_len] == (msgs[i * msg_len:(i + 1) * msg_len] if ok[i] else bytes(msg_len)), (msg_len, n, i)
    # one element of the largest batch through the whole model, multiplications included
    i = n - 1
    P = (int.from_bytes(bytes(pk[64 * i:64 * i + 32]), "big"), int.from_bytes(bytes(pk[64 * i + 32:64 * i + 64]), "big"))
    one = pm.encrypt(P, ks[i], msgs[i * msg_len:])
    if one is not None:
        assert (got[0][64 * i:], got[1][i * msg_len:], got[2][32 * i:]) == (pm.enc_xy(one[0]), one[1], one[2])


# ---- bad elements at every position among good ones -----------------------------------------------------------------------
def good_seven(Qpt, msg_len, seed):
    """seven elements under the vector's key whose model ciphertexts exist (at msg_len = 1 a nonce with a zero keystream is skipped)"""
    rng = random.Random(seed)
    ks, msgs, cts = [], [], []
    while len(ks) < 7:
        k, M = rng.randrange(1, C.n), rand_bytes(rng, msg_len)
        ct = pm.encrypt(Qpt, k, M)
        if ct is not None:
            ks.append(k); msgs.append(M); cts.append(ct)
    return ks, msgs, cts


@pytest.mark.parametrize("kind", ["k=0", "k=n", "k=2^256-1", "off-curve", "x=p", "zero-keystream"])
def test_encrypt_bad_element_at_every_position(eng, Q, kind):
    msg_len = 1 if kind == "zero-keystream" else 37
    ks, msgs, cts = good_seven(Q, msg_len, "enc-bad-" + kind)
    for pos in range(7):
        k = list(ks)
        pk = [Q] * 7
        if kind == "k=0": k[pos] = 0
        elif kind == "k=n": k[pos] = C.n
        elif kind == "k=2^256-1": k[pos] = 2 ** 256 - 1
        elif kind == "off-curve": pk[pos] = (Q[0], Q[1] ^ 1)
        elif kind == "x=p": pk[pos] = (C.p, Q[1])
        else: k[pos] = pm.ZERO_KEYSTREAM_NONCES[pos % 3]
        assert pm.encrypt(pk[pos], k[pos], msgs[pos]) is None
        c1, c2, c3, ok = device_encrypt(eng, b"".join(pm.enc_xy(P) for P in pk), enc32(k), b"".join(msgs), msg_len)
        assert ok == [int(i != pos) for i in range(7)], (kind, pos)
        for i in range(7):
            got = (c1[64 * i:64 * i + 64], c2[i * msg_len:(i + 1) * msg_len], c3[32 * i:32 * i + 32])
            want = (bytes(64), bytes(msg_len), bytes(32)) if i == pos else (pm.enc_xy(cts[i][0]), cts[i][1], cts[i][2])
            assert got == want, (kind, pos, i)


@pytest.mark.parametrize("kind", ["d=0", "d=n", "off-curve", "c2-bit", "c3-bit"])
def test_decrypt_bad_element_at_every_position(eng, Q, kind):
    msg_len = 37
    ks, msgs, cts = good_seven(Q, msg_len, "dec-bad-" + kind)
    for pos in range(7):
        d = [D] * 7
        c1 = [ct[0] for ct in cts]
        c2 = [bytearray(ct[1]) for ct in cts]
        c3 = [bytearray(ct[2]) for ct in cts]
        if kind == "d=0": d[pos] = 0
        elif kind == "d=n": d[pos] = C.n
        elif kind == "off-curve": c1[pos] = (c1[pos][0], c1[pos][1] ^ 1)
        elif kind == "c2-bit": c2[pos][(5 * pos) % msg_len] ^= 1 << pos
        else: c3[pos][(5 * pos) % 32] ^= 1 << pos
        assert pm.decrypt(d[pos], c1[pos], bytes(c2[pos]), bytes(c3[pos])) is None
        m, ok = device_decrypt(eng, enc32(d), b"".join(pm.enc_xy(P) for P in c1), b"".join(bytes(v) for v in c2), msg_len,
                               b"".join(bytes(v) for v in c3))
        assert ok == [int(i != pos) for i in range(7)], (kind, pos)
        for i in range(7):
            assert m[i * msg_len:(i + 1) * msg_len] == (bytes(msg_len) if i == pos else msgs[i]), (kind, pos, i)


def test_model_built_ciphertext_with_a_zero_keystream_decrypts(eng, Q):
    """t = 0 is a reason to draw another nonce when encrypting, not a defect of a ciphertext: C2 = M, C3 = SM3(x2 || M || y2) opens"""
    k = pm.ZERO_KEYSTREAM_NONCES[0]
    x2, y2 = pm.shared(k, Q)
    assert pm.kdf(x2, y2, 1) == b"\x00"
    C1 = pyec.mul(C, k, pyec.G(C))
    M = b"\xa7"
    assert pm.decrypt(D, C1, M, pm.sm3(x2 + M + y2)) == M
    assert device_decrypt(eng, enc32([D]), pm.enc_xy(C1), M, 1, pm.sm3(x2 + M + y2)) == (M, [1])


# ---- arguments and edge cases ----------------------------------------------------------------------------------------------
def test_empty_message(eng, Q):
    mod = ecgpu_module()
    with pytest.raises(mod.EcgpuError) as e:
        eng.sm2_pke_encrypt(pm.enc_xy(Q), enc32([5]), b"", 0)
    assert e.value.code == ERR_ARG and "ecgpu_sm2_pke_encrypt_batch" in str(e.value)
    # the context stays usable
    assert device_encrypt(eng, pm.enc_xy(Q), enc32([5]), b"m", 1)[3] == [1]
    # decrypt: ok = (SM3(x2 || y2) == C3), both ways
    ks = [5, 6, 7]
    c1 = b"".join(pm.enc_xy(pyec.mul(C, k, pyec.G(C))) for k in ks)
    c3 = [pm.sm3(b"".join(pm.shared(k, Q))) for k in ks]
    c3[1] = bytes([c3[1][0] ^ 0x10]) + c3[1][1:]
    m, ok = device_decrypt(eng, enc32([D] * 3), c1, b"", 0, b"".join(c3))
    assert (m, ok) == (b"", [1, 0, 1])
    assert pm.decrypt(D, pyec.mul(C, 5, pyec.G(C)), b"", c3[0]) == b"" and pm.decrypt(D, pyec.mul(C, 6, pyec.G(C)), b"", c3[1]) is None


def test_no_elements_and_null_arrays(eng, Q):
    mod = ecgpu_module()
    lib, ctx, sz = eng._lib, eng._ctx, ctypes.c_size_t
    assert lib.ecgpu_sm2_pke_encrypt_batch(ctx, None, None, None, sz(4), sz(0), None, None, None, None) == 0
    assert lib.ecgpu_sm2_pke_decrypt_batch(ctx, None, None, None, sz(4), None, sz(0), None, None) == 0
    buf = (ctypes.c_uint8 * 128)()
    for hole in range(8):
        args = [buf] * 8
        args[hole] = None
        rc = lib.ecgpu_sm2_pke_encrypt_batch(ctx, args[0], args[1], args[2], sz(4), sz(1), args[3], args[4], args[5], args[6]) \
            if hole < 7 else lib.ecgpu_sm2_pke_encrypt_batch(ctx, buf, buf, buf, sz(2 ** 32), sz(1), buf, buf, buf, buf)
        assert rc == ERR_ARG, hole
        assert b"ecgpu_sm2_pke_encrypt_batch" in lib.ecgpu_last_error(ctx)
    for hole in range(7):
        args = [buf] * 7
        args[hole] = None
        rc = lib.ecgpu_sm2_pke_decrypt_batch(ctx, args[0], args[1], args[2], sz(4), args[3], sz(1), args[4], args[5]) \
            if hole < 6 else lib.ecgpu_sm2_pke_decrypt_batch(ctx, buf, buf, buf, sz(2 ** 32), buf, sz(1), buf, buf)
        assert rc == ERR_ARG, hole
        assert b"ecgpu_sm2_pke_decrypt_batch" in lib.ecgpu_last_error(ctx)
    assert device_encrypt(eng, pm.enc_xy(Q), enc32([5]), b"m", 1)[3] == [1]


def test_asynchronous_context(eng, Q):
    rng = random.Random("gpu-pke-async")
    n, msg_len = 70, 45
    ks = [rng.randrange(1, C.n) for _ in range(n)]
    ks[9] = 0                                             # a bad element is a verdict, not a deferred error
    msgs = rand_bytes(rng, n * msg_len)
    pk = pm.enc_xy(Q) * n
    sync = device_encrypt(eng, pk, enc32(ks), msgs, msg_len)
    eng.set_async(True)
    try:
        got = device_encrypt(eng, pk, enc32(ks), msgs, msg_len)
        dec = device_decrypt(eng, enc32([D] * n), got[0], got[1], msg_len, got[2])
        eng.synchronize()
    finally:
        eng.set_async(False)
    assert got == sync and got[3] == [int(i != 9) for i in range(n)]
    want = model_encrypt_batch(pk, [k or 1 for k in ks], msgs, msg_len)
    for i in range(n):
        if i != 9:
            assert (got[0][64 * i:64 * i + 64], got[1][i * msg_len:(i + 1) * msg_len], got[2][32 * i:32 * i + 32]) == \
                (want[0][64 * i:64 * i + 64], want[1][i * msg_len:(i + 1) * msg_len], want[2][32 * i:32 * i + 32]), i
            assert dec[0][i * msg_len:(i + 1) * msg_len] == msgs[i * msg_len:(i + 1) * msg_len]
    assert dec[1] == got[3] and dec[0][9 * msg_len:10 * msg_len] == bytes(msg_len)


# ---- the pipelined path ----------------------------------------------------------------------------------------------------
def test_pipelined_path_round_trip(eng):
    """`staged` cuts from 2^19 elements on into chunks of 2^18: n = 2^19 + 1, msg_len = 5 (chunk bases on odd offsets)"""
    n, msg_len = 2 ** 19 + 1, 5
    rng = np.random.default_rng(0x5D2)
    def scalars():
        s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        s[:, 0] &= 0x7F                                   # below n
        s[:, 31] |= 1                                     # not zero
        return s.reshape(-1)
    d, k = scalars(), scalars()
    msgs = rng.integers(0, 256, n * msg_len, dtype=np.uint8)
    pk, inf = eng.mul_by_generator(SM2, d)
    assert not inf.any()
    c1, c2, c3, ok = eng.sm2_pke_encrypt(pk, k, msgs, msg_len)
    assert ok.all()
    m, ok2 = eng.sm2_pke_decrypt(d, c1, c2, msg_len, c3)
    assert ok2.all() and bytes(m) == bytes(msgs)
    pick = [0, 2 ** 18 - 1, 2 ** 18, 2 ** 19 - 1, 2 ** 19] + [int(v) for v in np.random.default_rng(59).integers(0, n, 59)]
    for i in pick:
        di, ki = int.from_bytes(bytes(d[32 * i:32 * i + 32]), "big"), int.from_bytes(bytes(k[32 * i:32 * i + 32]), "big")
        P = pyec.mul(C, di, pyec.G(C))
        assert bytes(pk[64 * i:64 * i + 64]) == pm.enc_xy(P), i
        C1, C2, C3 = pm.encrypt(P, ki, bytes(msgs[i * msg_len:(i + 1) * msg_len]))
        assert (bytes(c1[64 * i:64 * i + 64]), bytes(c2[i * msg_len:(i + 1) * msg_len]), bytes(c3[32 * i:32 * i + 32])) == \
            (pm.enc_xy(C1), C2, C3), i


# ---- the wipe --------------------------------------------------------------------------------------------------------------
def test_scratch_reads_zero_behind_the_calls(Q):
    """Every buffer that held k, d, x2 || y2, the sanitised copies or a staged secret is zero once the call has returned, read
    back through the library's test hook (which a variable-time call, which wipes nothing, must show as not zero first)."""
    e = ecgpu_module().Engine(0)
    try:
        hook = e._lib.ecgpu_testhook_wiped_scratch_nonzero
        hook.restype = ctypes.c_longlong
        rng = random.Random("gpu-pke-wipe")
        n, msg_len = 300, 33
        ks = [rng.randrange(1, C.n) for _ in range(n)]
        e.mul_by_generator(SM2, enc32(ks))
        assert hook(e._ctx) > 0
        e.wipe()
        assert hook(e._ctx) == 0
        msgs = rand_bytes(rng, n * msg_len)
        c1, c2, c3, ok = e.sm2_pke_encrypt(pm.enc_xy(Q) * n, enc32(ks), msgs, msg_len)
        assert ok.all()
        assert hook(e._ctx) == 0
        m, ok = e.sm2_pke_decrypt(enc32([D] * n), c1, c2, msg_len, c3)
        assert ok.all() and bytes(m) == msgs
        assert hook(e._ctx) == 0
    finally:
        e.close()


def test_c_sm2_pke_example_runs():
    """examples/sm2_pke.c: the reference's ciphertext, a round trip and a tampered ciphertext from plain C"""
    import subprocess
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["make", "-s", "-C", ex, "sm2_pke"])
    out = subprocess.run([os.path.join(ex, "sm2_pke")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": yes") == 3 and "NO" not in out.stdout
