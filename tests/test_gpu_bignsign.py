"""Batch bign signing on the device (ecgpu_bign_sign_batch / _sign_prehash_batch / _sign_msg_batch; host-pointer forms only) against
tests/bignsign_model.py: the reference's vector through the three forms, batches on the wave and workgroup boundaries forwards and
reversed, the belt-hash block edges, prehashes >= q (the generator takes the reduced value, S0 the raw bytes), the refusals that have
to be constructed planted among good elements, the generator kernels with a smaller bound (the retry path), the finish kernel on an S0
handed in directly, the wipe and the C example.

One reference batch of 257 elements is computed once (the model's arithmetic, with R = k G from the oracle's C code) and every batch
size is a prefix of it: elements are independent."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib
import pyec
import bignsign_model as m
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
ERR_ARG = -7
C = m.C
BIGN = C.cid
Q = m.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "bign_sign.json")))
D = int.from_bytes(bytes.fromhex(VEC["private_key"]), "little")
MSG, SIG = bytes.fromhex(VEC["msg"]), bytes.fromhex(VEC["sig"])
SIZES = [1, 63, 64, 65, 255, 256, 257]          # wave = 64 and block = 256: where a lane-indexed table stage or the parked state's stride goes wrong
SPOTS = [0, 63, 64, 255, 256]
NREF, MSG_LEN = 257, 13
GENK_SEED = "bignsign-genk-0"                   # tests/test_bignsign_model.py: at most 64 rounds at bound 2^254


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def enc32(values):
    return b"".join(m.le(int(v) % 2 ** 256) for v in values)


def rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "big") if n else b""


def xs_of(ks):
    """x(k G) for ks in [1, q) from the oracle's C code"""
    xy, inf = oracle_lib.batch_mul_base(BIGN, enc32(ks))
    assert not inf.any()
    xy = bytes(xy)
    return [int.from_bytes(xy[64 * i:64 * i + 32], "little") for i in range(len(ks))]


def model_sign(ds, ks, hs):
    """steps 3-7 for a batch, the multiplications batched -> [(sig, ok)]; an unusable k was multiplied as 1"""
    xs = xs_of([k if 1 <= k < Q else 1 for k in ks])
    out = []
    for d, k, h, x in zip(ds, ks, hs, xs):
        s0 = pyec.belt_hash(pyec.BELT_OID + m.le(x) + h)[:16]
        out.append(m.finish(d % 2 ** 256, k, True, h, s0))
    return out


def model_prehash(ds, hs):
    return model_sign(ds, [m.nonce(d, h) if 1 <= d < Q else 0 for d, h in zip(ds, hs)], hs)


def pack(out):
    return b"".join(s for s, _ in out), bytes(ok for _, ok in out)


def dev(got):
    return bytes(got[0]), bytes(got[1])


def cut(b, unit, idx):
    return b"".join(b[unit * i:unit * i + unit] for i in idx)


@pytest.fixture(scope="module")
def ref():
    rng = random.Random("gpu-bignsign-ref")
    r = {"ds": [rng.randrange(1, Q) for _ in range(NREF)], "ks": [rng.randrange(1, Q) for _ in range(NREF)],
         "hs": [m.le(rng.getrandbits(256)) for _ in range(NREF)], "msgs": rand_bytes(rng, NREF * MSG_LEN)}
    r["mh"] = [pyec.belt_hash(r["msgs"][i * MSG_LEN:(i + 1) * MSG_LEN]) for i in range(NREF)]
    r["q"] = bytes(oracle_lib.batch_mul_base(BIGN, enc32(r["ds"]))[0])
    assert r["q"][:64] == pyec.enc_point(C, m.public_key(r["ds"][0]))[0]
    r["nonce"] = pack(model_sign(r["ds"], r["ks"], r["hs"]))
    r["pre"] = pack(model_prehash(r["ds"], r["hs"]))
    r["msg"] = pack(model_prehash(r["ds"], r["mh"]))
    for f in ("nonce", "pre", "msg"):
        assert r[f][1] == b"\x01" * NREF                  # (no random element is refused: the refusals are constructed below)
    assert m.sign_prehash(r["ds"][3], r["hs"][3])[0] == r["pre"][0][48 * 3:48 * 4]        # the batched model is the model
    return r


def three_forms(eng, ds, ks, hs, msgs, msg_len):
    return {"nonce": dev(eng.bign_sign(enc32(ds), enc32(ks), b"".join(hs))), "pre": dev(eng.bign_sign_prehash(enc32(ds), b"".join(hs))),
            "msg": dev(eng.bign_sign_msg(enc32(ds), msgs, msg_len))}


def test_the_references_vector_through_the_three_forms(eng):
    d = enc32([D])
    h = pyec.belt_hash(MSG)
    assert dev(eng.bign_sign_msg(d, MSG, len(MSG))) == (SIG, b"\x01")
    assert dev(eng.bign_sign_prehash(d, h)) == (SIG, b"\x01")
    assert dev(eng.bign_sign(d, enc32([m.nonce(D, h)]), h)) == (SIG, b"\x01")
    assert bytes(eng.bign_verify_msg(bytes.fromhex(VEC["public_key"]), MSG, len(MSG), SIG)) == b"\x01"


@pytest.mark.parametrize("order", ["forwards", "reversed"])
@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(eng, ref, n, order):
    idx = list(range(n)) if order == "forwards" else list(range(n - 1, -1, -1))
    ds, ks, hs = [ref["ds"][i] for i in idx], [ref["ks"][i] for i in idx], [ref["hs"][i] for i in idx]
    msgs, q = cut(ref["msgs"], MSG_LEN, idx), cut(ref["q"], 64, idx)
    got = three_forms(eng, ds, ks, hs, msgs, MSG_LEN)
    for f, (sig, ok) in got.items():
        assert ok == b"\x01" * n, f
        assert sig == cut(ref[f][0], 48, idx), f
    # every signature verifies on the device, on the prehash and on the message
    for f in ("nonce", "pre"):
        assert bytes(eng.bign_verify(b"".join(hs), got[f][0], q)) == b"\x01" * n, f
    assert bytes(eng.bign_verify_msg(q, msgs, MSG_LEN, got["msg"][0])) == b"\x01" * n
    assert bytes(eng.bign_verify(cut(b"".join(ref["mh"]), 32, idx), got["msg"][0], q)) == b"\x01" * n


@pytest.mark.parametrize("msg_len", [0, 13, 31, 32, 33, 64, 65])
def test_message_lengths_at_the_belt_hash_block_edges(eng, ref, msg_len):
    n = 5
    rng = random.Random("gpu-bignsign-len-%d" % msg_len)
    msgs = rand_bytes(rng, n * msg_len)
    ds = ref["ds"][:n]
    want = pack(model_prehash(ds, [pyec.belt_hash(msgs[i * msg_len:(i + 1) * msg_len]) for i in range(n)]))
    got = dev(eng.bign_sign_msg(enc32(ds), msgs, msg_len))
    assert got == want and want[1] == b"\x01" * n
    assert bytes(eng.bign_verify_msg(ref["q"][:64 * n], msgs, msg_len, got[0])) == b"\x01" * n


@pytest.mark.parametrize("which", [0, 1, 2], ids=["all-ff", "q", "q+1"])
def test_prehashes_at_or_above_q(eng, ref, which):
    """all 0xFF, q and q + 1, each at elements 0, 63, 64, 255 and 256 of a batch of 257: the generator is fed H mod q, S0 the raw bytes"""
    hs = list(ref["hs"])
    for i in SPOTS:
        hs[i] = m.PREHASH_GE_Q[which]
    want = {"nonce": pack(model_sign(ref["ds"], ref["ks"], hs)), "pre": pack(model_prehash(ref["ds"], hs))}
    got = {"nonce": dev(eng.bign_sign(enc32(ref["ds"]), enc32(ref["ks"]), b"".join(hs))),
           "pre": dev(eng.bign_sign_prehash(enc32(ref["ds"]), b"".join(hs)))}
    for f in want:
        assert got[f] == want[f] and want[f][1] == b"\x01" * NREF, f
        assert bytes(eng.bign_verify(b"".join(hs), got[f][0], ref["q"])) == b"\x01" * NREF, f
    for i in range(NREF):
        mine = got["pre"][0][48 * i:48 * i + 48]
        if i in SPOTS:                                                        # the other reading is NOT what the device computes
            assert mine != m.sign_prehash(ref["ds"][i], hs[i], reduce_h=False)[0], i
        else:                                                                 # every other element is the reference batch's
            assert mine == ref["pre"][0][48 * i:48 * i + 48], i


def test_constructed_refusals_at_the_boundaries(eng, ref):
    """every refusal at elements 0, 63, 64, 255, 256 of a batch of 257: ok = 0 and a zero record there, the neighbours untouched"""
    rng = random.Random("gpu-bignsign-refusals")
    for label, d, k, h in m.refusals(rng):
        ds, ks, hs = list(ref["ds"]), list(ref["ks"]), list(ref["hs"])
        for i in SPOTS:
            ds[i], ks[i], hs[i] = d, k, h
        sig, ok = dev(eng.bign_sign(enc32(ds), enc32(ks), b"".join(hs)))
        forms = [("nonce", sig, ok)]
        if label.startswith("d ="):                                           # an unusable key is refused by the other two forms too
            forms.append(("pre", *dev(eng.bign_sign_prehash(enc32(ds), b"".join(ref["hs"])))))
            forms.append(("msg", *dev(eng.bign_sign_msg(enc32(ds), ref["msgs"], MSG_LEN))))
        for f, sig, ok in forms:
            for i in range(NREF):
                if i in SPOTS:
                    assert ok[i] == 0 and sig[48 * i:48 * i + 48] == bytes(48), (label, f, i)
                else:
                    assert ok[i] == 1 and sig[48 * i:48 * i + 48] == ref[f][0][48 * i:48 * i + 48], (label, f, i)


@pytest.mark.parametrize("bound", [1 << 254, 1 << 255, Q], ids=["2^254", "2^255", "q"])
def test_generator_kernels_with_the_callers_bound(eng, bound):
    """k_bign_genk and k_bign_genk_retry against the model, k and round count per element; at 2^254 three candidates in four are
    rejected, which no input achieves with q"""
    rng = random.Random(GENK_SEED)
    rows = [(rng.randrange(1, Q), rng.getrandbits(256)) for _ in range(257)]
    want = [m.genk(m.le(d), m.le(h % Q), bound) for d, h in rows]
    assert max(r for _, r in want) <= 64                                      # a condition on the seed, checked on the CPU as well
    k, rounds = eng.selftest_bign_genk(enc32([d for d, _ in rows]), enc32([h for _, h in rows]), m.le(bound))
    assert [int(r) for r in rounds] == [r for _, r in want]
    assert bytes(k) == enc32([kk for kk, _ in want])
    if bound == 1 << 254:
        assert {4, 8, 12} <= set(int(r) for r in rounds) and max(rounds) > 12


def test_finish_kernel_on_stages_no_input_produces(eng):
    """k_bign_sign_finish through ecgpu_selftest_sign_finish: S0 = 0, 1, 2^128 - 1 handed in directly, and a cleared flag"""
    mod = ecgpu_module()
    rng = random.Random("gpu-bignsign-finish")
    d, k, h = rng.randrange(1, Q), rng.randrange(1, Q), m.le(rng.getrandbits(256))
    rows = [(d, k, 1, h, s0) for s0 in (bytes(16), m.le(1, 16), m.le(2 ** 128 - 1, 16))]
    rows += [(d, k, 0, h, m.le(5, 16)), (d, 1, 0, h, m.le(5, 16)), (0, k, 1, h, m.le(5, 16)), (d, Q, 1, h, m.le(5, 16))]
    rows = rows * 37                                                          # 259 elements: more than one workgroup
    n = len(rows)
    rxy = b"".join(r[4] + bytes(48) for r in rows)
    sig, ok = eng.selftest_sign_finish(BIGN, mod.SIGN_SCHEME_BIGN, enc32([r[0] for r in rows]), enc32([r[1] for r in rows]),
                                       bytes(r[2] for r in rows), b"".join(r[3] for r in rows), rxy, bytes(n))
    want = [m.finish(*r) for r in rows]
    assert [o for _, o in want[:7]] == [0, 1, 1, 0, 0, 0, 0]
    assert (bytes(sig), bytes(ok)) == pack(want)
    # the identity flag of R (no k in [1, q) sets it) refuses too
    sig, ok = eng.selftest_sign_finish(BIGN, mod.SIGN_SCHEME_BIGN, enc32([d]), enc32([k]), b"\x01", h, m.le(5, 16) + bytes(48), b"\x01")
    assert (bytes(sig), bytes(ok)) == (bytes(48), b"\x00")
    with pytest.raises(mod.EcgpuError) as e:
        eng.selftest_sign_finish(mod.K256, mod.SIGN_SCHEME_BIGN, bytes(32), bytes(32), b"\x01", bytes(32), bytes(64), b"\x00")
    assert e.value.code != 0


def test_argument_errors(eng):
    mod = ecgpu_module()
    lib = eng._lib
    b = np.zeros(64, np.uint8)
    p = b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.ecgpu_bign_sign_batch(eng._ctx, p, None, p, ctypes.c_size_t(1), p, p) == ERR_ARG
    assert lib.ecgpu_bign_sign_prehash_batch(eng._ctx, p, p, ctypes.c_size_t(1), None, p) == ERR_ARG
    assert lib.ecgpu_bign_sign_msg_batch(eng._ctx, p, None, ctypes.c_size_t(3), ctypes.c_size_t(1), p, p) == ERR_ARG
    assert lib.ecgpu_selftest_bign_genk(eng._ctx, p, p, None, ctypes.c_size_t(1), p, p) == ERR_ARG
    sig, ok = eng.bign_sign_prehash(b"", b"")                                 # n = 0
    assert sig.size == 0 and ok.size == 0
    with pytest.raises(mod.EcgpuError):
        eng.bign_sign(bytes(32), bytes(31), bytes(32))


def test_wipe_and_the_parked_generator_state(eng, ref):
    """the staged keys, the nonces, S0 and the generator's parked state (theta, r1, r2, i) read back zero behind a call and after
    ecgpu_wipe, through the library's read-back hook (which a variable-time call, which wipes nothing, must show as not zero)"""
    e = ecgpu_module().Engine(0)
    try:
        hook = e._lib.ecgpu_testhook_wiped_scratch_nonzero
        hook.restype = ctypes.c_longlong
        n = 257
        e.mul_by_generator(BIGN, enc32(ref["ks"][:n]))
        assert hook(e._ctx) > 0
        e.wipe()
        assert hook(e._ctx) == 0
        got = dev(e.bign_sign_prehash(enc32(ref["ds"][:n]), b"".join(ref["hs"][:n])))
        assert got == (ref["pre"][0][:48 * n], b"\x01" * n)
        assert hook(e._ctx) == 0
        e.selftest_bign_genk(enc32(ref["ds"][:n]), b"".join(ref["hs"][:n]), m.le(1 << 254))
        assert hook(e._ctx) == 0
        e.wipe()
        assert hook(e._ctx) == 0
        assert dev(e.bign_sign_msg(enc32(ref["ds"][:n]), ref["msgs"][:n * MSG_LEN], MSG_LEN)) == (ref["msg"][0][:48 * n], b"\x01" * n)
    finally:
        e.close()


def test_c_bign_sign_example_runs():
    """examples/bign_sign.c: the reference's vector from plain C, verified on the device, and a refused key"""
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["make", "-s", "-C", ex, "bign_sign"])
    out = subprocess.run([os.path.join(ex, "bign_sign")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": yes") == 3 and "NO" not in out.stdout
    assert VEC["sig"] in out.stdout
