"""tests/sm2sign_model.py pinned to the known answer of GB/T 32918.5-2017 Annex A (tests/golden/sm2dsa_sign.json) and held against
the two verifiers the suite already trusts: the oracle's SM2DSA verification and pyec's.  CPU only."""
import json
import os
import random

import numpy as np
import pytest

import pyec
import sm2sign_model as m
from gpu_common import SM2DSA_KAT

VEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sm2dsa_sign.json")))
N = m.N


def xy(Q):
    return pyec.enc_point(m.C, Q)[0]


def test_the_standards_known_answer():
    d, k = int(VEC["d"], 16), int(VEC["k"], 16)
    distid, msg = VEC["distid"].encode(), VEC["msg"].encode()
    PA = m.public_key(d)
    assert "%064X" % PA[0] == VEC["pa_x"]
    assert pyec.sm2_za(m.C, distid, PA).hex().upper() == VEC["z"]
    e = m.message_hash(distid, PA, msg)
    assert "%064X" % e == VEC["e"]
    sig, ok = m.sign(d, k, e)
    assert ok == 1 and sig.hex().upper() == VEC["r"] + VEC["s"]
    # the first RFC 6979 / HMAC-SM3 candidate for this (d, e): a model value, pinned here and in the device code's twin
    assert m.rfc6979_candidate(d, e) == (int(VEC["rfc6979_candidate"], 16), True)
    sig2, ok2 = m.sign_msg(distid, d, msg)
    assert ok2 == 1 and (sig2, 1) == m.sign(d, int(VEC["rfc6979_candidate"], 16), e)


def test_the_generator_is_sign_models_with_sm3_and_one_candidate():
    rng = random.Random("sm2sign-model-gen")
    for _ in range(20):
        d, e = rng.randrange(1, N), rng.getrandbits(256)
        k, ok = m.rfc6979_candidate(d, e)
        assert ok and (k, 0) == m.sign_model.rfc6979_nonce(m.C, d, e, cap=m.sign_model.MAX_CANDIDATES)
        assert m.rfc6979_candidate(d, e % N) == (k, True)                                 # h1 = e mod n


def test_prehash_signatures_verify(oracle):
    rng = random.Random("sm2sign-model-prehash")
    n = 48
    ds = [rng.randrange(1, N - 1) for _ in range(n)]
    es = [rng.getrandbits(256) for _ in range(n)]
    sigs = []
    for i, (d, e) in enumerate(zip(ds, es)):
        sig, ok = m.sign_rfc6979(d, e) if i % 2 else m.sign(d, rng.randrange(1, N), e)
        assert ok == 1
        sigs.append(sig)
    qs = [m.public_key(d) for d in ds]
    enc = lambda vals: b"".join(v.to_bytes(32, "big") for v in vals)
    got = oracle.sm2dsa_verify(enc(es), b"".join(s[:32] for s in sigs), b"".join(s[32:] for s in sigs), b"".join(xy(Q) for Q in qs))
    assert bytes(got) == bytes([1] * n)
    for Q, e, s in zip(qs, es, sigs):
        assert pyec.sm2dsa_verify(m.C, Q, e, int.from_bytes(s[:32], "big"), int.from_bytes(s[32:], "big"))
    # and a signature under another prehash does not
    assert not oracle.sm2dsa_verify(enc([es[0] ^ 1]), sigs[0][:32], sigs[0][32:], xy(qs[0]))[0]


@pytest.mark.parametrize("distid", [b"", b"1234567812345678", bytes(range(100))], ids=["empty", "default", "100 bytes"])
def test_message_signatures_verify(oracle, distid):
    rng = random.Random("sm2sign-model-msg-%d" % len(distid))
    for msg_len in (0, 7, 32, 100):
        n = 6
        ds = [rng.randrange(1, N - 1) for _ in range(n)]
        msgs = bytes(rng.getrandbits(8) for _ in range(n * msg_len))
        out = [m.sign_msg(distid, d, msgs[i * msg_len:(i + 1) * msg_len]) for i, d in enumerate(ds)]
        assert all(ok for _, ok in out)
        q = b"".join(xy(m.public_key(d)) for d in ds)
        got = oracle.sm2dsa_verify_msg(distid, q, msgs, msg_len, b"".join(s for s, _ in out))
        assert bytes(got) == bytes([1] * n), msg_len
        for i, d in enumerate(ds):
            e = m.message_hash(distid, m.public_key(d), msgs[i * msg_len:(i + 1) * msg_len])
            assert pyec.sm2dsa_verify(m.C, m.public_key(d), e, int.from_bytes(out[i][0][:32], "big"), int.from_bytes(out[i][0][32:], "big"))


def test_unusable_inputs_give_a_zero_record():
    rng = random.Random("sm2sign-model-edges")
    for label, d, k, e in m.edge_cases(rng):
        sig, ok = m.sign(d, k, e)
        assert ok == (0 if label.startswith("fails") else 1), label
        assert (sig == bytes(64)) == (ok == 0), label
    assert m.sign_msg(b"id", 0, b"m") == m.ZERO and m.sign_msg(b"id", N - 1, b"m") == m.ZERO and m.sign_msg(b"id", N, b"m") == m.ZERO


def test_the_references_verification_vector_is_still_accepted(oracle):
    """sm2/tests/sm2dsa.rs: the message-level vector the verification tests use, through both verifiers"""
    K = SM2DSA_KAT
    pk, sig = bytes.fromhex(K["public_key"])[1:], bytes.fromhex(K["signature"])
    assert bytes(oracle.sm2dsa_verify_msg(K["identity"], pk, K["message"], len(K["message"]), sig)) == b"\x01"
    Q = pyec.dec_point(m.C, pk, 0)
    e = m.message_hash(K["identity"], Q, K["message"])
    assert pyec.sm2dsa_verify(m.C, Q, e, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big"))
    assert np.array_equal(oracle.sm2dsa_verify(e.to_bytes(32, "big"), sig[:32], sig[32:], pk), np.array([1], np.uint8))
