"""tests/bignsign_model.py pinned to the reference's own signature vector (bignp256/tests/ecdsa.rs:20-33, tests/golden/bign_sign.json):
with the nonce generator of STB 34.101.45 section 6.3.3 that vector is the deterministic signature of its key and message, so it pins
the generator, belt-hash and the finish step end to end.  The model's signatures are held against pyec's verifier, the prehashes >= q
separate the two readings of what the generator is fed, and the refusals are constructed.  CPU only."""
import json
import os
import random

import pyec
import bignsign_model as m

VEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bign_sign.json")))
Q = m.Q
D = int.from_bytes(bytes.fromhex(VEC["private_key"]), "little")
MSG, SIG = bytes.fromhex(VEC["msg"]), bytes.fromhex(VEC["sig"])
GENK_SEED = "bignsign-genk-0"                  # the model's maximum round count at bound 2^254 over 257 inputs is 64 with this seed


def genk_inputs(n=257, seed=GENK_SEED):
    rng = random.Random(seed)
    return [(rng.randrange(1, Q), rng.getrandbits(256)) for _ in range(n)]


def test_the_references_vector_is_the_deterministic_signature():
    assert pyec.enc_point(m.C, m.public_key(D))[0] == bytes.fromhex(VEC["public_key"])
    h = pyec.belt_hash(MSG)
    k, rounds = m.genk(m.le(D), m.le(int.from_bytes(h, "little") % Q))
    assert rounds == 4                                                     # the first candidate is accepted
    assert m.sign(D, k, h) == (SIG, 1)
    assert m.sign_prehash(D, h) == (SIG, 1) and m.sign_msg(D, MSG) == (SIG, 1)
    assert pyec.bign_verify(m.C, m.public_key(D), h, SIG)


def test_signatures_verify():
    rng = random.Random("bignsign-model-verify")
    for i in range(12):
        d, msg = rng.randrange(1, Q), bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 13, 32, 65))))
        sig, ok = m.sign_msg(d, msg)
        assert ok == 1 and pyec.bign_verify(m.C, m.public_key(d), pyec.belt_hash(msg), sig)
        h = m.le(rng.getrandbits(256))
        sig, ok = m.sign(d, rng.randrange(1, Q), h)
        assert ok == 1 and pyec.bign_verify(m.C, m.public_key(d), h, sig)
        assert not pyec.bign_verify(m.C, m.public_key(d), m.le(int.from_bytes(h, "little") ^ 1), sig)


def test_prehashes_at_or_above_q_feed_the_generator_the_reduced_value():
    rng = random.Random("bignsign-model-geq")
    for h in m.PREHASH_GE_Q:
        assert int.from_bytes(h, "little") >= Q
        d = rng.randrange(1, Q)
        sig, ok = m.sign_prehash(d, h)
        assert ok == 1 and pyec.bign_verify(m.C, m.public_key(d), h, sig)    # S0 absorbed the RAW bytes, as the verifier does
        other, ok2 = m.sign_prehash(d, h, reduce_h=False)                     # the other reading: raw H to the generator
        assert ok2 == 1 and other != sig
        assert m.nonce(d, h) == m.genk(m.le(d), m.le(int.from_bytes(h, "little") - Q))[0]
    h = m.le(Q - 1)                                                           # below q the two readings agree
    assert m.sign_prehash(5, h) == m.sign_prehash(5, h, reduce_h=False)


def test_round_counts_with_a_smaller_bound():
    rounds = [m.genk(m.le(d), m.le(h % Q), 1 << 254)[1] for d, h in genk_inputs()]
    assert {4, 8, 12} <= set(rounds) and max(rounds) > 12
    assert max(rounds) <= 64                                                  # what tests/test_gpu_bignsign.py relies on
    assert all(r % 4 == 0 for r in rounds)
    # three candidates in four are rejected: about a quarter of the elements stop at each of the first rounds
    assert 40 <= rounds.count(4) <= 90
    assert all(m.genk(m.le(d), m.le(h % Q))[1] == 4 for d, h in genk_inputs(16))   # with q itself nothing is rejected


def test_refusals_give_a_zero_record():
    rng = random.Random("bignsign-model-refusals")
    cases = m.refusals(rng)
    assert len(cases) == 7
    for label, d, k, h in cases:
        assert m.sign(d % 2 ** 256, k, h) == m.ZERO, label
    d, k, h = m.s1_zero_case(rng)
    s0 = m.s0_of(k, h)
    assert (k - int.from_bytes(h, "little") - (int.from_bytes(s0, "little") + m.TWO128) * d) % Q == 0
    assert m.finish(d, k, True, h, bytes(16)) == m.ZERO                       # S0 = 0, handed in directly
    assert m.finish(d + 1, k, True, h, s0)[1] == 1 and m.finish(d + 1, k, False, h, s0) == m.ZERO
    assert m.sign_prehash(0, h) == m.ZERO and m.sign_prehash(Q, h) == m.ZERO and m.sign_msg(Q, b"m") == m.ZERO
