"""tests/sign_model.py pinned to the reference's signing vectors (tests/golden/signing.json, the per-set `ecdsa` records and the
Ethereum example of k256.json) and to pyec's arithmetic.  CPU only."""
import hashlib
import json
import os
import random

import pytest

import pyec
import sign_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


SIGNING = golden("signing")


@pytest.mark.parametrize("name", ["k256", "p256", "p384", "p224", "p192", "p521"])
def test_caller_nonce_records(name):
    c = pyec.CURVES[name]
    vec = golden(name)["ecdsa"]
    assert vec
    for v in vec:
        d, k, z = (int(v[f], 16) for f in ("d", "k", "m"))
        sig, recid, ok = sm.ecdsa_sign(c, d, k, z, False)          # the records are not low-S normalised
        assert ok == 1 and sig.hex() == v["r"].rjust(2 * c.L, "0") + v["s"].rjust(2 * c.L, "0")
        # the recovery id leads back to the record's public key
        Q = pyec.ecdsa_recover(c, z, int(v["r"], 16), int(v["s"], 16), recid)
        assert Q == (int(v["q_x"], 16), int(v["q_y"], 16))


@pytest.mark.parametrize("name", sorted(SIGNING["rfc6979"]))
def test_rfc6979_vectors(name):
    c = pyec.CURVES[name]
    for v in SIGNING["rfc6979"][name]:
        sig, recid, ok = sm.ecdsa_sign_msg(c, int(v["d"], 16), v["msg"].encode(), sm.NORMALIZE_S.get(name, False))
        assert ok == 1 and sig.hex() == v["sig"]


@pytest.mark.parametrize("name", sorted(SIGNING["prehash"]))
def test_prehash_vectors(name):
    c = pyec.CURVES[name]
    v = SIGNING["prehash"][name]
    digest = hashlib.new(v["hash"], v["msg"].encode()).digest()
    assert len(digest) != c.L                                       # the point of these vectors: bits2field truncates / pads
    sig, recid, ok = sm.ecdsa_sign_rfc6979(c, int(v["d"], 16), sm.bits2field(c, digest), False)
    assert ok == 1 and sig.hex() == v["sig"]


def test_ethereum_example():
    v = [r for r in golden("k256")["recovery"] if "secret_key" in r]
    assert len(v) == 1
    v = v[0]
    z = int.from_bytes(pyec.keccak256(bytes.fromhex(v["msg_hex"])), "big")
    sig, recid, ok = sm.ecdsa_sign_rfc6979(pyec.K256, int(v["secret_key"], 16), z, True)
    assert ok == 1 and sig.hex() == v["sig"] and recid == v["recid"]


def test_bip340_sign_vectors():
    assert [v["index"] for v in SIGNING["bip340_sign"]] == [0, 1, 2, 3]
    for v in SIGNING["bip340_sign"]:
        sig, ok = sm.schnorr_sign_raw(bytes.fromhex(v["secret_key"]), bytes.fromhex(v["message"]), bytes.fromhex(v["aux_rand"]))
        assert ok == 1 and sig.hex() == v["signature"], v["index"]


def test_midstates():
    # the constants of ecgpu_sha256.h / ecgpu_sign.h
    src = os.path.join(os.path.dirname(GOLDEN), "..", "elliptic-curves_amd", "csrc")
    text = open(os.path.join(src, "ecgpu_sign.h")).read() + open(os.path.join(src, "ecgpu_sha256.h")).read()
    flat = "".join(text.split()).lower()
    for tag in (b"BIP0340/challenge", b"BIP0340/aux", b"BIP0340/nonce"):
        want = ",".join("0x%08xu" % w for w in sm.sha256_midstate(tag))
        assert want in flat, tag


def test_mul_g_against_pyec():
    rng = random.Random(0x51610)
    for name in sm.ECDSA_SETS:
        c = pyec.CURVES[name]
        for k in [0, 1, 2, c.n - 1, c.n] + [rng.randrange(c.n) for _ in range(3)]:
            assert sm.mul_g(c, k) == pyec.mul(c, k, pyec.G(c)), (name, k)


def test_edges_and_low_s():
    c = pyec.K256
    for d, k in ((0, 5), (c.n, 5), (5, 0), (5, c.n), (2 ** 256 - 1, 5)):
        assert sm.ecdsa_sign(c, d, k, 1, True) == (bytes(64), 0, 0)
    rng = random.Random(7)
    seen = set()
    for _ in range(40):
        d, k, z = rng.randrange(1, c.n), rng.randrange(1, c.n), rng.getrandbits(256)
        a, ra, _ = sm.ecdsa_sign(c, d, k, z, False)
        b, rb, _ = sm.ecdsa_sign(c, d, k, z, True)
        high = int.from_bytes(a[32:], "big") > (c.n - 1) // 2
        seen.add(high)
        assert (a != b) == high and (ra ^ rb) == int(high)
        assert int.from_bytes(b[32:], "big") <= (c.n - 1) // 2
        Q = sm.mul_g(c, d)
        for sig, rid in ((a, ra), (b, rb)):
            r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
            assert pyec.ecdsa_verify(c, Q, z, r, s) and pyec.ecdsa_recover(c, z, r, s, rid) == Q
    assert seen == {True, False}


def test_brainpool_rejections_and_cap():
    """The brainpool orders are well below 2^(8L): a third or more of the elements reject at least once."""
    rng = random.Random(0xB9)
    for name in ("bp256", "bp384"):
        c = pyec.CURVES[name]
        rej = [sm.rfc6979_nonce(c, rng.randrange(1, c.n), rng.getrandbits(8 * c.L))[1] for _ in range(300)]
        assert 0.2 < sum(1 for r in rej if r) / len(rej) < 0.6 and max(rej) >= 3
    c = pyec.BP256
    d, z = next((d, z) for d, z in ((rng.randrange(1, c.n), rng.getrandbits(256)) for _ in range(4000))
                if sm.rfc6979_nonce(c, d, z)[1] >= 3)
    assert sm.ecdsa_sign_rfc6979(c, d, z, False, cap=3) == (bytes(64), 0, 0)
    assert sm.ecdsa_sign_rfc6979(c, d, z, False, cap=sm.rfc6979_nonce(c, d, z)[1] + 1)[2] == 1
