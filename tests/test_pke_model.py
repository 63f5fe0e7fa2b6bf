"""tests/pke_model.py against the reference's vectors (tests/golden/sm2pke.json, from sm2/tests/sm2pke.rs) and against itself over the
message lengths the kernels' edges sit at.  CPU only."""
import json
import os
import random

import pytest

import pke_model as pm
import pyec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "sm2pke.json")))
D = int(VEC["private_key"], 16)
MSG = bytes.fromhex(VEC["msg"])


def der_four_fields(der):
    """SEQUENCE { INTEGER x, INTEGER y, OCTET STRING c3, OCTET STRING c2 } -> (x, y, c3, c2); short and one-byte long lengths"""
    def tlv(buf, at):
        tag, ln, at = buf[at], buf[at + 1], at + 2
        if ln & 0x80:
            nb = ln & 0x7F
            ln, at = int.from_bytes(buf[at:at + nb], "big"), at + nb
        return tag, buf[at:at + ln], at + ln
    tag, body, end = tlv(der, 0)
    assert tag == 0x30 and end == len(der)
    fields, at = [], 0
    for want in (0x02, 0x02, 0x04, 0x04):
        tag, val, at = tlv(body, at)
        assert tag == want
        fields.append(val)
    assert at == len(body)
    return int.from_bytes(fields[0], "big"), int.from_bytes(fields[1], "big"), fields[2], fields[3]


def test_extractor_regenerates_the_golden_file_shape():
    assert sorted(VEC) == ["asn1_cipher", "cipher", "msg", "private_key"]
    assert MSG == b"plaintext" and len(bytes.fromhex(VEC["cipher"])) == 106 and len(bytes.fromhex(VEC["asn1_cipher"])) == 116


def test_model_decrypts_the_reference_cipher():
    C1, C2, C3 = pm.split_cipher(bytes.fromhex(VEC["cipher"]))
    assert pm.decrypt(D, C1, C2, C3) == MSG


def test_model_decrypts_the_reference_asn1_cipher():
    x, y, c3, c2 = der_four_fields(bytes.fromhex(VEC["asn1_cipher"]))
    assert len(c3) == 32
    assert pm.decrypt(D, (x, y), c2, c3) == MSG


@pytest.mark.parametrize("msg_len", pm.LENGTHS)
def test_round_trip(msg_len):
    rng = random.Random(msg_len)
    d, k = rng.randrange(1, pm.C.n), rng.randrange(1, pm.C.n)
    P = pyec.mul(pm.C, d, pyec.G(pm.C))
    M = bytes(rng.getrandbits(8) for _ in range(msg_len))
    C1, C2, C3 = pm.encrypt(P, k, M)
    assert len(C2) == msg_len and C2 != M
    assert pm.decrypt(d, C1, C2, C3) == M
    assert pm.decrypt(d, C1, C2, bytes([C3[0] ^ 1]) + C3[1:]) is None
    assert pm.decrypt(d, C1, bytes([C2[0] ^ 1]) + C2[1:], C3) is None


def test_rejections_and_the_zero_keystream_nonces():
    P = pyec.mul(pm.C, D, pyec.G(pm.C))
    for k in pm.ZERO_KEYSTREAM_NONCES:
        assert pm.encrypt(P, k, b"\x5a") is None             # t = one zero byte: the reference's loop draws again
        assert pm.encrypt(P, k, b"\x5a\xa5") is not None
    for k in (0, pm.C.n, 2 ** 256 - 1):
        assert pm.encrypt(P, k, b"m") is None
    assert pm.encrypt((P[0], P[1] ^ 1), 5, b"m") is None and pm.encrypt((pm.C.p, P[1]), 5, b"m") is None
    assert pm.encrypt(P, 5, b"") is None
