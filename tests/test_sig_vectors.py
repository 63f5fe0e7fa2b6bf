"""The vectors of tests/sig_vectors.py against everything that runs without a GPU: the verdict the construction gives each vector
== the big-integer model (tests/pyec.py) == the oracle == the CPU build of the kernels' per-element code (tests/hostcheck), verdict
for verdict, and key for key where a key is recovered.  No family may be empty on a curve it applies to.
tests/test_gpu_sig_vectors.py runs the same vectors on gfx950; profiles/sig_vectors/mutations.txt records which statements of
csrc/ecgpu_verify.h these tests hold in place."""
import hashlib

import pytest

import hostcheck_lib as hc
import pyec
import sig_vectors as sv
import wycheproof_lib
from gpu_common import ALL_CURVES

BRAINPOOL = ("bp256", "bp384", "bp256t1", "bp384t1")


def check_families(scheme, curve, vec, extra=()):
    cnt = sv.counts(vec)
    for fam in sv.FAMILIES[scheme] + tuple(extra):
        assert cnt[fam] > 0, (scheme, curve, fam, "is empty")
    assert set(cnt) == set(sv.FAMILIES[scheme] + tuple(extra)), (scheme, curve, sorted(cnt))
    assert len({(v.family, v.label) + ((len(v.msg),) if hasattr(v, "msg") else ()) for v in vec}) == len(vec)   # every case is named once
    return cnt


def labels(vec, family):
    return [v.label for v in vec if v.family == family]


def test_the_curve_lists_are_the_projects():
    assert sv.ECDSA_CURVES == [c for c in ALL_CURVES if c != "sm2"]
    assert all(pyec.CURVES[c].p > pyec.CURVES[c].n for c in sv.ECDSA_CURVES + ["sm2", "bign256"])


@pytest.mark.parametrize("curve", sv.ECDSA_CURVES)
def test_ecdsa_prehash(oracle, curve):
    c = pyec.CURVES[curve]
    vec = sv.ecdsa_vectors(curve)
    cnt = check_families("ecdsa", curve, vec, ["edge_x_zero"] if pyec.lift_x(c, 0, 0) else [])
    assert 43 <= len(vec) <= 48
    assert cnt["x_ge_n"] == 13 and cnt["exceptional"] == 18                     # 5 s + 6 z + the r = x pair; six sums (nine cases) with z, z + n
    nc = labels(vec, "noncanonical")
    assert "key (x + p, y)" in nc and "r + n" in nc and "s + n" in nc
    assert ("key (x, y + p)" in nc) == (curve == "p521" or curve in BRAINPOOL)  # NIST and k256: 2^(8L) - p is below 2^-32 of the field
    assert sv.skipped("ecdsa", curve)["noncanonical"] == (0 if "key (x, y + p)" in nc else 1)
    # both holes the suite had: accepted signatures whose x(R) is at or above n, and rejected keys that are valid once reduced
    assert sum(v.exp for v in vec if v.family == "x_ge_n") == 12
    assert any(not v.exp and v.qx >= c.p and pyec.on_curve(c, (v.qx - c.p, v.qy)) for v in vec)
    # the exact high-S boundary, accepted on one side only
    hs = {v.label: (v.exp, v.exp_hs) for v in vec if v.family == "x_ge_n"}
    assert hs["s = (n - 1) / 2"] == (True, True) and hs["s = (n + 1) / 2"] == (True, False)
    z, r, s, q, exp, exp_hs = sv.pack_ecdsa(c, vec)
    for high, want in ((False, exp), (True, exp_hs)):
        model = bytes(int(pyec.ecdsa_verify(c, (v.qx, v.qy), v.z, v.r, v.s, high)) for v in vec)
        got_o, got_h = bytes(oracle.ecdsa_verify(c.cid, z, r, s, q, high)), bytes(hc.ecdsa_verify(c.cid, z, r, s, q, high))
        for i, v in enumerate(vec):
            assert want[i] == model[i] == got_o[i] == got_h[i], (curve, high, v.family, v.label, want[i], model[i], got_o[i], got_h[i])


@pytest.mark.parametrize("curve", sv.MSG_CURVES)
def test_ecdsa_messages(oracle, curve):
    c = pyec.CURVES[curve]
    vec = sv.ecdsa_msg_vectors(curve)
    check_families("ecdsa_msg", curve, vec)
    nc = labels(vec, "noncanonical")
    assert nc.count("s + n") == 2
    # a key cannot be chosen under a fixed digest: x + p, y + p only where derived keys leave room for p
    assert (nc.count("key (x + p, y)"), nc.count("key (x, y + p)")) == ((2, 2) if curve == "p521" or curve in BRAINPOOL else (0, 0))
    assert sorted(sv.by_len(vec)) == sorted(sv.MSG_LENS)
    for ln, part in sv.by_len(vec).items():
        q, m, sg, exp, exp_hs = sv.pack_ecdsa_msg(c, part)
        zs = b"".join(wycheproof_lib.bits2field(hashlib.new(sv.DIGEST[curve], v.msg).digest(), c.L) for v in part)
        assert hc.ecdsa_hash_msg(c.cid, m, ln) == zs
        r, s = (b"".join(sg[i * 2 * c.L + k * c.L: i * 2 * c.L + (k + 1) * c.L] for i in range(len(part))) for k in (0, 1))
        for high, want in ((False, exp), (True, exp_hs)):
            model = bytes(int(pyec.ecdsa_verify(c, (v.qx, v.qy), int.from_bytes(zs[i * c.L:(i + 1) * c.L], "big"), v.r, v.s, high))
                          for i, v in enumerate(part))
            got_o, got_h = bytes(oracle.ecdsa_verify_msg(c.cid, q, m, ln, sg, high)), bytes(hc.ecdsa_verify(c.cid, zs, r, s, q, high))
            for i, v in enumerate(part):
                assert want[i] == model[i] == got_o[i] == got_h[i], (curve, ln, high, v.family, v.label)
        assert any(exp) and not all(exp)


@pytest.mark.parametrize("curve", sv.ECDSA_CURVES)
def test_recovery(oracle, curve):
    c = pyec.CURVES[curve]
    vec = sv.recover_vectors(curve)
    check_families("recover", curve, vec, [] if curve == "p521" else ["carry_trap"])     # 66 bytes hold r + n
    trap = [v for v in vec if v.family == "carry_trap" and v.recid & 2]
    for v in trap:                                               # a sum without its carry would find a point
        assert v.exp is None and pyec.lift_x(c, (v.r + c.n) % (1 << (8 * c.L)), v.recid & 1) is not None
    assert all(v.exp is None for v in vec if v.family == "largest_r" and v.recid & 2)
    hs = {v.label: (v.exp is not None, v.exp_hs is not None) for v in vec if v.family == "high_s"}
    assert hs == {"s = (n - 1) / 2": (True, True), "s = (n + 1) / 2": (True, False)}
    z, r, s, recid, plain, high_s = sv.pack_recover(c, vec)
    for high, (want_xy, want_ok) in ((False, plain), (True, high_s)):
        for i, v in enumerate(vec):
            Q = pyec.ecdsa_recover(c, v.z, v.r, v.s, v.recid, high)
            assert Q == (v.exp_hs if high else v.exp), (curve, high, v.family, v.label)
        for lib in (oracle, hc):
            out, ok = lib.ecdsa_recover(c.cid, z, r, s, recid, high)
            for i, v in enumerate(vec):
                assert ok[i] == want_ok[i] and bytes(out[i * 2 * c.L:(i + 1) * 2 * c.L]) == want_xy[i * 2 * c.L:(i + 1) * 2 * c.L], \
                    (curve, high, lib.__name__, v.family, v.label)


def bip340_model(c, P, e, r, s):
    """BIP340 verification with the challenge given, on the big-integer model: the key's parity is not looked at"""
    if r >= c.p or not 0 < s < c.n or not pyec.on_curve(c, P):
        return False
    R = pyec.add(c, pyec.mul(c, s, pyec.G(c)), pyec.mul(c, -e % c.n, P))
    return R is not pyec.INF and R[1] % 2 == 0 and R[0] == r


def test_schnorr_challenge_given(oracle):
    c = pyec.K256
    vec = sv.schnorr_vectors("k256")
    check_families("schnorr", "k256", vec)
    assert any(v.exp and v.r >= c.n for v in vec)                # r >= n is valid: the rule is r < p
    e, r, s, pxy, exp = sv.pack_schnorr(vec)
    got_o, got_h = bytes(oracle.schnorr_verify(e, r, s, pxy)), bytes(hc.schnorr_verify(e, r, s, pxy))
    for i, v in enumerate(vec):
        want = got_o[i] if v.exp is None else int(v.exp)         # odd-y keys: the oracle's restatement of the reference decides
        assert want == got_o[i] == got_h[i] == int(bip340_model(c, (v.px, v.py), v.e, v.r, v.s)), (v.family, v.label)
    assert all(v.py & 1 for v in vec if v.family == "odd_key")


def test_schnorr_from_wire_bytes(oracle):
    c = pyec.K256
    vec = sv.schnorr_raw_vectors("k256")
    check_families("schnorr_raw", "k256", vec)
    for ln, part in sv.by_len(vec).items():
        pk, m, sg, exp = sv.pack_schnorr_raw(part)
        got_o, got_h = bytes(oracle.schnorr_verify_raw(pk, m, ln, sg)), bytes(hc.schnorr_verify_raw(pk, m, ln, sg))
        for i, v in enumerate(part):
            P = pyec.lift_x(c, v.pkx, 0)
            ch = int.from_bytes(sv._tagged(b"BIP0340/challenge", v.r.to_bytes(32, "big") + v.pkx.to_bytes(32, "big") + v.msg), "big")
            model = P is not None and bip340_model(c, P, ch, v.r, v.s)
            assert int(v.exp) == got_o[i] == got_h[i] == int(model), (ln, v.family, v.label)
        assert sum(exp) == 1


def test_sm2dsa_prehash(oracle):
    c = pyec.CURVES["sm2"]
    vec = sv.sm2dsa_vectors("sm2")
    check_families("sm2dsa", "sm2", vec)
    ident = [v for v in vec if v.family == "identity"]
    assert ident[0].exp is True                                  # x1 = 0 for the identity, as the reference takes it
    assert any(v.r + v.s >= 1 << 256 and v.exp for v in vec)     # the carry of r + s
    e, r, s, q, exp = sv.pack_sm2dsa(vec)
    got_o, got_h = bytes(oracle.sm2dsa_verify(e, r, s, q)), bytes(hc.sm2dsa_verify(e, r, s, q))
    for i, v in enumerate(vec):
        assert exp[i] == got_o[i] == got_h[i] == int(pyec.sm2dsa_verify(c, (v.qx, v.qy), v.e, v.r, v.s)), (v.family, v.label)


def test_bign_prehash_and_messages(oracle):
    c = pyec.CURVES["bign256"]
    vec = sv.bign_vectors("bign256")
    check_families("bign", "bign256", vec)
    s0s = {v.label: v for v in vec if v.family == "s0_extremes"}
    assert s0s["S0 with its top bit set"].s0 >> 127 and s0s["S0 with its top bit set"].exp
    assert s0s["S0 with a zero top byte"].s0 < 1 << 120 and s0s["S0 with a zero top byte"].exp
    assert any(v.exp and v.s1 + v.h >= 1 << 256 for v in vec)    # the carry of S1 + H
    assert any(v.exp and (v.s1 + v.h % c.n) % c.n == 0 for v in vec)
    assert any(not v.exp and v.qx == c.p for v in vec)           # (p, y) reduces to the generator (0, y): a point of the curve
    h, sg, q, exp = sv.pack_bign(vec)
    got_o, got_h = bytes(oracle.bign_verify(h, sg, q)), bytes(hc.bign_verify(h, sg, q))
    for i, v in enumerate(vec):
        model = pyec.bign_verify(c, (v.qx, v.qy), h[32 * i:32 * i + 32], sg[48 * i:48 * i + 48])
        assert exp[i] == got_o[i] == got_h[i] == int(model), (v.family, v.label)
    mvec = sv.bign_msg_vectors("bign256")
    check_families("bign_msg", "bign256", mvec)
    for ln, part in sv.by_len(mvec).items():
        q, m, sg, exp = sv.pack_bign_msg(part)
        got_o, got_h = bytes(oracle.bign_verify_msg(q, m, ln, sg)), bytes(hc.bign_verify_msg(q, m, ln, sg))
        for i, v in enumerate(part):
            model = pyec.bign_verify(c, (v.qx, v.qy), pyec.belt_hash(v.msg), sg[48 * i:48 * i + 48])
            assert exp[i] == got_o[i] == got_h[i] == int(model), (ln, v.family, v.label)
        assert any(exp) and not all(exp)
