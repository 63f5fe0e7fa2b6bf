"""-m gpu: the vectors of tests/sign_vectors.py ("s chosen first") on gfx950.

Per set, the same batches go through ecgpu_ecdsa_sign_batch forwards and through ecgpu_ecdsa_sign_batch_dev reversed (SM2DSA:
ecgpu_sm2dsa_sign_batch both ways; it has no _dev form), and every record is compared byte for byte with what the construction says
and with the g++ twin; every ok = 1 record goes back through the device verifier under reject_high_s = normalize_s and through key
recovery, which must return d G.  The stages no pipeline input produces (x(R) in [n, p), x(R) = n, r_inf = 1, a cleared flag, a
Schnorr nonce that cancels e d') reach the product's finish kernels through ecgpu_selftest_sign_finish.  BIP340 signing gets the
message lengths around the padding boundaries of Bip340::tagged, which pads on its own."""
import random

import numpy as np
import pytest

import oracle_lib
import pyec
import sign_model as sm
import sign_vectors as sv
import sm2sign_model
import test_hostcheck_sign as ths
import test_hostcheck_sm2sign as ths2
import test_sign_vectors as tsv
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
ERR_CURVE, ERR_ARG = -1, -7


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def enc(c, values):
    return np.frombuffer(b"".join(int(v).to_bytes(c.L, "big") for v in values), np.uint8).copy()


def records(c, sig, recid, ok):
    sig = bytes(sig)
    return [(sig[2 * c.L * i:2 * c.L * (i + 1)], int(recid[i]), int(ok[i])) for i in range(len(ok))]


def sign_host(eng, c, vec, normalize_s):
    return records(c, *eng.ecdsa_sign(c.cid, enc(c, [v.d for v in vec]), enc(c, [v.k for v in vec]), enc(c, [v.z for v in vec]), normalize_s=normalize_s))


def sign_dev_reversed(eng, c, vec, normalize_s):
    """the device-pointer form on the batch in reverse order -> the records in the vectors' order"""
    n, L = len(vec), c.L
    rev = vec[::-1]
    d_d, d_k, d_z = (eng.to_device(enc(c, [getattr(v, f) for v in rev])) for f in ("d", "k", "z"))
    sig, rid, ok = eng.dev_alloc(n * 2 * L + 16), eng.dev_alloc(n + 16), eng.dev_alloc(n + 16)
    eng.ecdsa_sign_dev(c.cid, d_d, d_k, d_z, n, normalize_s, sig, rid, ok)
    return records(c, eng.to_host(sig, n * 2 * L), eng.to_host(rid, n), eng.to_host(ok, n))[::-1]


def round_trip(eng, c, vec, got, normalize_s, what):
    """every ok record verifies on the device under reject_high_s = normalize_s, and its recovery id leads back to d G"""
    n, L = len(vec), c.L
    q, qinf = eng.mul_by_generator(c.cid, enc(c, [v.d if 1 <= v.d < c.n else 1 for v in vec]))
    assert not qinf.any()
    r, s = (np.frombuffer(b"".join(g[0][i * L:(i + 1) * L] for g in got), np.uint8).copy() for i in (0, 1))
    z = enc(c, [v.z for v in vec])
    ok = [g[2] for g in got]
    ver = eng.ecdsa_verify(c.cid, z, r, s, q, reject_high_s=bool(normalize_s))
    bad = sv.first_mismatch(c.name, what + ": device verifier", vec, [int(x) for x in ver], ok)
    assert bad is None, bad
    keys, rok = eng.ecdsa_recover(c.cid, z, r, s, np.array([g[1] for g in got], np.uint8), reject_high_s=bool(normalize_s))
    bad = sv.first_mismatch(c.name, what + ": device recovery verdict", vec, [int(x) for x in rok], ok)
    assert bad is None, bad
    keys, q = bytes(keys), bytes(q)
    rec = [keys[2 * L * i:2 * L * (i + 1)] if ok[i] else b"" for i in range(n)]
    bad = sv.first_mismatch(c.name, what + ": recovered key", vec, rec, [q[2 * L * i:2 * L * (i + 1)] if ok[i] else b"" for i in range(n)])
    assert bad is None, bad


# ---- ECDSA ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_families(eng, name):
    c = pyec.CURVES[name]
    vec, _, _ = sv.ecdsa_vectors(name, oracle_lib)
    for normalize_s in (0, 1):
        want = sv.ecdsa_expected(name, vec, normalize_s, oracle_lib)
        twin = tsv.twin_ecdsa_vectors(ths.lib(), name, vec, normalize_s, oracle_lib)
        fwd = sign_host(eng, c, vec, normalize_s)
        rev = sign_dev_reversed(eng, c, vec, normalize_s)
        for what, got, ref in (("host form against the construction", fwd, want), ("_dev form reversed against the construction", rev, want),
                               ("host form against the twin", fwd, twin)):
            bad = sv.first_mismatch(name, "%s, normalize_s = %d" % (what, normalize_s), vec, got, ref)
            assert bad is None, bad
        round_trip(eng, c, vec, fwd, normalize_s, "normalize_s = %d" % normalize_s)


@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_positions(eng, name):
    c = pyec.CURVES[name]
    good, fails, layouts = sv.position_batches(name)
    zero = (bytes(2 * c.L), 0, 0)
    for normalize_s in (0, 1):
        base = sign_host(eng, c, good, normalize_s)
        bad = sv.first_mismatch(name, "neighbours, normalize_s = %d" % normalize_s, good, base, sv.ecdsa_expected(name, good, normalize_s, oracle_lib))
        assert bad is None, bad
        for j, lay in enumerate(layouts):
            batch = sv.placed(good, fails, lay)
            got = sign_host(eng, c, batch, normalize_s) if (j + normalize_s) % 2 == 0 else sign_dev_reversed(eng, c, batch, normalize_s)
            want = list(base)
            for p, _ in lay:
                want[p] = zero
            bad = sv.first_mismatch(name, "positions %r, normalize_s = %d" % (lay, normalize_s), batch, got, want)
            assert bad is None, bad


@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_finish_kernel_on_forged_stages(eng, name):
    c = pyec.CURVES[name]
    vec, _ = sv.hook_ecdsa(name)
    d, k, z = (enc(c, [getattr(v, f) for v in vec]) for f in ("d", "k", "z"))
    flag, rinf = bytes(v.flag for v in vec), bytes(v.r_inf for v in vec)
    rxy = enc(c, [t for v in vec for t in (v.x, v.y)])
    for normalize_s in (0, 1):
        got = records(c, *eng.selftest_sign_finish(c.cid, 0, d, k, flag, z, rxy, rinf, normalize_s=normalize_s))
        twin = tsv.twin_ecdsa(ths.lib(), c, [v.d for v in vec], [v.k for v in vec], [v.flag for v in vec], [v.z for v in vec],
                              [(v.x, v.y) for v in vec], [v.r_inf for v in vec], normalize_s)
        for what, ref in (("construction", sv.hook_ecdsa_expected(name, vec, normalize_s)), ("twin", twin)):
            bad = sv.first_mismatch(name, "finish kernel against the %s, normalize_s = %d" % (what, normalize_s), vec, got, ref)
            assert bad is None, bad
        assert sum(g[1] >> 1 for g in got) == 2 * ((len(vec) - 3) // 4 - 1)                      # recid bit 1: x = n + 1 and x = p - 1, s != 0
    # the hook on honest stages is the pipeline: one element of the entry point, its R from the oracle
    v = next(v for v in vec if v.label == "honest stages")
    assert records(c, *eng.ecdsa_sign(c.cid, enc(c, [v.d]), enc(c, [v.k]), enc(c, [v.z]), normalize_s=1)) == \
        records(c, *eng.selftest_sign_finish(c.cid, 0, enc(c, [v.d]), enc(c, [v.k]), b"\x01", enc(c, [v.z]), enc(c, [v.x, v.y]), b"\x00", normalize_s=1))


def test_finish_hook_arguments(eng):
    mod = ecgpu_module()
    b32, b64, one = np.ones(32, np.uint8), np.ones(64, np.uint8), b"\x01"
    for curve, scheme in ((mod.SM2, 0), (mod.BIGN256, 0), (mod.K256, 1), (mod.P256, 2), (mod.SM2, 2), (99, 0)):
        with pytest.raises(mod.EcgpuError) as e:
            eng.selftest_sign_finish(curve, scheme, b64 if scheme == 2 else b32, b32, one, b32, b64, one)
        assert e.value.code == ERR_CURVE, (curve, scheme)
    for scheme in (-1, 3):
        with pytest.raises(mod.EcgpuError) as e:
            eng.selftest_sign_finish(mod.K256, scheme, b32, b32, one, b32, b64, one)
        assert e.value.code == ERR_ARG
    with pytest.raises(mod.EcgpuError) as e:
        eng.selftest_sign_finish(mod.K256, 0, b32, b32, one, None, b64, one)                    # ECDSA without z
    assert e.value.code == ERR_ARG
    sig, recid, ok = eng.selftest_sign_finish(mod.K256, 0, b"", b"", b"", b"", b"", b"")       # n = 0
    assert sig.size == 0 and ok.size == 0


# ---- SM2DSA ---------------------------------------------------------------------------------------------------------------------

def sm2_sign(eng, vec, reverse=False):
    e32 = lambda f: np.frombuffer(b"".join(int(getattr(v, f)).to_bytes(32, "big") for v in (vec[::-1] if reverse else vec)), np.uint8).copy()
    sig, ok = eng.sm2dsa_sign(e32("d"), e32("k"), e32("e"))
    sig = bytes(sig)
    out = [(sig[64 * i:64 * i + 64], int(ok[i])) for i in range(len(vec))]
    return out[::-1] if reverse else out


def test_sm2_families(eng):
    vec, _, _ = sv.sm2_vectors(oracle_lib)
    pts = sv.Points(pyec.SM2, oracle_lib)
    pts.prefetch([v.k for v in vec] + [v.d for v in vec])
    want = [sv.expect_sm2(v) for v in vec]
    twin = ths2.twin_finish([(v.d, v.k, 1, v.e, pts(v.k)[0], 0) for v in vec])
    fwd, rev = sm2_sign(eng, vec), sm2_sign(eng, vec, reverse=True)
    for what, got, ref in (("forwards against the construction", fwd, want), ("reversed against the construction", rev, want),
                           ("forwards against the twin", fwd, twin)):
        bad = sv.first_mismatch("sm2", what, vec, got, ref)
        assert bad is None, bad
    e32 = lambda vals: np.frombuffer(b"".join(int(x).to_bytes(32, "big") for x in vals), np.uint8).copy()
    ver = eng.sm2dsa_verify(e32(v.e % pyec.SM2.n for v in vec), e32(int.from_bytes(g[0][:32], "big") for g in fwd),
                            e32(int.from_bytes(g[0][32:], "big") for g in fwd), e32(t for v in vec for t in pts(v.d)))
    bad = sv.first_mismatch("sm2", "device verifier", vec, [int(x) for x in ver], [g[1] for g in fwd])
    assert bad is None, bad


def test_sm2_positions_and_forged_stages(eng):
    good, fails, layouts = sv.sm2_position_batches()
    base = sm2_sign(eng, good)
    bad = sv.first_mismatch("sm2", "neighbours", good, base, [sv.expect_sm2(v) for v in good])
    assert bad is None, bad
    for j, lay in enumerate(layouts):
        batch = sv.placed(good, fails, lay)
        want = list(base)
        for p, _ in lay:
            want[p] = sm2sign_model.ZERO
        bad = sv.first_mismatch("sm2", "positions %r" % (lay,), batch, sm2_sign(eng, batch, reverse=bool(j & 1)), want)
        assert bad is None, bad
    hook = sv.hook_sm2()
    rows = [r for _, r in hook]
    e32 = lambda j: b"".join(int(r[j]).to_bytes(32, "big") for r in rows)
    rxy = b"".join(int(r[4]).to_bytes(32, "big") + bytes(32) for r in rows)                     # the kernel reads x(R) alone
    sig, ok = eng.selftest_sign_finish(pyec.SM2.cid, 1, e32(0), e32(1), bytes(r[2] for r in rows), e32(3), rxy, bytes(r[5] for r in rows))
    sig = bytes(sig)
    got = [(sig[64 * i:64 * i + 64], int(ok[i])) for i in range(len(rows))]
    twin = ths2.twin_finish(rows)
    for (label, r), g, t in zip(hook, got, twin):
        assert g == sm2sign_model.finish(*r) == t, ("sm2", "H", label, g)


# ---- BIP340 ---------------------------------------------------------------------------------------------------------------------

def test_schnorr_finish_kernel_on_forged_stages(eng):
    c = pyec.K256
    for msg_len, vec in sorted(tsv.schnorr_by_length(sv.hook_schnorr()).items()):
        dp = enc(c, [t for v in vec for t in (v.d, v.px)])
        rxy = enc(c, [t for v in vec for t in (v.x, v.y)])
        sig, ok = eng.selftest_sign_finish(c.cid, 2, dp, enc(c, [v.k for v in vec]), bytes(v.flag for v in vec), None, rxy,
                                           bytes(v.r_inf for v in vec), msgs=b"".join(v.msg for v in vec) if msg_len else None, msg_len=msg_len)
        sig = bytes(sig)
        got = [(sig[64 * i:64 * i + 64], int(ok[i])) for i in range(len(vec))]
        for what, ref in (("construction", [sv.expect_schnorr(v) for v in vec]), ("twin", tsv.twin_schnorr(vec))):
            bad = sv.first_mismatch("k256", "schnorr finish kernel against the %s, msg_len = %d" % (what, msg_len), vec, got, ref)
            assert bad is None, bad


@pytest.mark.parametrize("msg_len", [1, 23, 24, 55, 56, 63, 64, 119, 120, 121])
def test_schnorr_sign_message_lengths(eng, msg_len):
    """Bip340::tagged pads on its own (it does not go through hash_pieces): behind the 64 bytes of t || x(P) or x(R) || x(P) the
    padding moves to a further block at msg_len = 56 and 120 (64 + msg_len + 9 > 128, 192)"""
    c = pyec.K256
    rng = random.Random(7000 + msg_len)
    n = 65
    rb = lambda m: rng.getrandbits(8 * m).to_bytes(m, "big")
    sks, auxs, msgs = [rng.randrange(1, c.n).to_bytes(32, "big") for _ in range(n)], [rb(32) for _ in range(n)], [rb(msg_len) for _ in range(n)]
    sig, ok = eng.schnorr_sign_raw(b"".join(sks), b"".join(msgs), msg_len, b"".join(auxs))
    sig = bytes(sig)
    for i in range(n):
        assert (sig[64 * i:64 * i + 64], int(ok[i])) == sm.schnorr_sign_raw(sks[i], msgs[i], auxs[i]), ("k256", "bip340", msg_len, i)
    pk, _ = eng.mul_by_generator(c.cid, b"".join(sks))
    pkx = np.asarray(pk).reshape(n, 64)[:, :32].copy().reshape(-1)
    assert all(int(v) == 1 for v in eng.schnorr_verify_raw(pkx, b"".join(msgs), msg_len, sig))
