"""The adversarial scalars of tests/scalar_vectors.py through the g++ twin of the device code (tests/hostcheck): the MSM digit
recoding window by window (hc_msm_digits: MsmSplit::split + MsmDigitStream, what k_msm_prepare runs), the Pippenger pipeline end to
end, the k256 GLV split and both ladders.  The models' own checks come first: a wrong model would aim every vector wrongly.
tests/test_gpu_scalar_vectors.py runs the same vectors on gfx950, where take()'s v_alignbit path exists."""
import ctypes
import random

import numpy as np
import pytest

import hostcheck_lib as hc
import pyec
import scalar_vectors as sv

SPLITS = [(name, False) for name in sv.CURVES] + [("k256", True)]
SPLIT_IDS = ["%s-%s" % (n, "glv" if g else "plain") for n, g in SPLITS]
E2E_SPLITS = [("k256", False), ("k256", True), ("p256", False), ("p192", False), ("p224", False), ("p384", False), ("p521", False)]
E2E_WIDTHS = (4, 7, 13, 15, 16)


def enc(c, ks):
    return b"".join(pyec.enc_scalar(c, k) for k in ks)


def be32(k):
    return k.to_bytes(32, "big")


# ---- the models ----------------------------------------------------------------------------------------------------------------

def test_sources_state_what_the_vectors_aim_at():
    sv._facts_checked = False
    sv.source_facts()
    assert sv._facts_checked


@pytest.mark.parametrize("name,glv", SPLITS, ids=SPLIT_IDS)
def test_model_digits_reconstruct_the_scalar(name, glv):
    """sum_w (+-weight(bucket_w)) 2^(c w) over the halves (the second times lambda) is k mod n, every bucket is below 2^(c-1),
    and the D set of every width holds the events it was built for."""
    c = pyec.CURVES[name]
    kbits, _ = sv.geometry(name, glv)
    for cbits in sv.WIDTHS:
        ks = sv.family_d(name, glv, cbits)
        sv.check_coverage_d(name, glv, cbits, ks)
        nwin = sv.window_count(kbits, cbits)
        for i, k in enumerate(ks):
            total = 0
            for h, (sub, flip) in enumerate(sv.subs(name, glv, k)):
                digs = sv.msm_digits(sub, kbits, cbits, 77 * i + 5, flip)
                assert len(digs) == nwin
                v = 0
                for w, (bucket, neg, nonzero) in enumerate(digs):
                    assert bucket < 1 << (cbits - 1) and (nonzero or (bucket, neg) == (0, 0))
                    if nonzero:
                        v += (-1 if neg else 1) * sv.bucket_weight(w, nwin, bucket, kbits, cbits) << (cbits * w)
                total += v * (sv.LAMBDA if h else 1)
            assert total % c.n == k, (name, glv, cbits, hex(k))


def test_model_split_is_the_oracles(oracle):
    """r1 + r2 lambda = k, both halves below 2^128, and the residues are the oracle's k256_glv_decompose on all of G."""
    n = sv.N_K256
    sv.check_coverage_g()
    for k in sv.g_all():
        r1, r2, c1, c2 = sv.glv_split(k)
        assert (r1 + r2 * sv.LAMBDA - k) % n == 0 and abs(r1) < 1 << 128 and abs(r2) < 1 << 128
        assert (c1, c2) == (r1 % n, r2 % n)
        assert oracle.k256_glv_decompose(be32(k)) == (be32(c1), be32(c2)), hex(k)


def test_model_radix16_is_the_oracles_and_the_twins(oracle):
    for name, nl in (("k256", 8), ("p384", 12)):
        c = pyec.CURVES[name]
        for k in sv.family_x(name)[::3] if name == "k256" else sv.family_x(name):
            want = sv.radix16(k, nl)
            assert list(oracle.radix16(pyec.enc_scalar(c, k), 8 * nl + 1)) == want
            assert list(hc.radix16(pyec.enc_scalar(c, k), nl)) == want
    for name in sv.CURVES:
        sv.check_coverage_x(name)


# ---- the twin, digit for digit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,glv", SPLITS, ids=SPLIT_IDS)
def test_twin_digits_equal_the_model(name, glv):
    """MsmSplit::split + MsmDigitStream on every D vector at every width: each vector as term i of its own set (second half:
    npad + i), and the vectors with a non-zero top digit again at the term indices around the sub-bucket mask."""
    c = pyec.CURVES[name]
    kbits, _ = sv.geometry(name, glv)
    for cbits in sv.WIDTHS:
        ks = sv.family_d(name, glv, cbits)
        npad = (len(ks) + 63) // 64 * 64
        got = hc.msm_digits(c.cid, glv, cbits, 0, npad, enc(c, ks))
        for i, k in enumerate(ks):
            msg = sv.first_digit_mismatch(name, glv, cbits, k, i, npad, got[i])
            assert msg is None, msg
        shift = sv.top_shift(kbits, cbits)
        tops = [k for k in ks if any(sv.signed_digits(sub, kbits, cbits)[-1] for sub, _ in sv.subs(name, glv, k))]
        if glv or kbits == sv.geometry(name, glv)[1]:
            assert len(tops) >= 20, (name, glv, cbits, len(tops))
        for base, pad in ((0, 64), ((1 << shift) - 1, 1 << 16), (1 << shift, 1 << 17), ((1 << 31) - len(tops) - 1, 1 << 30)):
            if not tops or (glv and pad + base + len(tops) >= 1 << 31):
                continue
            got = hc.msm_digits(c.cid, glv, cbits, base, pad, enc(c, tops))
            for i, k in enumerate(tops):
                msg = sv.first_digit_mismatch(name, glv, cbits, k, base + i, pad, got[i])
                assert msg is None, msg


def test_twin_digits_reject_what_they_do_not_know():
    c = pyec.CURVES["p256"]
    assert hc.lib().hc_msm_digits(1, 1, 5, 0, 64, None, 0, None) == -1           # GLV exists for k256 only
    assert hc.lib().hc_msm_digits(1, 0, 3, 0, 64, None, 0, None) == -1
    assert hc.lib().hc_msm_digits(1, 0, 17, 0, 64, None, 0, None) == -1
    bad = hc._a(pyec.enc_scalar(c, c.n))
    out = np.zeros(200, np.uint32)
    assert hc.lib().hc_msm_digits(1, 0, 5, 0, 64, hc._p(bad), ctypes.c_size_t(1), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -2


# ---- the twin, end to end ----------------------------------------------------------------------------------------------------------

_points = {}


def points_for(oracle, name, count):
    """(s_i, P_i = s_i G as wire bytes) for i < count, made once per parameter set."""
    c = pyec.CURVES[name]
    if name not in _points or len(_points[name][0]) < count:
        rng = random.Random(0x5EED + c.cid)
        s = [rng.randrange(1, c.n) for _ in range(max(count, 2600))]
        pts, inf = oracle.batch_mul_base(c.cid, enc(c, s))
        assert not inf.any()
        _points[name] = (s, bytes(pts))
    s, pts = _points[name]
    return s[:count], pts[: count * 2 * c.L]


@pytest.mark.parametrize("cbits", E2E_WIDTHS)
@pytest.mark.parametrize("name,glv", E2E_SPLITS, ids=["%s-%s" % (n, "glv" if g else "plain") for n, g in E2E_SPLITS])
def test_twin_pippenger_on_digit_strings(oracle, name, glv, cbits):
    """hc.msm (prepare / scan / scatter / accumulate / reduce / combine as on the device) over the D set with P_i = s_i G against
    (sum k_i s_i mod n) G by the oracle's fixed-base multiplication."""
    c = pyec.CURVES[name]
    ks = sv.family_d(name, glv, cbits)
    s, pts = points_for(oracle, name, len(ks))
    want, winf = oracle.batch_mul_base(c.cid, pyec.enc_scalar(c, sum(k * x for k, x in zip(ks, s)) % c.n))
    rc, out, inf = hc.msm(c.cid, cbits, enc(c, ks), pts, None, chunk=32, glv=glv)
    assert rc == 0
    assert (out, inf) == (bytes(want), int(winf[0])), (name, glv, cbits)


# ---- the twin, the split and the ladders ----------------------------------------------------------------------------------------------

def test_twin_split_equals_oracle_and_model(oracle):
    n = sv.N_K256
    for k in sv.g_all() + sv.family_x("k256"):
        r1, r2, c1, c2 = sv.glv_split(k)
        g1, g2, flags = hc.k256_glv(be32(k))
        if (g1, g2) != (be32(c1), be32(c2)) or flags != (1 if r1 < 0 else 0) | (2 if r2 < 0 else 0):
            raise AssertionError("k = %#x: the twin splits into %s, %s (flags %d), the model into %#x, %#x (signed %#x, %#x; "
                                 "rounded quotients %#x, %#x)" % ((k, g1.hex(), g2.hex(), flags, c1, c2, r1, r2) + sv.glv_quotients(k)))
        assert (g1, g2) == oracle.k256_glv_decompose(be32(k))


def ladder_scalars(name):
    """Family X, and for k256 the corners and the rounding boundary of G as well."""
    ks = list(sv.family_x(name))
    if name == "k256":
        g = sv.family_g()
        ks += g["corners"] + g["boundary"][::4] + g["boundary"][1::4]
    return ks


@pytest.mark.parametrize("name", sv.CURVES)
def test_twin_ladders_on_radix16_words(oracle, name):
    """var_base_mul (ecgpu_varmul.h) and var_base_mul_ct (ecgpu_ctmul.h) on family X against the oracle, on G and a random point."""
    c = pyec.CURVES[name]
    ks = ladder_scalars(name)
    scal = enc(c, ks)
    rng = random.Random(0x1ADD + c.cid)
    for P in (pyec.G(c), pyec.mul(c, rng.randrange(2, c.n), pyec.G(c))):
        pxy = pyec.enc_point(c, P)[0] * len(ks)
        want, winf = oracle.batch_mul(c.cid, scal, pxy, None)
        rc, out, inf = hc.batch_mul(c.cid, scal, pxy)
        assert rc == 0 and bytes(out) == bytes(want) and bytes(inf) == bytes(winf)
        rc, out, inf = hc.batch_mul_ct(c.cid, scal, pxy)
        assert rc == 0 and bytes(out) == bytes(want) and bytes(inf) == bytes(winf)
