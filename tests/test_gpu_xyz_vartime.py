"""-m gpu: the variable-time entry points on projective (X : Y : Z) records — ecgpu_batch_mul_xyz, ecgpu_msm_xyz,
ecgpu_batch_mul_base_and_mul_add_xyz (with their _dev forms), ecgpu_msm_parts_xyz_dev and ecgpu_group_msm_xyz[_dev].  The
defining rule: for every input, the output bytes and the return code are those of `to_affine` applied to every record (the
oracle's ecref_batch_normalize) followed by the affine twin.  Checked against the oracle, not only against the twin.  Records of
large batches come from the compiled generator of tests/hostcheck_xyz_var (a random z under every record)."""
import ctypes
import random

import numpy as np
import pytest

import oracle_lib
import pyec
from gpu_common import ALL_CURVES, CURVES, dot_mod, ecgpu_module, fast_scalars, load_golden, rand_scalars
from test_gpu_msm_plans import _plan
from test_gpu_xyz_ct import bad_records, enc_xyz, inputs, rescale, to_affine
from test_xyz_vartime import build_helper

pytestmark = pytest.mark.gpu
ERR_SCALAR_RANGE, ERR_POINT = -2, -3
_u8p = ctypes.POINTER(ctypes.c_uint8)
pad = lambda x: (x + 15) // 16 * 16


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


@pytest.fixture(scope="module")
def hx():
    return build_helper()


def gen_xyz(hx, c, xy, inf, seed, shared=False):
    """X || Y || Z records of the affine points xy / inf, each under a random z in [2, p) (one z for all when shared)"""
    n = len(xy) // (2 * c.L)
    a = np.ascontiguousarray(xy, np.uint8)
    f = np.ascontiguousarray(inf if inf is not None else np.zeros(n, np.uint8), np.uint8)
    out = np.empty(n * 3 * c.L, np.uint8)
    assert hx.hx_rescale(c.cid, a.ctypes.data_as(_u8p), f.ctypes.data_as(_u8p), ctypes.c_size_t(n), ctypes.c_uint64(seed),
                         1 if shared else 0, out.ctypes.data_as(_u8p)) == 0
    return out


# ---- the defining rule, every entry point, every parameter set ----------------------------------------------------------

@pytest.mark.parametrize("curve", ALL_CURVES + ["bign256"])
def test_mul_vartime_xyz_equals_to_affine_then_mul(eng, curve):
    c = pyec.CURVES[curve]
    scal, xyz = inputs(eng, c, 200, 0x7A50 + c.cid)
    aff, ainf = to_affine(c, xyz)
    assert ainf.sum() >= 3
    want, winf = oracle_lib.batch_mul(c.cid, scal, aff, ainf, vartime=True)
    got, ginf = eng.mul_vartime_xyz(c.cid, scal, xyz)
    assert bytes(got) == bytes(want) and bytes(ginf) == bytes(winf)
    twin, tinf = eng.mul(c.cid, scal, aff, ainf)
    assert bytes(got) == bytes(twin) and bytes(ginf) == bytes(tinf)
    m = len(ginf)
    d_k, d_p = eng.to_device(scal), eng.to_device(np.frombuffer(xyz, np.uint8))
    d_o, d_f = eng.dev_alloc(pad(m * 2 * c.L)), eng.dev_alloc(pad(m))
    eng.mul_vartime_xyz_dev(c.cid, d_k, d_p, m, d_o, d_f)
    assert bytes(eng.to_host(d_o, m * 2 * c.L)) == bytes(want) and bytes(eng.to_host(d_f, m)) == bytes(winf)


@pytest.mark.parametrize("curve", ALL_CURVES + ["bign256"])
def test_lincomb_xyz_equals_to_affine_then_lincomb(eng, curve):
    c = pyec.CURVES[curve]
    scal, xyz = inputs(eng, c, 150, 0x11C5 + c.cid)
    aff, ainf = to_affine(c, xyz)
    want, winf = oracle_lib.msm(c.cid, scal, aff, ainf, vartime=True)
    got, ginf = eng.lincomb_xyz(c.cid, scal, xyz)
    assert bytes(got) == bytes(want) and ginf == winf
    twin, tinf = eng.lincomb(c.cid, scal, aff, ainf)
    assert bytes(got) == bytes(twin) and ginf == tinf
    m = len(scal) // c.L
    d_k, d_p = eng.to_device(scal), eng.to_device(np.frombuffer(xyz, np.uint8))
    d_o, d_f = eng.dev_alloc(pad(2 * c.L)), eng.dev_alloc(16)
    eng.lincomb_xyz_dev(c.cid, d_k, d_p, m, d_o, d_f)
    assert bytes(eng.to_host(d_o, 2 * c.L)) == bytes(want) and int(eng.to_host(d_f, 1)[0]) == winf
    # the parts form: one local half, then the combining half, gives the same record
    plan = m
    d_parts = eng.dev_alloc(pad(eng.msm_parts_bytes(c.cid, plan)))
    eng.msm_parts_xyz_dev(c.cid, d_k, d_p, m, plan, d_parts)
    eng.msm_finish_dev(c.cid, d_parts, 1, plan, d_o, d_f)
    assert bytes(eng.to_host(d_o, 2 * c.L)) == bytes(want) and int(eng.to_host(d_f, 1)[0]) == winf
    # a cancelling sum, and the empty sum
    P = pyec.mul(c, 0x1234567, pyec.G(c))
    rng = random.Random(c.cid)
    xyz2 = rescale(c, P, rng.randrange(1, c.p)) + rescale(c, pyec.neg(c, P), rng.randrange(1, c.p))
    k = pyec.enc_scalar(c, 0xABCDEF)
    got, ginf = eng.lincomb_xyz(c.cid, k + k, xyz2)
    assert ginf == 1 and bytes(got) == bytes(2 * c.L)
    got, ginf = eng.lincomb_xyz(c.cid, b"", b"")
    assert ginf == 1 and bytes(got) == bytes(2 * c.L)


@pytest.mark.parametrize("curve", ALL_CURVES + ["bign256"])
def test_mul_add_xyz_equals_to_affine_then_mul_add(eng, curve):
    c = pyec.CURVES[curve]
    b, xyz = inputs(eng, c, 120, 0xADD0 + c.cid)
    m = len(b) // c.L
    a = rand_scalars(c.cid, m, 0xADD1 + c.cid)
    aff, ainf = to_affine(c, xyz)
    ag, agi = oracle_lib.batch_mul_base(c.cid, a)
    bp, bpi = oracle_lib.batch_mul(c.cid, b, aff, ainf, vartime=True)
    want = []
    for i in range(m):
        P = pyec.dec_point(c, bytes(ag[i * 2 * c.L:(i + 1) * 2 * c.L]), int(agi[i]))
        Q = pyec.dec_point(c, bytes(bp[i * 2 * c.L:(i + 1) * 2 * c.L]), int(bpi[i]))
        want.append(pyec.enc_point(c, pyec.add(c, P, Q)))
    wxy, winf = b"".join(w[0] for w in want), bytes(w[1] for w in want)
    got, ginf = eng.mul_by_generator_and_mul_add_xyz(c.cid, a, b, xyz)
    assert bytes(got) == wxy and bytes(ginf) == winf
    twin, tinf = eng.mul_by_generator_and_mul_add(c.cid, a, b, aff, ainf)
    assert bytes(got) == bytes(twin) and bytes(ginf) == bytes(tinf)
    d_a, d_b, d_p = eng.to_device(a), eng.to_device(b), eng.to_device(np.frombuffer(xyz, np.uint8))
    d_o, d_f = eng.dev_alloc(pad(m * 2 * c.L)), eng.dev_alloc(pad(m))
    eng.mul_by_generator_and_mul_add_xyz_dev(c.cid, d_a, d_b, d_p, m, d_o, d_f)
    assert bytes(eng.to_host(d_o, m * 2 * c.L)) == wxy and bytes(eng.to_host(d_f, m)) == winf


@pytest.mark.parametrize("curve", CURVES)
def test_golden_group_vectors_through_xyz_vartime(eng, curve):
    """The reference's group vectors: k G with G given as (x z : y z : z), by mul_vartime_xyz and as one-term lincombs."""
    c = pyec.CURVES[curve]
    g = load_golden(curve)["group"]
    ks = [pyec.enc_scalar(c, v["k"]) for v in g["add"]] + [bytes.fromhex(v["k"]) for v in g["mul"]]
    want = b"".join(bytes.fromhex(v["x"]) + bytes.fromhex(v["y"]) for v in g["add"] + g["mul"])
    rng = random.Random(0x601E + c.cid)
    xyz = b"".join(rescale(c, pyec.G(c), rng.randrange(1, c.p)) for _ in ks)
    out, inf = eng.mul_vartime_xyz(c.cid, b"".join(ks), xyz)
    assert bytes(out) == want and not inf.any()
    for i in (0, 1, len(ks) - 1):
        o, f = eng.lincomb_xyz(c.cid, ks[i], xyz[i * 3 * c.L:(i + 1) * 3 * c.L])
        assert bytes(o) == want[2 * c.L * i: 2 * c.L * (i + 1)] and f == 0


# ---- errors -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", ["k256", "p256", "p384", "p521", "p224", "bign256"])
def test_xyz_vartime_input_errors(eng, curve):
    """Each bad record fails every form with ECGPU_ERR_POINT, a scalar >= n with ECGPU_ERR_SCALAR_RANGE; below 2^19 units a
    failed host-pointer call writes nothing."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES[curve]
    L, n = c.L, 64
    rng = random.Random(0xE780 + c.cid)
    scal, xyz = inputs(eng, c, n, 0xE781 + c.cid)
    scal, xyz = scal[:n * L], xyz[:n * 3 * L]
    lib = eng._lib
    sentinel = lambda k: np.full(k, 0xA5, np.uint8)

    def host_calls(ks, recs):
        p = np.frombuffer(recs, np.uint8).copy()
        k = np.ascontiguousarray(ks, np.uint8)
        o1, f1, o2, f2, o3, f3 = sentinel(n * 2 * L), sentinel(n), sentinel(2 * L), sentinel(1), sentinel(n * 2 * L), sentinel(n)
        h = lambda a: a.ctypes.data_as(_u8p)
        rcs = [lib.ecgpu_batch_mul_xyz(eng._ctx, c.cid, h(k), h(p), ctypes.c_size_t(n), h(o1), h(f1)),
               lib.ecgpu_msm_xyz(eng._ctx, c.cid, h(k), h(p), ctypes.c_size_t(n), h(o2), h(f2)),
               lib.ecgpu_batch_mul_base_and_mul_add_xyz(eng._ctx, c.cid, h(k), h(k), h(p), ctypes.c_size_t(n), h(o3), h(f3))]
        for buf in (o1, f1, o2, f2, o3, f3):
            assert (buf == 0xA5).all()                                # nothing written
        return rcs

    d_k, d_o, d_f = eng.to_device(scal), eng.dev_alloc(pad(n * 2 * L)), eng.dev_alloc(pad(n))
    d_parts = eng.dev_alloc(pad(eng.msm_parts_bytes(c.cid, n)))
    for bad in bad_records(c, rng) + [enc_xyz(c, 0, c.p, 0)]:
        j = rng.randrange(n)
        rec = xyz[:j * 3 * L] + bad + xyz[(j + 1) * 3 * L:]
        assert host_calls(scal, rec) == [ERR_POINT] * 3, bad.hex()
        d_p = eng.to_device(np.frombuffer(rec, np.uint8))
        for call in (lambda: eng.mul_vartime_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f),
                     lambda: eng.lincomb_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f),
                     lambda: eng.mul_by_generator_and_mul_add_xyz_dev(c.cid, d_k, d_k, d_p, n, d_o, d_f),
                     lambda: eng.msm_parts_xyz_dev(c.cid, d_k, d_p, n, n, d_parts)):
            with pytest.raises(ecgpu.EcgpuError) as e:
                call()
            assert e.value.code == ERR_POINT
        d_p.free()
    ks = scal.copy()
    ks[3 * L:4 * L] = np.frombuffer(c.n.to_bytes(L, c.order), np.uint8)
    assert host_calls(ks, xyz) == [ERR_SCALAR_RANGE] * 3
    d_bk, d_p = eng.to_device(ks), eng.to_device(np.frombuffer(xyz, np.uint8))
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.lincomb_xyz_dev(c.cid, d_bk, d_p, n, d_o, d_f)
    assert e.value.code == ERR_SCALAR_RANGE
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.mul_vartime_xyz_dev(c.cid, d_bk, d_p, n, d_o, d_f)
    assert e.value.code == ERR_SCALAR_RANGE


def test_xyz_vartime_deferred_errors(eng):
    """On an asynchronous context an input error of any _xyz form surfaces at ecgpu_synchronize, once."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES["p256"]
    L = c.L
    scal, xyz = inputs(eng, c, 300, 0xDE80)
    m = len(scal) // L
    rng = random.Random(0xDE81)
    d_k, d_p = eng.to_device(scal), eng.to_device(np.frombuffer(xyz, np.uint8))
    d_bad = eng.to_device(np.frombuffer(bad_records(c, rng)[0] + xyz[3 * L:], np.uint8))
    d_o, d_f = eng.dev_alloc(pad(m * 2 * L)), eng.dev_alloc(pad(m))
    d_parts = eng.dev_alloc(pad(eng.msm_parts_bytes(c.cid, m)))
    eng.set_async(True)
    try:
        for call in (lambda p: eng.mul_vartime_xyz_dev(c.cid, d_k, p, m, d_o, d_f),
                     lambda p: eng.lincomb_xyz_dev(c.cid, d_k, p, m, d_o, d_f),
                     lambda p: eng.mul_by_generator_and_mul_add_xyz_dev(c.cid, d_k, d_k, p, m, d_o, d_f),
                     lambda p: eng.msm_parts_xyz_dev(c.cid, d_k, p, m, m, d_parts)):
            call(d_p)
            call(d_bad)                                               # queued: returns
            with pytest.raises(ecgpu.EcgpuError) as e:
                eng.synchronize()
            assert e.value.code == ERR_POINT
            eng.synchronize()                                         # reported once
    finally:
        eng.set_async(False)


# ---- the MSM planner's thresholds ---------------------------------------------------------------------------------------

MSM_GLV_MAX_TERMS = 13 << 17
# each planner threshold of tests/test_gpu_msm_plans.py up to 2^20 terms, with a size on either side
PLAN_SIZES = {"k256": [1 << 16, (1 << 16) + 1, (1 << 19) - 1, 1 << 19, MSM_GLV_MAX_TERMS - 1, MSM_GLV_MAX_TERMS],
              "p256": [1 << 16, (1 << 16) + 1, (1 << 17) - 64, 1 << 17, 1 << 20, MSM_GLV_MAX_TERMS - 1, MSM_GLV_MAX_TERMS],
              "p384": [1 << 10, (1 << 10) + 1],
              "p521": [(1 << 10) + 1]}


@pytest.mark.parametrize("curve,n", [(cv, n) for cv, v in PLAN_SIZES.items() for n in v])
def test_msm_xyz_at_plan_boundaries(eng, hx, curve, n):
    """Both sides of the planner's thresholds (small path, one- and two-level sort, the k256 GLV range, c = 16): the xyz MSM
    equals the affine MSM of the same points and the exact value (sum k_i s_i mod n) G."""
    c = pyec.CURVES[curve]
    L = c.L
    assert eng.msm_plan_window(c.cid, n) == _plan(curve, n)[0]
    s = fast_scalars(c, n, 0xB0 + n) if c.n >> (8 * L - 32) == 0xFFFFFFFF else \
        rand_scalars(c.cid, n, 0xB0 + n).reshape(n, L)
    k = fast_scalars(c, n, 0xB1 + n) if c.n >> (8 * L - 32) == 0xFFFFFFFF else \
        rand_scalars(c.cid, n, 0xB1 + n).reshape(n, L)
    pts, pinf = eng.mul_by_generator(c.cid, s.reshape(-1))
    xyz = gen_xyz(hx, c, pts, pinf, 0xB2 + n)
    d_k, d_p, d_a = eng.to_device(k.reshape(-1)), eng.to_device(xyz), eng.to_device(pts)
    d_o, d_f, d_t, d_tf = eng.dev_alloc(pad(2 * L)), eng.dev_alloc(16), eng.dev_alloc(pad(2 * L)), eng.dev_alloc(16)
    eng.lincomb_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f)
    eng.lincomb_dev(c.cid, d_k, d_a, None, n, d_t, d_tf)
    got = bytes(eng.to_host(d_o, 2 * L))
    assert got == bytes(eng.to_host(d_t, 2 * L)) and int(eng.to_host(d_f, 1)[0]) == int(eng.to_host(d_tf, 1)[0])
    e = dot_mod(k, s, c.n)
    want, winf = oracle_lib.batch_mul_base(c.cid, np.frombuffer(pyec.enc_scalar(c, e), np.uint8))
    assert got == bytes(want) and int(eng.to_host(d_f, 1)[0]) == int(winf[0])
    for buf in (d_k, d_p, d_a):
        buf.free()


def test_k256_msm_xyz_2_24(eng, hx):
    """k256 ecgpu_msm_xyz_dev at 2^24 terms, a random z != 1 under every record, against (sum k_i s_i mod n) G."""
    c = pyec.CURVES["k256"]
    L, n = c.L, 1 << 24
    s, k = fast_scalars(c, n, 0x2424), fast_scalars(c, n, 0x2425)
    d_s = eng.to_device(s.reshape(-1))
    d_pts = eng.dev_alloc(n * 2 * L)
    eng.mul_by_generator_dev(c.cid, d_s, n, d_pts, None)
    pts = eng.to_host(d_pts)
    d_pts.free()
    d_s.free()
    xyz = gen_xyz(hx, c, pts, None, 0x2426)
    del pts
    d_k, d_p = eng.to_device(k.reshape(-1)), eng.to_device(xyz)
    d_o, d_f = eng.dev_alloc(pad(2 * L)), eng.dev_alloc(16)
    eng.lincomb_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f)
    want, _ = oracle_lib.batch_mul_base(c.cid, np.frombuffer(pyec.enc_scalar(c, dot_mod(k, s, c.n)), np.uint8))
    assert bytes(eng.to_host(d_o, 2 * L)) == bytes(want) and int(eng.to_host(d_f, 1)[0]) == 0
    d_k.free()
    d_p.free()


def test_host_pipelines_give_the_dev_bytes(eng, hx):
    """ecgpu_msm_xyz at 2^23 + 1 terms (partial MSMs over chunks of 2^22) and ecgpu_batch_mul_xyz at 2^19 + 1 records (chunk
    pipeline) give the bytes of their _dev forms."""
    c = pyec.CURVES["p256"]
    L = c.L
    n = (1 << 23) + 1
    s, k = fast_scalars(c, n, 0x9A), fast_scalars(c, n, 0x9B)
    pts, pinf = eng.mul_by_generator(c.cid, s.reshape(-1))
    xyz = gen_xyz(hx, c, pts, pinf, 0x9C)
    got, ginf = eng.lincomb_xyz(c.cid, k.reshape(-1), xyz)
    d_k, d_p = eng.to_device(k.reshape(-1)), eng.to_device(xyz)
    d_o, d_f = eng.dev_alloc(pad(2 * L)), eng.dev_alloc(16)
    eng.lincomb_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f)
    assert bytes(got) == bytes(eng.to_host(d_o, 2 * L)) and ginf == int(eng.to_host(d_f, 1)[0])
    m = (1 << 19) + 1
    got, ginf = eng.mul_vartime_xyz(c.cid, k[:m].reshape(-1), xyz[:m * 3 * L])
    d_o2, d_f2 = eng.dev_alloc(pad(m * 2 * L)), eng.dev_alloc(pad(m))
    eng.mul_vartime_xyz_dev(c.cid, d_k, d_p, m, d_o2, d_f2)
    assert bytes(got) == bytes(eng.to_host(d_o2, m * 2 * L)) and bytes(ginf) == bytes(eng.to_host(d_f2, m))
    want, winf = oracle_lib.batch_mul(c.cid, k[:300].reshape(-1), pts[:300 * 2 * L], pinf[:300], vartime=True)
    assert bytes(got[:300 * 2 * L]) == bytes(want)
    for buf in (d_k, d_p, d_o2, d_f2):
        buf.free()


# ---- lanes, groups, scratch sharing -------------------------------------------------------------------------------------

def test_lanes_back_to_back_and_parts(hx):
    """Asynchronous context, two MSM lanes: back-to-back ecgpu_msm_xyz_dev calls on different inputs (each converted on its lane)
    give their stand-alone results; msm_parts_xyz_dev -> join -> msm_finish_dev equals ecgpu_msm_xyz."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES["k256"]
    L, n = c.L, (1 << 18) + 3
    e = ecgpu.Engine(0)
    try:
        sets = []
        for i in range(3):
            s, k = fast_scalars(c, n, 0x1A0 + i), fast_scalars(c, n, 0x1B0 + i)
            pts, pinf = e.mul_by_generator(c.cid, s.reshape(-1))
            xyz = gen_xyz(hx, c, pts, pinf, 0x1C0 + i)
            sets.append((k.reshape(-1), xyz, e.lincomb_xyz(c.cid, k.reshape(-1), xyz)))
        dev = [(e.to_device(k), e.to_device(x)) for k, x, _ in sets]
        outs = [(e.dev_alloc(pad(2 * L)), e.dev_alloc(16)) for _ in sets]
        pb = pad(e.msm_parts_bytes(c.cid, n))
        parts = [e.dev_alloc(pb) for _ in sets]
        fin = [(e.dev_alloc(pad(2 * L)), e.dev_alloc(16)) for _ in sets]
        e.set_async(True)
        e.set_msm_lanes(2)
        try:
            for (d_k, d_p), (d_o, d_f) in zip(dev, outs):
                e.lincomb_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f)
            for i, ((d_k, d_p), d_parts) in enumerate(zip(dev, parts)):
                e.msm_parts_xyz_dev(c.cid, d_k, d_p, n, n, d_parts)
                if i:
                    e.msm_parts_join_dev(parts[i - 1])
                    e.msm_finish_dev(c.cid, parts[i - 1], 1, n, fin[i - 1][0], fin[i - 1][1])
            e.msm_parts_join_dev(parts[-1])
            e.msm_finish_dev(c.cid, parts[-1], 1, n, fin[-1][0], fin[-1][1])
            e.synchronize()
        finally:
            e.set_msm_lanes(1)
            e.set_async(False)
        for (_, _, (w, wi)), (d_o, d_f), (d_fo, d_ff) in zip(sets, outs, fin):
            assert bytes(e.to_host(d_o, 2 * L)) == bytes(w) and int(e.to_host(d_f, 1)[0]) == wi
            assert bytes(e.to_host(d_fo, 2 * L)) == bytes(w) and int(e.to_host(d_ff, 1)[0]) == wi
    finally:
        e.close()


def test_group_msm_xyz_equals_msm_xyz(eng, hx):
    """A group with device 0 listed twice: ecgpu_group_msm_xyz[_dev] equals ecgpu_msm_xyz."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES["p256"]
    L, n = c.L, 100003
    s = fast_scalars(c, n, 0x6A)
    k = fast_scalars(c, n, 0x6B).reshape(-1)
    pts, pinf = eng.mul_by_generator(c.cid, s.reshape(-1))
    xyz = gen_xyz(hx, c, pts, pinf, 0x6C)
    want = eng.lincomb_xyz(c.cid, k, xyz)
    grp = ecgpu.Group([0, 0], exchange="peer")
    try:
        got = grp.lincomb_xyz(c.cid, k, xyz)
        assert bytes(got[0]) == bytes(want[0]) and got[1] == want[1]
        h = n // 2
        d_k = [eng.to_device(k[:h * L]), eng.to_device(k[h * L:])]
        d_p = [eng.to_device(xyz[:h * 3 * L]), eng.to_device(xyz[h * 3 * L:])]
        got = grp.lincomb_xyz_dev(c.cid, d_k, d_p, [h, n - h])
        assert bytes(got[0]) == bytes(want[0]) and got[1] == want[1]
    finally:
        grp.close()


def test_affine_compressed_and_xyz_msms_share_scratch(eng, hx):
    """Interleaved on one context, the affine, compressed and xyz MSMs each give their stand-alone bytes."""
    c = pyec.CURVES["k256"]
    L = c.L
    runs = []
    for i, n in enumerate((5000, (1 << 17) + 9, 777)):
        s, k = fast_scalars(c, n, 0x5A0 + i), fast_scalars(c, n, 0x5B0 + i).reshape(-1)
        pts, pinf = eng.mul_by_generator(c.cid, s.reshape(-1))
        x, tag = eng.mul_by_generator_compressed(c.cid, s.reshape(-1))
        xyz = gen_xyz(hx, c, pts, pinf, 0x5C0 + i)
        want = oracle_lib.batch_mul_base(c.cid, np.frombuffer(pyec.enc_scalar(c, dot_mod(k.reshape(n, L), s, c.n)), np.uint8))
        runs.append((k, pts, x, tag, xyz, bytes(want[0])))
    for _ in range(2):
        for k, pts, x, tag, xyz, want in runs + runs[::-1]:
            assert bytes(eng.lincomb_xyz(c.cid, k, xyz)[0]) == want
            assert bytes(eng.lincomb(c.cid, k, pts)[0]) == want
            assert bytes(eng.lincomb_compressed(c.cid, k, x, tag)[0]) == want
