"""-m gpu: the uniform-schedule entry points on projective (X : Y : Z) records — ecgpu_batch_mul_ct_xyz[_dev] and
ecgpu_lincomb_ct_xyz[_dev].  The defining rule: for every input, the output bytes and the return code are those of `to_affine`
applied to every record (the oracle's ecref_batch_normalize) followed by the affine twin (ecgpu_batch_mul_ct /
ecgpu_lincomb_ct).  Every point is rescaled by a random z of its own (X = x z, Y = y z, Z = z)."""
import random

import numpy as np
import pytest

import oracle_lib
import pyec
from gpu_common import ALL_CURVES, CURVES, ecgpu_module, load_golden, msm_exceptional_terms, rand_scalars

pytestmark = pytest.mark.gpu
ERR_SCALAR_RANGE, ERR_POINT = -2, -3


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def enc_xyz(c, X, Y, Z):
    return X.to_bytes(c.L, c.order) + Y.to_bytes(c.L, c.order) + Z.to_bytes(c.L, c.order)


def rescale(c, P, z):
    if P is None:
        return enc_xyz(c, 0, z % c.p, 0)
    return enc_xyz(c, P[0] * z % c.p, P[1] * z % c.p, z)


def rescale_wire(c, xy, inf, rng, same_z=None):
    """affine wire records -> X || Y || Z, each under its own random z (or under same_z)"""
    out = []
    for i in range(len(inf)):
        z = same_z if same_z is not None else rng.randrange(1, c.p)
        P = pyec.dec_point(c, bytes(xy[i * 2 * c.L:(i + 1) * 2 * c.L]), int(inf[i]))
        out.append(rescale(c, P, z))
    return b"".join(out)


def to_affine(c, xyz):
    return oracle_lib.batch_normalize(c.cid, np.frombuffer(xyz, np.uint8))


def inputs(eng, c, n, seed):
    """n scalars and n records: points from the generator under random z, z G and z (-G), Z = 0 records with arbitrary
    X, Y < p, the exceptional terms of the MSM tests, and a stretch where every record has the same z"""
    rng = random.Random(seed)
    pts, pinf = eng.mul_by_generator(c.cid, rand_scalars(c.cid, n, seed))
    recs = [rescale_wire(c, pts, pinf, rng)]
    G = pyec.G(c)
    extra = [G, pyec.neg(c, G), G, pyec.neg(c, G)]
    recs += [rescale(c, P, rng.randrange(1, c.p)) for P in extra]
    recs += [enc_xyz(c, rng.randrange(c.p), rng.randrange(c.p), 0), enc_xyz(c, 0, 1, 0), enc_xyz(c, 0, 0, 0)]
    eks, eps = msm_exceptional_terms(c, rng, filler=4)
    recs += [rescale(c, P, rng.randrange(1, c.p)) for P in eps]
    z = rng.randrange(1, c.p)
    recs += [rescale_wire(c, pts[:24 * 2 * c.L], pinf[:24], rng, same_z=z)]
    xyz = b"".join(recs)
    m = len(xyz) // (3 * c.L)
    ks = [int.from_bytes(bytes(k), c.order) for k in rand_scalars(c.cid, m, seed + 1).reshape(m, c.L)]
    ks[n:n + len(extra)] = [1, 1, c.n - 1, 0]
    ks[n + len(extra) + 3:n + len(extra) + 3 + len(eks)] = eks
    scal = np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in ks), np.uint8).copy()
    return scal, xyz


@pytest.mark.parametrize("curve", ALL_CURVES + ["bign256"])
def test_mul_ct_xyz_equals_to_affine_then_mul_ct(eng, curve):
    c = pyec.CURVES[curve]
    scal, xyz = inputs(eng, c, 200, 0x5C70 + c.cid)
    aff, ainf = to_affine(c, xyz)
    assert ainf.sum() >= 3
    want, winf = oracle_lib.batch_mul(c.cid, scal, aff, ainf)
    got, ginf = eng.mul_xyz(c.cid, scal, xyz, constant_time=True)
    assert bytes(got) == bytes(want) and bytes(ginf) == bytes(winf)
    twin, tinf = eng.mul(c.cid, scal, aff, ainf, constant_time=True)
    assert bytes(got) == bytes(twin) and bytes(ginf) == bytes(tinf)


@pytest.mark.parametrize("curve", ALL_CURVES + ["bign256"])
def test_lincomb_ct_xyz_equals_to_affine_then_lincomb_ct(eng, curve):
    c = pyec.CURVES[curve]
    scal, xyz = inputs(eng, c, 120, 0x11C0 + c.cid)
    aff, ainf = to_affine(c, xyz)
    want, winf = oracle_lib.msm(c.cid, scal, aff, ainf, vartime=False)
    got, ginf = eng.lincomb_ct_xyz(c.cid, scal, xyz)
    assert bytes(got) == bytes(want) and ginf == winf
    twin, tinf = eng.lincomb_ct(c.cid, scal, aff, ainf)
    assert bytes(got) == bytes(twin) and ginf == tinf
    # a cancelling sum: k P + k (-P) under two different z is the identity
    L = c.L
    P = pyec.mul(c, 0x1234567, pyec.G(c))
    rng = random.Random(c.cid)
    xyz2 = rescale(c, P, rng.randrange(1, c.p)) + rescale(c, pyec.neg(c, P), rng.randrange(1, c.p))
    k = pyec.enc_scalar(c, 0xABCDEF)
    got, ginf = eng.lincomb_ct_xyz(c.cid, k + k, xyz2)
    assert ginf == 1 and bytes(got) == bytes(2 * L)
    got, ginf = eng.lincomb_ct_xyz(c.cid, b"", b"")                   # the empty sum
    assert ginf == 1 and bytes(got) == bytes(2 * L)


@pytest.mark.parametrize("curve", CURVES)
def test_golden_group_vectors_through_xyz(eng, curve):
    """The reference's group vectors ({k256,p256,p384,...}/src/test_vectors/group.rs): k G with G given as (x z : y z : z)."""
    c = pyec.CURVES[curve]
    g = load_golden(curve)["group"]
    ks = [pyec.enc_scalar(c, v["k"]) for v in g["add"]] + [bytes.fromhex(v["k"]) for v in g["mul"]]
    want = b"".join(bytes.fromhex(v["x"]) + bytes.fromhex(v["y"]) for v in g["add"] + g["mul"])
    rng = random.Random(0x601D + c.cid)
    xyz = b"".join(rescale(c, pyec.G(c), rng.randrange(1, c.p)) for _ in ks)
    out, inf = eng.mul_xyz(c.cid, b"".join(ks), xyz, constant_time=True)
    assert bytes(out) == want and not inf.any()
    for i in (0, 1, len(ks) - 1):
        o, f = eng.lincomb_ct_xyz(c.cid, ks[i], xyz[i * 3 * c.L:(i + 1) * 3 * c.L])
        assert bytes(o) == want[2 * c.L * i: 2 * c.L * (i + 1)] and f == 0


def bad_records(c, rng):
    P = pyec.mul(c, rng.randrange(1, c.n), pyec.G(c))
    z = rng.randrange(1, c.p)
    X, Y, Z = P[0] * z % c.p, P[1] * z % c.p, z
    return [enc_xyz(c, X, (Y + 1) % c.p, Z), enc_xyz(c, c.p, Y, Z), enc_xyz(c, X, c.p, Z), enc_xyz(c, X, Y, c.p),
            enc_xyz(c, c.p + 1, 0, 0)]


@pytest.mark.parametrize("curve", ["k256", "p256", "p384", "p521", "bign256"])
def test_xyz_input_errors(eng, curve):
    """Off-curve records with Z != 0 and coordinates >= p fail with ECGPU_ERR_POINT, a scalar >= n with ECGPU_ERR_SCALAR_RANGE,
    through the host-pointer and the device-pointer forms."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES[curve]
    rng = random.Random(0xE770 + c.cid)
    n = 64
    scal, xyz = inputs(eng, c, n, 0xE771 + c.cid)
    scal, xyz = scal[:n * c.L], xyz[:n * 3 * c.L]
    for bad in bad_records(c, rng):
        j = rng.randrange(n)
        rec = xyz[:j * 3 * c.L] + bad + xyz[(j + 1) * 3 * c.L:]
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.mul_xyz(c.cid, scal, rec, constant_time=True)
        assert e.value.code == ERR_POINT
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.lincomb_ct_xyz(c.cid, scal, rec)
        assert e.value.code == ERR_POINT
    ks = scal.copy()
    ks[3 * c.L:4 * c.L] = np.frombuffer(c.n.to_bytes(c.L, c.order), np.uint8)
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.mul_xyz(c.cid, ks, xyz, constant_time=True)
    assert e.value.code == ERR_SCALAR_RANGE
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.lincomb_ct_xyz(c.cid, ks, xyz)
    assert e.value.code == ERR_SCALAR_RANGE
    # the device forms
    d_k, d_p = eng.to_device(scal), eng.to_device(xyz[:(n - 1) * 3 * c.L] + bad_records(c, rng)[0])
    d_o, d_f = eng.dev_alloc(n * 2 * c.L + 16), eng.dev_alloc(n + 16)
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.mul_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f, constant_time=True)
    assert e.value.code == ERR_POINT
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.lincomb_ct_xyz_dev(c.cid, d_k, d_p, n, d_o, d_f)
    assert e.value.code == ERR_POINT


def test_xyz_dev_forms_and_deferred_errors(eng):
    """The _dev forms give the host forms' bytes; on an asynchronous context an input error surfaces at ecgpu_synchronize."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES["p256"]
    L, n = c.L, 300
    pad = lambda x: (x + 15) // 16 * 16
    scal, xyz = inputs(eng, c, n, 0xDE70)
    m = len(scal) // L
    want, winf = eng.mul_xyz(c.cid, scal, xyz, constant_time=True)
    wsum, wsinf = eng.lincomb_ct_xyz(c.cid, scal, xyz)
    d_k, d_p = eng.to_device(scal), eng.to_device(np.frombuffer(xyz, np.uint8))
    d_o, d_f = eng.dev_alloc(pad(m * 2 * L)), eng.dev_alloc(pad(m))
    d_s, d_sf = eng.dev_alloc(pad(2 * L)), eng.dev_alloc(16)
    eng.mul_xyz_dev(c.cid, d_k, d_p, m, d_o, d_f, constant_time=True)
    eng.lincomb_ct_xyz_dev(c.cid, d_k, d_p, m, d_s, d_sf)
    assert bytes(eng.to_host(d_o, m * 2 * L)) == bytes(want) and bytes(eng.to_host(d_f, m)) == bytes(winf)
    assert bytes(eng.to_host(d_s, 2 * L)) == bytes(wsum) and int(eng.to_host(d_sf, 1)[0]) == wsinf
    rng = random.Random(0xDE71)
    d_bad = eng.to_device(np.frombuffer(bad_records(c, rng)[0] + xyz[3 * L:], np.uint8))
    eng.set_async(True)
    try:
        eng.mul_xyz_dev(c.cid, d_k, d_p, m, d_o, d_f, constant_time=True)
        eng.mul_xyz_dev(c.cid, d_k, d_bad, m, d_o, d_f, constant_time=True)            # queued: returns
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.synchronize()
        assert e.value.code == ERR_POINT
        eng.synchronize()                                             # reported once
        eng.lincomb_ct_xyz_dev(c.cid, d_k, d_bad, m, d_s, d_sf)
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.synchronize()
        assert e.value.code == ERR_POINT
    finally:
        eng.set_async(False)


def test_mul_ct_xyz_host_pipeline(eng):
    """From 2^19 points the host-pointer call runs the chunk pipeline with 3L-byte records: the result equals the affine twin on
    the same points, and the oracle on a sample."""
    c = pyec.CURVES["k256"]
    L, n = c.L, (1 << 19) + 777
    scal = rand_scalars(c.cid, n, 0x91BE)
    pts, pinf = eng.mul_by_generator(c.cid, rand_scalars(c.cid, n, 0x91BF))
    # one z per 4,096 points (Python big integers at this size): every chunk of the pipeline sees many distinct z
    P = np.asarray(pts).reshape(n, 2, L)
    xs = [int.from_bytes(bytes(r), "big") for r in P[:, 0]]
    ys = [int.from_bytes(bytes(r), "big") for r in P[:, 1]]
    rng = random.Random(0x91C0)
    zs = [rng.randrange(1, c.p) for _ in range((n + 4095) // 4096)]
    xyz = b"".join(enc_xyz(c, x * zs[i >> 12] % c.p, y * zs[i >> 12] % c.p, zs[i >> 12]) for i, (x, y) in enumerate(zip(xs, ys)))
    got, ginf = eng.mul_xyz(c.cid, scal, xyz, constant_time=True)
    twin, tinf = eng.mul(c.cid, scal, pts, pinf, constant_time=True)
    assert bytes(got) == bytes(twin) and bytes(ginf) == bytes(tinf)
    for lo in (0, (1 << 18) - 5, n - 300):
        want, winf = oracle_lib.batch_mul(c.cid, scal[lo * L:(lo + 300) * L], pts[lo * 2 * L:(lo + 300) * 2 * L])
        assert bytes(got[lo * 2 * L:(lo + 300) * 2 * L]) == bytes(want)
