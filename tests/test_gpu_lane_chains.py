"""-m gpu: degenerate records at every position of a lane's record chain (tests/lane_chains.py has the geometry and the classes).

Three launch geometries make one lane walk several records and carry state between them: the Montgomery-trick kernels
(k_normalize in its three output modes, k_xyz_affine, k_scalar_batch_inv: K = min(64, ceil(n / 65536)) records per lane), the
variable-base kernels above 524,288 lanes (k_var_base and its ADD form, k_var_base_ct, k_xyz_mul_ct: a lane does record i and then
i + 524288 on the same table slot), and — by cutting batches into 2^18-element device calls — the host-pointer pipeline, which
therefore never shows a device call K > 4 or a striding lane: only the _dev forms reach those.

Every batch here is a small table of m cases (m prime, no divisor of a lane count) tiled over n records by an index map, with
identities planted by position class: first, middle, last, adjacent, all, all-but-one of a chain, the last record of a ragged lane,
records n - 1, T - 1 and T.  The expectation is always small_result[idx_map], where small_result is the entry point's own output on
the m cases in one small call (K = 1, no stride), first compared byte for byte with the oracle; nothing is compared with the code
under test at the geometry under test.

  (a) forced K (ECGPU_NORM_K on the tool build) at small n, every parameter set, every entry point that ends in launch_normalize
  (b) the product library at its own thresholds: n = 65537 (K = 2), n = 131075 (K = 3), the compressed form, k_xyz_affine,
      k_scalar_batch_inv
  (c) striding variable-base lanes at n = 524288 + 300 (the normalisation behind them runs at K = 9)
  (d) the K = 64 cap at n = 64 * 65536 + 5
  (e) a bad record fails the call from any position, and the next clean call is unharmed
"""
import functools
import os

import numpy as np
import pytest

import lane_chains as lc
import oracle_lib
import pyec
from gpu_common import ALL_CURVES, ecdsa_cases, ecdsa_pack, ecgpu_module, rand_scalars, recover_cases, recover_pack

pytestmark = pytest.mark.gpu

EVERY_SET = ALL_CURVES + ["bign256"]
M = 61                                              # cases per table
SIGNATURE_M = (67, 47)                              # ECDSA verification / recovery case sets
FORCED_K = [(701, 3), (323, 64), (257, 2), (256, 1024)]
N_K2 = 65537                                        # K = 2, T = 32769: lane 32768 is ragged, with a single record
N_K3 = 131075                                       # K = 3, T = 43692: lane 43691 is ragged
N_STRIDE = 524288 + 300                             # variable-base lanes 0..299 own two records; normalisation at K = 9, T = 58288
N_CAP = 64 * 65536 + 5                              # K capped at 64 (uncapped: 65), T = 65537, lanes 0..65477 own 64 records, the rest 63
PAIR_LANES = (5, 63, 64, 255, 256, 290)             # the variable-base lanes of section (c)'s pairs (wave and workgroup edges among them)
BAD_POSITIONS = (524288 + 7, N_STRIDE - 1, 7 + 4 * 58288)    # section (e): second stride, record n - 1, the middle of a K = 9 chain
ORD, IDENT, KZERO = "ordinary", "identity point", "k = 0"
PAIRS = [(ORD, IDENT), (IDENT, ORD), (KZERO, ORD), (ORD, KZERO), (IDENT, IDENT), (KZERO, KZERO)]


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)          # raises without the HIP extension / a gfx950 device: no fallback
    yield e
    e.close()


@pytest.fixture(scope="module")
def keng():
    """the tool build (lib/libecgpu_knobs.so): the same kernel objects, ECGPU_NORM_K read from the environment"""
    e = ecgpu_module().Engine(0, variant="knobs")
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


# ---- case tables ------------------------------------------------------------------------------------------------------------

def _int(c, row):
    return int.from_bytes(bytes(row), c.order)


def _enc(c, v):
    return np.frombuffer(int(v).to_bytes(c.L, c.order), np.uint8)


@functools.lru_cache(None)
def tables(curve):
    """The M-case tables of one parameter set (rows of uint8):
      gen   k                 0: k = 0                                   1: k = 1, 2: k = n - 1
      var   k, xy, inf        0: k = 0, 1: identity flag, 2: both        3..5: k = 1, n - 1, 2
      ecdh  k, xy_real        (the same scalars over points without flags: 0 and 2 give the identity)
      madd  a, b, xy, inf     0: a = 0, 1: b = 0, 2: both, 3: a = -b s mod n with P = s G (the complete addition cancels), 4: identity flag
      norm  xyz               0: Z = 0 under non-zero X, Y, 1: (0 : 1 : 0)  2: Z = 1
      xyz   kx, xyz           0: Z = 0, 1: Z = 0 and k = 0, 2: k = 0"""
    c = pyec.CURVES[curve]
    L = c.L
    seed = 0x1A7E0000 + 16 * c.cid
    s = rand_scalars(c.cid, M, seed).reshape(M, L)
    xy_real = oracle_lib.batch_mul_base(c.cid, s.reshape(-1))[0].reshape(M, 2 * L)
    t = {"c": c, "xy_real": xy_real}
    gen = rand_scalars(c.cid, M, seed + 1).reshape(M, L).copy()
    gen[0], gen[1], gen[2] = 0, _enc(c, 1), _enc(c, c.n - 1)
    t["gen"] = gen
    k = rand_scalars(c.cid, M, seed + 2).reshape(M, L).copy()
    k[0], k[2], k[3], k[4], k[5] = 0, 0, _enc(c, 1), _enc(c, c.n - 1), _enc(c, 2)
    xy, inf = xy_real.copy(), np.zeros((M, 1), np.uint8)
    xy[1], xy[2], inf[1], inf[2] = 0, 0, 1, 1
    t["k"], t["xy"], t["inf"] = k, xy, inf
    a, b = rand_scalars(c.cid, M, seed + 3).reshape(M, L).copy(), rand_scalars(c.cid, M, seed + 4).reshape(M, L).copy()
    a[0], b[1], a[2], b[2] = 0, 0, 0, 0
    a[3] = _enc(c, -_int(c, b[3]) * _int(c, s[3]) % c.n)
    mxy, minf = xy_real.copy(), np.zeros((M, 1), np.uint8)
    mxy[4], minf[4] = 0, 1
    t["a"], t["b"], t["mxy"], t["minf"] = a, b, mxy, minf
    rng = np.random.default_rng(seed + 5)
    xyz = np.zeros((M, 3 * L), np.uint8)
    for j in range(M):
        z = int.from_bytes(rng.bytes(L), "big") % (c.p - 2) + 2
        x, y = _int(c, xy_real[j, :L]), _int(c, xy_real[j, L:])
        if j in (0, 1):
            xyz[j] = np.concatenate([_enc(c, z), _enc(c, x), _enc(c, 0)]) if j == 0 else np.concatenate([_enc(c, 0), _enc(c, 1), _enc(c, 0)])
        elif j == 2:
            xyz[j] = np.concatenate([xy_real[j], _enc(c, 1)])
        else:
            xyz[j] = np.concatenate([_enc(c, x * z % c.p), _enc(c, y * z % c.p), _enc(c, z)])
    t["xyz"] = xyz
    kx = rand_scalars(c.cid, M, seed + 6).reshape(M, L).copy()
    kx[1], kx[2] = 0, 0
    t["kx"] = kx
    return t


def flat(a):
    return np.ascontiguousarray(a).reshape(-1)


def rows(xy, inf):
    m = len(inf)
    return np.asarray(xy).reshape(m, -1).copy(), np.asarray(inf).reshape(m, 1).copy()


def same(got, want):
    return all(bytes(flat(g)) == bytes(flat(w)) for g, w in zip(got, want))


_SMALL = {}


def small(eng, curve):
    """name -> (value rows, flag rows): each entry point's own output on its M cases in ONE small call (K = 1, no stride), equal to the
    oracle's byte for byte.  Computed once per engine and parameter set (a batch is compared with the small call of the library build
    that ran it), with no tuning knob in the environment."""
    if (eng, curve) in _SMALL:
        return _SMALL[(eng, curve)]
    assert "ECGPU_NORM_K" not in os.environ
    t = tables(curve)
    c = t["c"]
    L, cid = c.L, c.cid
    out = {}
    want = rows(*oracle_lib.batch_mul_base(cid, flat(t["gen"])))
    out["gen"] = rows(*eng.mul_by_generator(cid, flat(t["gen"])))
    out["gen_ct"] = rows(*eng.mul_by_generator(cid, flat(t["gen"]), constant_time=True))
    assert same(out["gen"], want) and same(out["gen_ct"], want), curve
    assert want[1][0] == 1 and want[1].sum() == 1
    ypar = want[0][:, L if c.le else 2 * L - 1] & 1
    out["comp"] = rows(*eng.mul_by_generator_compressed(cid, flat(t["gen"])))
    assert same(out["comp"], (want[0][:, :L], np.where(want[1][:, 0] == 1, 0, 2 + ypar).astype(np.uint8))), curve
    want = rows(*oracle_lib.batch_mul(cid, flat(t["k"]), flat(t["xy"]), flat(t["inf"])))
    out["var"] = rows(*eng.mul(cid, flat(t["k"]), flat(t["xy"]), flat(t["inf"])))
    out["var_ct"] = rows(*eng.mul(cid, flat(t["k"]), flat(t["xy"]), flat(t["inf"]), constant_time=True))
    assert same(out["var"], want) and same(out["var_ct"], want), curve
    assert want[1][:3].all() and want[1].sum() == 3
    want = rows(*oracle_lib.batch_mul(cid, flat(t["k"]), flat(t["xy_real"])))
    out["ecdh"] = rows(*eng.ecdh(cid, flat(t["k"]), flat(t["xy_real"])))
    assert same(out["ecdh"], (want[0][:, :L], 1 - want[1])) and list(np.nonzero(want[1][:, 0])[0]) == [0, 2], curve
    each = [oracle_lib.mul_base_and_mul_add_vartime(cid, t["a"][j], t["b"][j], t["mxy"][j], int(t["minf"][j, 0])) for j in range(M)]
    want = (np.stack([e[0] for e in each]), np.array([[e[1]] for e in each], np.uint8))
    out["madd"] = rows(*eng.mul_by_generator_and_mul_add(cid, flat(t["a"]), flat(t["b"]), flat(t["mxy"]), flat(t["minf"])))
    assert same(out["madd"], want) and list(np.nonzero(want[1][:, 0])[0]) == [2, 3], curve
    aff = rows(*oracle_lib.batch_normalize(cid, flat(t["xyz"])))
    out["norm"] = rows(*eng.batch_normalize(cid, flat(t["xyz"])))
    assert same(out["norm"], aff) and list(np.nonzero(aff[1][:, 0])[0]) == [0, 1], curve
    want = rows(*oracle_lib.batch_mul(cid, flat(t["kx"]), flat(aff[0]), flat(aff[1])))
    out["xyz"] = rows(*eng.mul_vartime_xyz(cid, flat(t["kx"]), flat(t["xyz"])))
    out["xyz_ct"] = rows(*eng.mul_xyz(cid, flat(t["kx"]), flat(t["xyz"]), constant_time=True))
    assert same(out["xyz"], want) and same(out["xyz_ct"], want) and list(np.nonzero(want[1][:, 0])[0]) == [0, 1, 2], curve
    _SMALL[(eng, curve)] = out
    return out


# which table ids `plant` uses for each family: the cases whose RESULT is the identity (they are what a normalisation chain
# has to keep out of its product); the other degenerate inputs ride along in the tiling
PLANT_IDS = {"gen": (0,), "var": (0, 1, 2), "ecdh": (0, 2), "madd": (2, 3), "norm": (0, 1), "xyz": (0, 1)}


def check(got, want_small, idx, rep, what):
    """got: (values, flags) of the batch; the expectation is the small result's rows gathered by the index map"""
    for g, w, part in zip(got, want_small, ("values", "flags")):
        msg = lc.first_mismatch(np.asarray(g).reshape(len(idx), -1), w[idx], rep, "%s %s" % (what, part))
        if msg:
            print(msg)
        assert msg is None, msg


# ---- (a) forced K at small n ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K", FORCED_K)
@pytest.mark.parametrize("curve", EVERY_SET)
def test_forced_k_every_entry_point_that_normalizes(keng, curve, n, K, monkeypatch):
    """ECGPU_NORM_K on the tool build: chains of 3 (one ragged lane), 54 / 53, 2 (one ragged single record) and ONE lane of 256
    records, through every entry point that ends in launch_normalize."""
    sm = small(keng, curve)
    t = tables(curve)
    cid = t["c"].cid
    T = lc.norm_geometry(n, K)[1]
    maps = {fam: lc.plant(n, T, M, ids, 0xA0 + K) for fam, ids in PLANT_IDS.items()}
    g = lambda fam, col: flat(t[col][maps[fam][0]])
    monkeypatch.setenv("ECGPU_NORM_K", str(K))
    try:
        what = "%s n=%d K=%d " % (curve, n, K)
        check(keng.mul_by_generator(cid, g("gen", "gen")), sm["gen"], *maps["gen"], what + "mul_by_generator")
        check(keng.mul_by_generator(cid, g("gen", "gen"), constant_time=True), sm["gen_ct"], *maps["gen"], what + "mul_by_generator ct")
        check(keng.mul(cid, g("var", "k"), g("var", "xy"), g("var", "inf")), sm["var"], *maps["var"], what + "mul")
        check(keng.mul(cid, g("var", "k"), g("var", "xy"), g("var", "inf"), constant_time=True), sm["var_ct"], *maps["var"], what + "mul ct")
        check(keng.batch_normalize(cid, g("norm", "xyz")), sm["norm"], *maps["norm"], what + "batch_normalize")
        check(keng.mul_by_generator_and_mul_add(cid, g("madd", "a"), g("madd", "b"), g("madd", "mxy"), g("madd", "minf")), sm["madd"],
              *maps["madd"], what + "mul_by_generator_and_mul_add")
        check(keng.ecdh(cid, g("ecdh", "k"), g("ecdh", "xy_real")), sm["ecdh"], *maps["ecdh"], what + "ecdh")
    finally:
        monkeypatch.delenv("ECGPU_NORM_K")


# ---- (b) the product library at its own thresholds ------------------------------------------------------------------------------

@pytest.mark.parametrize("n,curve", [(N_K2, c) for c in EVERY_SET] + [(N_K3, c) for c in ("k256", "p256", "p384", "p521", "p224")])
def test_fixed_base_at_the_k2_and_k3_thresholds(eng, curve, n):
    """x || y (k_normalize, quad-major hand-over) and compressed output (launch_normalize_compressed, which has no knob)."""
    sm = small(eng, curve)
    t = tables(curve)
    K, T = lc.norm_geometry(n)
    assert K == (2 if n == N_K2 else 3)
    idx, rep = lc.plant(n, T, M, PLANT_IDS["gen"], 0xB0)
    scal = flat(t["gen"][idx])
    check(eng.mul_by_generator(t["c"].cid, scal), sm["gen"], idx, rep, "%s n=%d mul_by_generator" % (curve, n))
    check(eng.mul_by_generator_compressed(t["c"].cid, scal), sm["comp"], idx, rep, "%s n=%d mul_by_generator_compressed" % (curve, n))


@pytest.mark.parametrize("curve", ["k256", "p256", "p384", "p521", "bign256"])
def test_xyz_records_at_the_k2_threshold(eng, curve):
    """ecgpu_batch_mul_xyz and ecgpu_msm_xyz at n = 65537: k_xyz_affine on the device at K = 2 with Z = 0 records of every class.  The
    MSM's expectation is the oracle's MSM over the distinct cases, each weighted by its multiplicity in the index map."""
    sm = small(eng, curve)
    t = tables(curve)
    c = t["c"]
    n = N_K2
    idx, rep = lc.plant(n, lc.norm_geometry(n)[1], M, PLANT_IDS["xyz"], 0xB1)
    kx, xyz = flat(t["kx"][idx]), flat(t["xyz"][idx])
    check(eng.mul_vartime_xyz(c.cid, kx, xyz), sm["xyz"], idx, rep, "%s n=%d mul_vartime_xyz" % (curve, n))
    count = np.bincount(idx, minlength=M)
    weighted = b"".join(pyec.enc_scalar(c, int(count[j]) * _int(c, t["kx"][j]) % c.n) for j in range(M))
    aff = oracle_lib.batch_normalize(c.cid, flat(t["xyz"]))
    want = oracle_lib.msm(c.cid, weighted, aff[0], aff[1], vartime=True)
    got = eng.lincomb_xyz(c.cid, kx, xyz)
    planted = {name: [int(idx[r]) for r in cl["records"]] for name, cl in rep["classes"].items()}
    assert bytes(got[0]) == bytes(want[0]) and got[1] == want[1] == 0, \
        "%s n=%d lincomb_xyz: a sum has no failing index; multiplicities of cases 0, 1, 2 (Z = 0; Z = 0 and k = 0; k = 0): %s; planted case " \
        "ids by class: %s" % (curve, n, count[:3].tolist(), planted)


@functools.lru_cache(None)
def signature_tables(curve):
    c = pyec.CURVES[curve]
    ver = ecdsa_cases(c, 0x5161 + c.cid, nvalid=6)[:SIGNATURE_M[0]]
    rec = recover_cases(c, 0x5162 + c.cid, nvalid=5)
    rec = rec[:SIGNATURE_M[1] - 3] + rec[-3:]                 # the head (range failures among it) and the tail (x off the curve, x reduced)
    assert len(ver) == SIGNATURE_M[0] and len(rec) == SIGNATURE_M[1]
    return c, ver, rec


def _out_of_range(c, cases, col):
    """the cases whose column `col` (1 = r, 2 = s) is 0 or n: what k_scalar_batch_inv leaves out of a chain that inverts that column"""
    return tuple(j for j, t in enumerate(cases) if int.from_bytes(t[col], "big") in (0, c.n))


def assert_planted_records_are_skipped(idx, rep, skipped, what):
    """every record of every planted class holds a case the chain leaves out, and the rest of its lane holds none"""
    skip = np.zeros(idx.max() + 1, bool)
    skip[list(skipped)] = True
    for name, cl in rep["classes"].items():
        recs = lc.chain(cl["lane"], rep["n"], rep["T"])
        assert set(np.nonzero(skip[idx[recs]])[0].tolist()) == set(cl["positions"]), (what, name)


@pytest.mark.parametrize("curve", ["k256", "p384"])
def test_ecdsa_verify_and_recover_at_the_k2_threshold(eng, curve):
    """k_scalar_batch_inv at K = 2.  Verification inverts s and recovery r; an element that is 0 or n stays out of the lane's product.
    Those cases alone are planted by class — s = 0 and s = n for verification, r = 0 and r = n for recovery — so that a lane's whole
    chain is left out (`all`: the lane inverts the bare one), and so is the single record of the ragged lane; a tiled case set
    cannot produce either.  The other range failures (r for verification, s for recovery) ride along in the tiling."""
    c, ver, rec = signature_tables(curve)
    n, L = N_K2, c.L
    T = lc.norm_geometry(n)[1]
    z, r, s, q, exp = ecdsa_pack(ver)
    small_ok = eng.ecdsa_verify(c.cid, z, r, s, q)
    assert bytes(small_ok) == bytes(oracle_lib.ecdsa_verify(c.cid, z, r, s, q)) == bytes(exp)
    deg = _out_of_range(c, ver, 2)
    assert {int.from_bytes(ver[j][2], "big") for j in deg} == {0, c.n} and _out_of_range(c, ver, 1)     # (r = 0 / n: in the tiling)
    idx, rep = lc.plant(n, T, len(ver), deg, 0xB2)
    assert {"all", "ragged-last", "first", "last", "all-but-one", "record n-1", "record T-1", "record T"} == set(rep["classes"])
    assert_planted_records_are_skipped(idx, rep, deg, "verify")
    col = lambda b, w: flat(np.frombuffer(b, np.uint8).reshape(len(ver), w)[idx])
    got = eng.ecdsa_verify(c.cid, col(z, L), col(r, L), col(s, L), col(q, 2 * L))
    msg = lc.first_mismatch(got, small_ok.reshape(-1, 1)[idx], rep, "%s n=%d ecdsa_verify" % (curve, n))
    assert msg is None, msg
    z, r, s, recid, exp_xy, exp_ok = recover_pack(rec, L)
    small_xy, small_rok = eng.ecdsa_recover(c.cid, z, r, s, recid)
    want = oracle_lib.ecdsa_recover(c.cid, z, r, s, recid)
    assert bytes(small_xy) == bytes(want[0]) == exp_xy and bytes(small_rok) == bytes(want[1]) == bytes(exp_ok)
    deg = _out_of_range(c, rec, 1)
    assert {int.from_bytes(rec[j][1], "big") for j in deg} == {0, c.n} and _out_of_range(c, rec, 2)
    idx, rep = lc.plant(n, T, len(rec), deg, 0xB3)
    assert {"all", "ragged-last", "first", "last", "all-but-one", "record n-1", "record T-1", "record T"} == set(rep["classes"])
    assert_planted_records_are_skipped(idx, rep, deg, "recover")
    col = lambda b, w: flat(np.frombuffer(bytes(b), np.uint8).reshape(len(rec), w)[idx])
    got = eng.ecdsa_recover(c.cid, col(z, L), col(r, L), col(s, L), col(recid, 1))
    check(got, rows(small_xy, small_rok), idx, rep, "%s n=%d ecdsa_recover" % (curve, n))


# ---- device-resident calls ---------------------------------------------------------------------------------------------------

class Dev:
    """the device buffers of one test, freed together"""

    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def up(self, a):
        self.bufs.append(self.eng.to_device(flat(a)))
        return self.bufs[-1]

    def alloc(self, nbytes):
        self.bufs.append(self.eng.dev_alloc(nbytes + 16))
        return self.bufs[-1]

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


# name -> (table family, the small result it must reproduce, table columns, call(eng, cid, device columns, n, out, flags))
DEV_ENTRY = {
    "ecgpu_batch_mul_dev": ("var", "var", ("k", "xy", "inf"), lambda e, cid, d, n, o, f: e.mul_dev(cid, d[0], d[1], d[2], n, o, f)),
    "ecgpu_batch_mul_ct_dev": ("var", "var_ct", ("k", "xy", "inf"),
                               lambda e, cid, d, n, o, f: e.mul_dev(cid, d[0], d[1], d[2], n, o, f, constant_time=True)),
    "ecgpu_batch_mul_ct_xyz_dev": ("xyz", "xyz_ct", ("kx", "xyz"), lambda e, cid, d, n, o, f: e.mul_xyz_dev(cid, d[0], d[1], n, o, f, constant_time=True)),
    "ecgpu_batch_mul_xyz_dev": ("xyz", "xyz", ("kx", "xyz"), lambda e, cid, d, n, o, f: e.mul_vartime_xyz_dev(cid, d[0], d[1], n, o, f)),
    "ecgpu_batch_mul_base_and_mul_add_dev": ("madd", "madd", ("a", "b", "mxy", "minf"),
                                             lambda e, cid, d, n, o, f: e.mul_by_generator_and_mul_add_dev(cid, d[0], d[1], d[2], d[3], n, o, f)),
}
# the table ids of a pair's kinds in each family (madd: "k = 0" is b = 0, the multiplication the striding lane does)
PAIR_IDS = {"var": {ORD: 11, IDENT: 1, KZERO: 0}, "xyz": {ORD: 11, IDENT: 0, KZERO: 2}, "madd": {ORD: 11, IDENT: 4, KZERO: 1}}


def stride_map(family):
    """The index map of section (c): the classes of the K = 9 normalisation chains (lanes of 9 and 8 records), and on the variable-base
    lanes PAIR_LANES the pairs (record i, record i + 524288) of PAIRS.  -> (idx_map, report, {record: description})"""
    n, T = N_STRIDE, lc.var_geometry(N_STRIDE)
    Tn = lc.norm_geometry(n)[1]
    avoid = {r % Tn for lane in PAIR_LANES for r in (lane, lane + T)}
    idx, rep = lc.plant(n, Tn, M, PLANT_IDS[family], 0xC0, avoid=avoid)
    assert not rep["absent"] and not avoid & set(rep["lane_class"])
    pairs = {}
    for lane, (first, second) in zip(PAIR_LANES, PAIRS):
        idx[lane], idx[lane + T] = PAIR_IDS[family][first], PAIR_IDS[family][second]
        for r, pos in ((lane, 0), (lane + T, 1)):
            pairs[r] = "variable-base lane %d, record %d of its pair (%s, %s)" % (lane, pos, first, second)
    return idx, rep, pairs


def run_dev(eng, name, curve, idx):
    family, key, cols, call = DEV_ENTRY[name]
    t = tables(curve)
    c = t["c"]
    n = len(idx)
    dev = Dev(eng)
    try:
        d = [dev.up(t[col][idx]) for col in cols]
        o, f = dev.alloc(n * 2 * c.L), dev.alloc(n)
        call(eng, c.cid, d, n, o, f)
        return eng.to_host(o, n * 2 * c.L), eng.to_host(f, n)
    finally:
        dev.free()


def check_stride(got, want_small, idx, rep, pairs, what):
    T = lc.var_geometry(N_STRIDE)
    for g, w, part in zip(got, want_small, ("values", "flags")):
        g, want = np.asarray(g).reshape(len(idx), -1), w[idx]
        msg = lc.first_mismatch(g, want, rep, "%s %s" % (what, part))
        if msg:
            i = int(np.nonzero((g != want).any(axis=1))[0][0])
            msg += "; variable-base lane %d, record %d of its chain; %s" % (i % T, i // T, pairs.get(i, "no planted pair"))
            print(msg)
        assert msg is None, msg


@pytest.mark.parametrize("curve", ["k256", "p256", "p384"])
@pytest.mark.parametrize("name", sorted(DEV_ENTRY))
def test_striding_variable_base_lanes(eng, name, curve):
    """n = 524288 + 300 through the _dev forms (the host-pointer forms are cut into pieces below the stride): a lane's second record
    after a first that was the identity point / k = 0 / ordinary, and the other way round, on the lane's one table slot."""
    family, key = DEV_ENTRY[name][:2]
    sm = small(eng, curve)
    idx, rep, pairs = stride_map(family)
    check_stride(run_dev(eng, name, curve, idx), sm[key], idx, rep, pairs, "%s %s n=%d" % (name, curve, N_STRIDE))


# ---- (d) the K = 64 cap -------------------------------------------------------------------------------------------------------

def test_fixed_base_at_the_k64_cap(eng):
    """k256, n = 64 * 65536 + 5 device-resident: K = 64 (uncapped it would be 65), 65537 lanes, chains of 64 and 63; x || y and
    compressed output.  About 0.5 GB of caller buffers."""
    sm = small(eng, "k256")
    t = tables("k256")
    n, L = N_CAP, 32
    K, T = lc.norm_geometry(n)
    assert K == 64
    idx, rep = lc.plant(n, T, M, PLANT_IDS["gen"], 0xD0)
    assert not rep["absent"]
    dev = Dev(eng)
    try:
        d_k = dev.up(t["gen"][idx])
        d_o, d_f = dev.alloc(n * 2 * L), dev.alloc(n)
        eng.mul_by_generator_dev(0, d_k, n, d_o, d_f)
        check((eng.to_host(d_o, n * 2 * L), eng.to_host(d_f, n)), sm["gen"], idx, rep, "ecgpu_batch_mul_base_dev k256 n=%d" % n)
        eng.mul_by_generator_compressed_dev(0, d_k, n, d_o, d_f)
        check((eng.to_host(d_o, n * L), eng.to_host(d_f, n)), sm["comp"], idx, rep, "ecgpu_batch_mul_base_compressed_dev k256 n=%d" % n)
    finally:
        dev.free()


# ---- (e) a bad record's position does not matter ---------------------------------------------------------------------------------

def _code(call):
    ecgpu = ecgpu_module()
    with pytest.raises(ecgpu.EcgpuError) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("curve", ["k256", "p256"])
@pytest.mark.parametrize("name", ["ecgpu_batch_mul_dev", "ecgpu_batch_mul_xyz_dev"])
def test_a_bad_record_fails_the_striding_call_from_any_position(eng, name, curve):
    """An off-curve point, or a scalar >= n, in the second stride, at record n - 1 or in the middle of a normalisation chain: the error
    code of the small call with that record at index 0; the next clean call gives the planted batch's expectation."""
    ecgpu = ecgpu_module()
    family, key, cols, call = DEV_ENTRY[name]
    sm = small(eng, curve)
    t = tables(curve)
    c = t["c"]
    L = c.L
    idx, rep, pairs = stride_map(family)
    n = len(idx)
    bad_scalar = _enc(c, c.n)
    bad_point = t[cols[1]][20].copy()
    bad_point[2 * L - 1] ^= 1                                            # y with its lowest bit flipped: off the curve (Z != 0 in the xyz form)
    host = [flat(t[col][idx]).reshape(n, -1) for col in cols]

    def spoil(arrays, i, column):
        """record i: the bad scalar, or the bad point under an ordinary scalar and no identity flag"""
        arrays[0][i] = bad_scalar if column == 0 else _enc(c, 5)
        if column == 1:
            arrays[1][i] = bad_point
            if len(arrays) > 2:
                arrays[2][i] = 0

    dev = Dev(eng)
    try:
        d = [dev.up(h) for h in host]
        o, f = dev.alloc(n * 2 * L), dev.alloc(n)
        tiny = [dev.up(t[col][:4]) for col in cols]
        for column, expect in ((0, ecgpu.ERR_SCALAR_RANGE), (1, ecgpu.ERR_POINT)):
            first = [t[col][:4].copy() for col in cols]
            spoil(first, 0, column)
            for buf, h in zip(tiny, first):
                eng.to_device(flat(h), buf)
            small_code = _code(lambda: call(eng, c.cid, tiny, 4, o, f))
            assert small_code == expect
            for pos in BAD_POSITIONS:
                saved = [h[pos].copy() for h in host]
                spoil(host, pos, column)
                for buf, h in zip(d, host):
                    eng.to_device(flat(h), buf)
                assert _code(lambda: call(eng, c.cid, d, n, o, f)) == small_code, (name, curve, column, lc.describe(pos, rep))
                for h, v in zip(host, saved):
                    h[pos] = v
        for buf, h in zip(d, host):
            eng.to_device(flat(h), buf)
        call(eng, c.cid, d, n, o, f)
        check_stride((eng.to_host(o, n * 2 * L), eng.to_host(f, n)), sm[key], idx, rep, pairs, "%s %s after the failed calls" % (name, curve))
    finally:
        dev.free()


@pytest.mark.parametrize("curve", ["k256", "p521"])
def test_a_bad_scalar_fails_the_fixed_base_call_from_any_position(eng, curve):
    """mul_by_generator at n = 65537 with a scalar >= n at record n - 1, at the last position of a chain and on the ragged lane."""
    ecgpu = ecgpu_module()
    sm = small(eng, curve)
    t = tables(curve)
    c = t["c"]
    n = N_K2
    T = lc.norm_geometry(n)[1]
    idx, rep = lc.plant(n, T, M, PLANT_IDS["gen"], 0xE0)
    scal = t["gen"][idx]
    first = t["gen"][:4].copy()
    first[0] = _enc(c, c.n)
    small_code = _code(lambda: eng.mul_by_generator(c.cid, flat(first)))
    assert small_code == ecgpu.ERR_SCALAR_RANGE
    for pos in (n - 1, T + 5, T - 1):
        broken = scal.copy()
        broken[pos] = _enc(c, c.n)
        assert _code(lambda: eng.mul_by_generator(c.cid, flat(broken))) == small_code, (curve, lc.describe(pos, rep))
    check(eng.mul_by_generator(c.cid, flat(scal)), sm["gen"], idx, rep, "%s n=%d mul_by_generator after the failed calls" % (curve, n))
