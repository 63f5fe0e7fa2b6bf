"""Degenerate records at every position of a lane's record chain, without a GPU: the geometry and planting helper
(tests/lane_chains.py), the sizes of tests/test_gpu_lane_chains.py, and the lane bodies of k_xyz_affine, k_normalize and
k_scalar_batch_inv — three policies of one chain skeleton, csrc/ecgpu_batchinv.h — compiled for the CPU (tests/hostcheck_xyz_var,
tests/hostcheck; `nthreads` lanes) with planted degenerate and off-curve records against big-integer arithmetic, once more in a
stand-alone program under AddressSanitizer + UBSan."""
import fcntl
import itertools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import hostcheck_lib
import lane_chains as lc
import pyec
import test_gpu_lane_chains as gpu_file
from test_xyz_vartime import build_helper, convert, enc_xyz

XYZ_CURVES = ["k256", "p256", "p384", "p521", "p224", "bign256"]


# ---- the helper ---------------------------------------------------------------------------------------------------------

def gpu_geometries():
    """every (n, T) the GPU file runs: forced K, the launch's own K at its sizes, the variable-base stride"""
    out = [(n, lc.norm_geometry(n, K)[1]) for n, K in gpu_file.FORCED_K]
    out += [(n, lc.norm_geometry(n)[1]) for n in (gpu_file.N_K2, gpu_file.N_K3, gpu_file.N_STRIDE, gpu_file.N_CAP)]
    out.append((gpu_file.N_STRIDE, lc.var_geometry(gpu_file.N_STRIDE)))
    return out


def assert_partition(n, T):
    """the chains of T lanes cover range(n) once each, in steps of T, with the lengths chain_lengths gives (no loop over lanes)"""
    length, full = lc.chain_lengths(n, T)
    assert 0 < full <= T and full * length + (T - full) * (length - 1) == n, (n, T)
    assert (np.bincount(np.arange(n) % T, minlength=T) == np.where(np.arange(T) < full, length, length - 1)).all(), (n, T)
    for t in {0, full - 1, min(full, T - 1), T - 1}:
        recs = lc.chain(t, n, T)
        assert recs.tolist() == list(range(t, n, T)) and len(recs) == (length if t < full else length - 1), (n, T, t)


def test_chain_partitions_the_batch():
    for n in range(1, 601):
        for K in range(1, 10):
            assert_partition(n, lc.norm_geometry(n, K)[1])
    for n in (7, 40, 323):                                    # and lane by lane, where that is cheap
        for T in (1, 2, 6, 7, n):
            assert sorted(np.concatenate([lc.chain(t, n, T) for t in range(T)]).tolist()) == list(range(n))
    for n, T in gpu_geometries():
        assert_partition(n, T)


def test_geometry_restates_the_launchers():
    assert lc.norm_geometry(1) == (1, 1) and lc.norm_geometry(65536) == (1, 65536) and lc.norm_geometry(65537) == (2, 32769)
    assert lc.norm_geometry(64 * 65536) == (64, 65536) and lc.norm_geometry(1 << 24) == (64, 1 << 18)
    assert lc.norm_geometry(300) == (1, 300)                 # test_batch_normalize_and_point_sum_vs_oracle: no chain
    assert lc.var_geometry(1) == 256 and lc.var_geometry(257) == 512 and lc.var_geometry(524288) == 524288
    assert lc.var_geometry(524289) == 524288 and lc.var_geometry(1 << 20) == 524288
    # the host-pointer pipeline (PIPE_MIN = 2^19, pieces of 2^18) never shows a device call K > 4 or a striding lane
    assert lc.norm_geometry(1 << 18)[0] == 4 and lc.var_geometry(1 << 18) == 1 << 18


def test_gpu_parameter_table():
    """The sizes of tests/test_gpu_lane_chains.py give the geometries its docstrings promise."""
    assert gpu_file.FORCED_K == [(701, 3), (323, 64), (257, 2), (256, 1024)]
    geo = {(n, K): (lc.norm_geometry(n, K)[1],) + lc.chain_lengths(n, lc.norm_geometry(n, K)[1]) for n, K in gpu_file.FORCED_K}
    assert geo[(701, 3)] == (234, 3, 233)                    # (T, chain length, full lanes)
    assert geo[(323, 64)] == (6, 54, 5)
    assert geo[(257, 2)] == (129, 2, 128)
    assert geo[(256, 1024)] == (1, 256, 1)                   # one lane owns the whole batch
    assert gpu_file.N_K2 == 65537 and lc.norm_geometry(65537) == (2, 32769) and lc.chain_lengths(65537, 32769) == (2, 32768)
    assert gpu_file.N_K3 == 131075 and lc.norm_geometry(131075) == (3, 43692) and lc.chain_lengths(131075, 43692) == (3, 43691)
    assert gpu_file.N_STRIDE == 524288 + 300 and lc.var_geometry(gpu_file.N_STRIDE) == 524288
    assert lc.chain_lengths(gpu_file.N_STRIDE, 524288) == (2, 300)          # lanes 0..299 own two records
    assert lc.norm_geometry(gpu_file.N_STRIDE) == (9, 58288)
    assert gpu_file.N_CAP == 64 * 65536 + 5 == 4194309
    assert (gpu_file.N_CAP + 65535) // 65536 == 65 and lc.norm_geometry(gpu_file.N_CAP) == (64, 65537)
    assert lc.chain_lengths(gpu_file.N_CAP, 65537) == (64, 65478)           # lanes 0..65477: 64 records, the rest 63
    for n, T in gpu_geometries():
        assert T == 1 or T % gpu_file.M, (n, T)              # the tiling prime divides no lane count
        for m in gpu_file.SIGNATURE_M:
            assert T % m, (n, T, m)
    assert all(m > 1 and all(m % q for q in range(2, int(m ** 0.5) + 1)) for m in [gpu_file.M] + list(gpu_file.SIGNATURE_M))
    # the pairs of section (c) and the bad positions of section (e) lie where they are meant to
    T, Tn = 524288, 58288
    for lane in gpu_file.PAIR_LANES:
        assert 0 < lane < 299 and lane + T < gpu_file.N_STRIDE
    assert gpu_file.BAD_POSITIONS[0] == T + 7 and gpu_file.BAD_POSITIONS[1] == gpu_file.N_STRIDE - 1
    mid = gpu_file.BAD_POSITIONS[2]
    assert 0 < mid // Tn < 8 and mid < T                     # an interior position of a K = 9 chain, a first-stride record


def admitted(n, T):
    """the classes the geometry has a chain for"""
    length, full = lc.chain_lengths(n, T)
    out = {"record n-1", "record T-1", "all"}
    if n > T:
        out.add("record T")
    if length >= 2:
        out |= {"first", "last", "all-but-one"}
    if length >= 3:
        out |= {"middle", "adjacent"}
    if full < T:
        out.add("ragged-last")
    return out


def check_plant(n, T, m, deg, seed):
    """-> (idx, report, roomy).  Every class is planted or reported absent; a planted lane is degenerate at its class's positions and
    nowhere else; where lanes are to spare (`roomy`) every class the geometry admits is planted."""
    idx, rep = lc.plant(n, T, m, deg, seed)
    assert idx.dtype == np.int32 and idx.shape == (n,) and idx.min() >= 0 and idx.max() < m
    want = admitted(n, T)
    length, full = lc.chain_lengths(n, T)
    record_lanes = {T - 1, (n - 1) % T} | ({0} if n > T else set())
    roomy = full - len([t for t in record_lanes if t < full]) >= 6 and (full == T or any(t not in record_lanes for t in range(full, T))) \
        and len(record_lanes) == (3 if n > T else 2)
    cl = rep["classes"]
    for name in lc.CLASSES:
        assert (name in cl) != (name in rep["absent"]), (n, T, name)
        if name in cl:
            assert name in want, (n, T, name)
        elif roomy:
            assert name not in want, (n, T, name, rep["absent"][name])
    is_deg = np.zeros(m, bool)
    is_deg[list(deg)] = True
    by_lane = {}
    for name, c in cl.items():
        recs = lc.chain(c["lane"], n, T)
        assert [int(recs[p]) for p in c["positions"]] == c["records"]
        assert by_lane.setdefault(c["lane"], c["positions"]) == c["positions"], (n, T, name)     # a lane of its own, or the same records
        assert set(np.nonzero(is_deg[idx[recs]])[0].tolist()) == set(c["positions"]), (n, T, name)
        assert name in rep["lane_class"][c["lane"]]
    # the shape of each class
    k = lambda name: len(lc.chain(cl[name]["lane"], n, T))
    if "first" in cl:
        assert cl["first"]["positions"] == [0] and k("first") >= 2
    if "middle" in cl:
        assert 0 < cl["middle"]["positions"][0] < k("middle") - 1
    if "last" in cl:
        assert cl["last"]["lane"] < full and cl["last"]["positions"] == [length - 1] and length >= 2
    if "adjacent" in cl:
        a, b = cl["adjacent"]["positions"]
        assert b == a + 1 and k("adjacent") >= 3
    if "all" in cl:
        assert cl["all"]["positions"] == list(range(k("all")))
    if "all-but-one" in cl:
        assert len(cl["all-but-one"]["positions"]) == k("all-but-one") - 1 >= 1
    if "ragged-last" in cl:
        assert cl["ragged-last"]["lane"] >= full and cl["ragged-last"]["positions"] == [length - 2]
    for name, rec in (("record n-1", n - 1), ("record T-1", T - 1), ("record T", T)):
        if name in cl:
            assert cl[name]["records"] == [rec]
    # outside the planted lanes the map is the tiling
    mask = np.ones(n, bool)
    for t in by_lane:
        mask[lc.chain(t, n, T)] = False
    assert (idx[mask] == (np.arange(n)[mask] % m)).all()
    return idx, rep, roomy


def test_plant_reports_every_class_the_geometry_admits():
    for n, T in gpu_geometries():
        idx, rep, _ = check_plant(n, T, gpu_file.M, (0, 1, 2), 7)
        if "record n-1" in rep["classes"]:
            assert "record %d = lane" % (n - 1) in lc.describe(n - 1, rep) and "record n-1" in lc.describe(n - 1, rep)
    # the geometries with every class: a ragged group of several lanes, chains of 3 or more, lanes to spare
    for n in (gpu_file.N_CAP, gpu_file.N_STRIDE):
        _, rep, roomy = check_plant(n, lc.norm_geometry(n)[1], gpu_file.M, (0, 3), 11)
        assert roomy and not rep["absent"], rep["absent"]
    # one ragged lane, which is lane T - 1: `ragged-last` has it, and `record T-1` would make the lane another shape
    for n, K in ((701, 3), (131075, None)):
        _, rep, _ = check_plant(n, lc.norm_geometry(n, K)[1], gpu_file.M, (0, 3), 11)
        assert list(rep["absent"]) == ["record T-1"], rep["absent"]
    # chains of 2: no middle, no adjacent (the single record of the ragged lane is `ragged-last` and `record T-1` at once)
    _, rep, _ = check_plant(65537, 32769, gpu_file.M, (0,), 3)
    assert sorted(rep["absent"]) == ["adjacent", "middle"]
    # one record per lane: nothing but the record classes and `all`; one lane: one class
    _, rep, _ = check_plant(300, 300, gpu_file.M, (0,), 3)
    assert sorted(rep["classes"]) == ["all", "record T-1", "record n-1"]
    _, rep, _ = check_plant(256, 1, gpu_file.M, (0,), 3)
    assert list(rep["classes"]) == ["middle"]
    for n in range(2, 120, 7):
        for K in (1, 2, 3, 5, 64):
            T = lc.norm_geometry(n, K)[1]
            if T == 1 or T % 7:
                check_plant(n, T, 7, (0, 4), n + K)


def test_first_mismatch_names_lane_position_and_class():
    n, T = 701, 234
    idx, rep = lc.plant(n, T, 61, (0,), 5)
    want = np.arange(n * 4, dtype=np.uint8).reshape(n, 4)
    assert lc.first_mismatch(want.copy(), want, rep) is None
    got = want.copy()
    lane = rep["classes"]["middle"]["lane"]
    got[lane] ^= 1                                            # position 0 of the `middle` lane: what a poisoned inverse spoils
    msg = lc.first_mismatch(got, want, rep, "x")
    assert "record %d = lane %d, chain position 0 of 3, class middle" % (lane, lane) in msg and "classes hit: middle" in msg


# ---- the lane body of k_xyz_affine on the CPU -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hx():
    return build_helper()


def to_affine(c, X, Y, Z):
    """-> (x || y bytes, identity flag): `ProjectivePoint::to_affine` on Python integers"""
    if Z == 0:
        return bytes(2 * c.L), 1
    zi = pow(Z, -1, c.p)
    return (X * zi % c.p).to_bytes(c.L, c.order) + (Y * zi % c.p).to_bytes(c.L, c.order), 0


def ordinary(c, rng):
    P = pyec.mul(c, rng.randrange(1, c.n), pyec.G(c))
    z = rng.randrange(2, c.p)
    return (P[0] * z % c.p, P[1] * z % c.p, z)


def run(hx, c, recs, nthreads):
    """the conversion of `recs` ((X, Y, Z) integer triples) and its expectation"""
    xyz = b"".join(enc_xyz(c, *r) for r in recs)
    got, ginf, ok = convert(hx, c, xyz, nthreads)
    want = [to_affine(c, *r) for r in recs]
    return got.reshape(len(recs), 2 * c.L), ginf, ok, np.frombuffer(b"".join(w[0] for w in want), np.uint8).reshape(len(recs), 2 * c.L), \
        np.array([w[1] for w in want], np.uint8)


@pytest.mark.parametrize("name", XYZ_CURVES)
def test_every_subset_of_identities_on_a_chain(hx, name):
    """n = 11 records on 4 lanes: chains of 3, 3, 3 and 2.  All 8 subsets of Z = 0 on the length-3 lane 1 times all 4 on the
    length-2 lane 3; lanes 0 and 2 hold ordinary records."""
    c = pyec.CURVES[name]
    rng = random.Random(0x1A5E + c.cid)
    n, T = 11, 4
    assert [len(lc.chain(t, n, T)) for t in range(T)] == [3, 3, 3, 2]
    base = [ordinary(c, rng) for _ in range(n)]
    for sub3 in itertools.product((0, 1), repeat=3):
        for sub2 in itertools.product((0, 1), repeat=2):
            recs = list(base)
            for hit, j in zip(sub3 + sub2, lc.chain(1, n, T).tolist() + lc.chain(3, n, T).tolist()):
                if hit:
                    recs[j] = (rng.randrange(1, c.p), rng.randrange(1, c.p), 0)
            got, ginf, ok, want, winf = run(hx, c, recs, T)
            assert ok.all(), (name, sub3, sub2)
            bad = np.nonzero((got != want).any(axis=1) | (ginf != winf))[0]
            assert bad.size == 0, (name, sub3, sub2, "record %d = lane %d, position %d" % (bad[0], bad[0] % T, bad[0] // T))


def xyz_table(c, rng, m):
    """m records: 0 = Z = 0 under arbitrary X, Y; 1 = (0 : 1 : 0); 2 = (0 : 0 : 0); 3 = Z = 1; the rest under random Z"""
    tab = [ordinary(c, rng) for _ in range(m)]
    tab[0] = (rng.randrange(1, c.p), rng.randrange(1, c.p), 0)
    tab[1] = (0, 1, 0)
    tab[2] = (0, 0, 0)
    P = pyec.mul(c, rng.randrange(1, c.n), pyec.G(c))
    tab[3] = (P[0], P[1], 1)
    return tab


@pytest.mark.parametrize("name", XYZ_CURVES)
@pytest.mark.parametrize("T", [6, 22])
def test_planted_identities_on_long_chains(hx, name, T):
    """n = 323 records on 6 lanes (chains of 54 and 53) with every class of lane_chains.plant that 6 lanes have room for, and on 22
    lanes (chains of 15 and 14) with all of them."""
    c = pyec.CURVES[name]
    rng = random.Random(0x1A5F + c.cid)
    n, m = 323, 13
    tab = xyz_table(c, rng, m)
    idx, rep = lc.plant(n, T, m, (0, 1, 2), 0x51 + c.cid)
    assert {"first", "middle", "last", "adjacent", "ragged-last", "record n-1"} <= set(rep["classes"])
    assert T == 6 or not rep["absent"]
    got, ginf, ok, want, winf = run(hx, c, [tab[j] for j in idx], T)
    assert ok.all()
    assert lc.first_mismatch(got, want, rep, name) is None, lc.first_mismatch(got, want, rep, name)
    assert lc.first_mismatch(ginf, winf, rep, name) is None, lc.first_mismatch(ginf, winf, rep, name)
    assert winf.sum() >= len({r for c in rep["classes"].values() for r in c["records"]}) >= 7      # every planted record is an identity


@pytest.mark.parametrize("name", XYZ_CURVES)
def test_a_bad_record_fails_alone_wherever_it_sits(hx, name):
    """An off-curve X || Y || Z (Z != 0) at the first, a middle and the last position of a chain: ok = 0 for that record only and
    every other output unchanged — also with an identity beside it in the chain."""
    c = pyec.CURVES[name]
    rng = random.Random(0x1A60 + c.cid)
    n, T = 11, 4
    base = [ordinary(c, rng) for _ in range(n)]
    base[6] = (rng.randrange(1, c.p), rng.randrange(1, c.p), 0)           # lane 2, middle: an identity in the chain of record 2 / 10
    good = run(hx, c, base, T)
    assert good[2].all()
    X, Y, Z = ordinary(c, rng)
    bad = (X, (Y + 1) % c.p, Z)
    for j in (1, 5, 9, 2, 10, 3, 7):                          # lane 1: first, middle, last; lane 2 around its identity; lane 3: both ends
        recs = list(base)
        recs[j] = bad
        got, ginf, ok, _, _ = run(hx, c, recs, T)
        assert np.nonzero(ok == 0)[0].tolist() == [j], (name, j)
        keep = np.arange(n) != j
        assert np.array_equal(got[keep], good[0][keep]) and np.array_equal(ginf[keep], good[1][keep]), (name, j)


# ---- the lane bodies of k_normalize and k_scalar_batch_inv on the CPU -------------------------------------------------------------
# Expectations from Python integers alone: pow(Z, -1, p), pow(a, -1, n).

NORM_MODES = {"wire": 0, "compressed": 2}                     # NORM_WIRE, NORM_COMPRESSED (csrc/ecgpu_batchinv.h)
N_SUB, T_SUB = 11, 4                                          # chains of 3, 3, 3, 2
N_LONG, M_LONG = 323, 13


def subsets():
    """the 8 x 4 subsets of the records of lane 1 (3 records) and lane 3 (2 records) of 11 records on 4 lanes"""
    recs = lc.chain(1, N_SUB, T_SUB).tolist() + lc.chain(3, N_SUB, T_SUB).tolist()
    assert recs == [1, 5, 9, 3, 7]
    return [[j for hit, j in zip(bits, recs) if hit] for bits in itertools.product((0, 1), repeat=5)]


def normalized(c, mode, recs):
    """-> (rows, flags) of k_normalize in `mode` for (X, Y, Z) integer triples"""
    rows, flags = [], []
    for r in recs:
        xy, inf = to_affine(c, *r)
        rows.append(xy if mode == 0 else xy[: c.L])
        flags.append(inf if mode == 0 else 0 if inf else 2 + (int.from_bytes(xy[c.L:], c.order) & 1))
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(recs), -1), np.array(flags, np.uint8)


def xyz_bytes(c, recs):
    return b"".join(enc_xyz(c, *r) for r in recs)


def subset_records(c, rng):
    """[(records, planted)]: the 32 subsets as Z = 0 records under arbitrary X, Y among ordinary ones"""
    base = [ordinary(c, rng) for _ in range(N_SUB)]
    out = []
    for hit in subsets():
        recs = list(base)
        for j in hit:
            recs[j] = (rng.randrange(1, c.p), rng.randrange(1, c.p), 0)
        out.append((recs, hit))
    return out


@pytest.mark.parametrize("mode", sorted(NORM_MODES))
@pytest.mark.parametrize("name", XYZ_CURVES)
def test_normalize_body_every_subset_of_identities_on_a_chain(name, mode):
    """The shape of test_every_subset_of_identities_on_a_chain through the lane body of k_normalize, x || y and compressed output."""
    c = pyec.CURVES[name]
    for recs, hit in subset_records(c, random.Random(0x2A5E + c.cid)):
        got, gflag = hostcheck_lib.normalize(c.cid, NORM_MODES[mode], xyz_bytes(c, recs), T_SUB)
        want, wflag = normalized(c, NORM_MODES[mode], recs)
        bad = np.nonzero((got.reshape(N_SUB, -1) != want).any(axis=1) | (gflag != wflag))[0]
        assert bad.size == 0, (name, mode, hit, "record %d = lane %d, position %d" % (bad[0], bad[0] % T_SUB, bad[0] // T_SUB))


@pytest.mark.parametrize("mode", sorted(NORM_MODES))
@pytest.mark.parametrize("name", XYZ_CURVES)
@pytest.mark.parametrize("T", [6, 22])
def test_normalize_body_planted_identities_on_long_chains(name, T, mode):
    """n = 323 on 6 and 22 lanes with the classes of lane_chains.plant, as test_planted_identities_on_long_chains."""
    c = pyec.CURVES[name]
    tab = xyz_table(c, random.Random(0x2A5F + c.cid), M_LONG)
    idx, rep = lc.plant(N_LONG, T, M_LONG, (0, 1, 2), 0x52 + c.cid)
    assert {"first", "middle", "last", "adjacent", "ragged-last", "record n-1"} <= set(rep["classes"]) and (T == 6 or not rep["absent"])
    recs = [tab[j] for j in idx]
    got, gflag = hostcheck_lib.normalize(c.cid, NORM_MODES[mode], xyz_bytes(c, recs), T)
    want, wflag = normalized(c, NORM_MODES[mode], recs)
    assert lc.first_mismatch(got, want, rep, name) is None, lc.first_mismatch(got, want, rep, name)
    assert lc.first_mismatch(gflag, wflag, rep, name) is None, lc.first_mismatch(gflag, wflag, rep, name)
    assert (wflag == 0).sum() >= 7 if mode == "compressed" else wflag.sum() >= 7


def scalar_degenerates(c):
    return [0, c.n, 2 ** (8 * c.L) - 1]


def inverses(c, xs):
    """k_scalar_batch_inv's contract: 0 for an element outside [1, n - 1], the inverse modulo n otherwise"""
    return b"".join((pow(x, -1, c.n) if 0 < x < c.n else 0).to_bytes(c.L, c.order) for x in xs)


def scalar_bytes(c, xs):
    return b"".join(x.to_bytes(c.L, c.order) for x in xs)


def subset_scalars(c, rng):
    base = [rng.randrange(1, c.n) for _ in range(N_SUB)]
    base[0], base[2] = 1, c.n - 1                             # the ends of the range are ordinary elements
    out = []
    for k, hit in enumerate(subsets()):
        xs = list(base)
        for i, j in enumerate(hit):
            xs[j] = scalar_degenerates(c)[(i + k) % 3]
        out.append((xs, hit))
    return out


def long_scalars(c, rng, T, seed):
    tab = scalar_degenerates(c) + [1, c.n - 1] + [rng.randrange(1, c.n) for _ in range(M_LONG - 5)]
    idx, rep = lc.plant(N_LONG, T, M_LONG, (0, 1, 2), seed)
    return [tab[j] for j in idx], rep


@pytest.mark.parametrize("name", sorted(pyec.CURVES))
def test_scalar_body_every_subset_of_degenerates_on_a_chain(name):
    """0, n and 2^(8L) - 1 at every subset of positions of a length-3 and a length-2 chain: 0 for those, the inverse modulo n for
    every other element of the lane."""
    c = pyec.CURVES[name]
    for xs, hit in subset_scalars(c, random.Random(0x3A5E + c.cid)):
        got = hostcheck_lib.scalar_batch_inv(c.cid, scalar_bytes(c, xs), T_SUB).reshape(N_SUB, c.L)
        want = np.frombuffer(inverses(c, xs), np.uint8).reshape(N_SUB, c.L)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (name, hit, "record %d = lane %d, position %d" % (bad[0], bad[0] % T_SUB, bad[0] // T_SUB))


@pytest.mark.parametrize("name", sorted(pyec.CURVES))
@pytest.mark.parametrize("T", [6, 22])
def test_scalar_body_planted_degenerates_on_long_chains(name, T):
    c = pyec.CURVES[name]
    xs, rep = long_scalars(c, random.Random(0x3A5F + c.cid), T, 0x53 + c.cid)
    assert {"first", "middle", "last", "adjacent", "ragged-last", "record n-1"} <= set(rep["classes"]) and (T == 6 or not rep["absent"])
    got = hostcheck_lib.scalar_batch_inv(c.cid, scalar_bytes(c, xs), T)
    want = np.frombuffer(inverses(c, xs), np.uint8)
    assert lc.first_mismatch(got, want, rep, name) is None, lc.first_mismatch(got, want, rep, name)
    assert sum(1 for x in xs if not 0 < x < c.n) >= 7


# ---- the three bodies in a stand-alone program under the sanitizers ------------------------------------------------------------------

HC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")
SAN_SRC, SAN_PROG = os.path.join(HC, "batchinv_san.cpp"), os.path.join(HC, "batchinv_san")


def build_san():
    csrc = os.path.join(os.path.dirname(os.path.dirname(HC)), "elliptic-curves_amd", "csrc")
    deps = [SAN_SRC, os.path.join(HC, "batchinv_host.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    with open(SAN_PROG + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(SAN_PROG) or os.path.getmtime(SAN_PROG) < max(os.path.getmtime(d) for d in deps):
            tmp = SAN_PROG + ".tmp.%d" % os.getpid()
            # (the runtimes linked into the program itself: it needs no preload)
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=undefined,address",
                                   "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", tmp, SAN_SRC])
            os.replace(tmp, SAN_PROG)


def san_case(kind, c, mode, n, T, data, want):
    return struct.pack("<7I", kind, c.cid, mode, n, T, len(data), len(want)) + data + want


def test_sanitized_standalone_program():
    """AddressSanitizer + UBSan on the three lane bodies over buffers of exactly n records: both shapes, outputs compared inside
    the program with the values computed here."""
    build_san()
    cases = []
    for name in sorted(pyec.CURVES):
        c = pyec.CURVES[name]
        rng = random.Random(0x4A5E + c.cid)
        shapes = [(xs, T_SUB) for xs, _ in subset_scalars(c, rng)[::5]] + [(long_scalars(c, rng, T, 0x54 + c.cid)[0], T) for T in (6, 22)]
        cases += [san_case(2, c, 0, len(xs), T, scalar_bytes(c, xs), inverses(c, xs)) for xs, T in shapes]
        if name not in XYZ_CURVES:
            continue
        tab = xyz_table(c, rng, M_LONG)
        shapes = [(recs, T_SUB) for recs, _ in subset_records(c, rng)[::5]]
        shapes += [([tab[j] for j in lc.plant(N_LONG, T, M_LONG, (0, 1, 2), 0x55 + c.cid)[0]], T) for T in (6, 22)]
        for recs, T in shapes:
            n = len(recs)
            for mode in NORM_MODES.values():
                rows, flags = normalized(c, mode, recs)
                cases.append(san_case(0, c, mode, n, T, xyz_bytes(c, recs), rows.tobytes() + flags.tobytes()))
            rows, flags = normalized(c, 0, recs)              # every record here is on the curve or an identity: verdict 1
            cases.append(san_case(1, c, 0, n, T, xyz_bytes(c, recs), rows.tobytes() + flags.tobytes() + bytes([1]) * n))
    r = subprocess.run([SAN_PROG], input=b"".join(cases), capture_output=True)
    assert r.returncode == 0 and r.stdout.decode().strip() == "%d cases equal" % len(cases), (r.returncode, r.stdout[-300:], r.stderr[-3000:])
