"""Projective (X : Y : Z) inputs of the variable-time entry points (ecgpu_batch_mul_xyz, ecgpu_msm_xyz,
ecgpu_batch_mul_base_and_mul_add_xyz, ecgpu_msm_parts_xyz_dev, ecgpu_group_msm_xyz and their _dev forms), checked without a
GPU: the ABI surface (header, library, Python and Rust bindings, the Rust call sites), the record codecs of the new kernel
(k_xyz_affine) under tools/wire_codec_isa_check.py, and its lane body compiled for the CPU (tests/hostcheck_xyz_var) against
the oracle's `to_affine` (ecref_batch_normalize)."""
import ctypes
import fcntl
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import lane_chains
import oracle_lib
import pyec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostcheck_xyz_var")
SRC = os.path.join(HERE, "hostcheck_xyz_var.cpp")
LIB = os.path.join(HERE, "libhostcheck_xyz_var.so")
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")
NEW = ["ecgpu_batch_mul_xyz", "ecgpu_batch_mul_xyz_dev", "ecgpu_msm_xyz", "ecgpu_msm_xyz_dev", "ecgpu_batch_mul_base_and_mul_add_xyz",
       "ecgpu_batch_mul_base_and_mul_add_xyz_dev", "ecgpu_msm_parts_xyz_dev", "ecgpu_group_msm_xyz", "ecgpu_group_msm_xyz_dev"]
_u8p = ctypes.POINTER(ctypes.c_uint8)


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ---- the ABI surface ----------------------------------------------------------------------------------------------------

def test_header_declares_the_vartime_xyz_entry_points():
    src = _strip_comments(open(os.path.join(ROOT, "include", "ecgpu.h")).read())
    for name in NEW:
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, src)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        pts = [a for a in args if "points" in a]
        assert len(pts) == 1 and "points_xyz" in pts[0], (name, args)      # one point array, X || Y || Z
        assert not any("inf" in a and "out" not in a for a in args), (name, args)   # no identity-flag input


def test_bindings_list_the_vartime_xyz_entry_points():
    sys.path.insert(0, ROOT)
    import importlib
    mod = importlib.import_module("elliptic-curves_amd")
    for name in NEW:
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("mul_vartime_xyz", "mul_vartime_xyz_dev", "lincomb_xyz", "lincomb_xyz_dev", "mul_by_generator_and_mul_add_xyz",
                 "mul_by_generator_and_mul_add_xyz_dev", "msm_parts_xyz_dev"):
        assert callable(getattr(mod.Engine, meth)), meth
    for meth in ("lincomb_xyz", "lincomb_xyz_dev"):
        assert callable(getattr(mod.Group, meth)), meth
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, rs), name


def test_library_exports_the_vartime_xyz_entry_points():
    so = os.path.join(ROOT, "elliptic-curves_amd", "lib", "libecgpu.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    for name in NEW:
        assert hasattr(lib, name), name


def _shim_fn(src, name):
    """the body of `pub fn name` in the shim (up to the next `pub fn` / end of the module)"""
    m = re.search(r"pub fn %s\b.*?(?=\n    pub fn |\n}\s*$)" % name, src, re.S)
    assert m, name
    return m.group(0)


@pytest.mark.parametrize("name,calls", [
    ("batch_mul_vartime", ["ecgpu_batch_mul_xyz("]),
    ("lincomb_vartime", ["ecgpu_group_msm_xyz(", "ecgpu_msm_xyz("]),
    ("batch_mul_by_generator_and_mul_add_vartime", ["ecgpu_batch_mul_base_and_mul_add_xyz("]),
])
def test_shim_ships_projective_records(name, calls):
    """The Rust drop-ins of `mul_vartime`, `lincomb_vartime` (group branch and single-engine fallback) and
    `mul_by_generator_and_mul_add_vartime` ship X || Y || Z: no `to_affine` per point on the CPU."""
    body = _strip_comments(open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read())
    fn = _shim_fn(body, name)
    for call in calls:
        assert call in fn, (name, call)
    assert "points_to_wire_xyz::<C>" in fn and "points_to_wire::<C>" not in fn, name
    assert "ProjectiveCoordinates<C>" in fn, name
    for affine in ("ecgpu_batch_mul(", "ecgpu_msm(", "ecgpu_group_msm(", "ecgpu_batch_mul_base_and_mul_add("):
        assert affine not in fn, (name, affine)


def test_mul_xyz_points_at_the_vartime_forms():
    """mul_xyz(constant_time=False) is still an argument error, and its message names the variable-time methods."""
    sys.path.insert(0, ROOT)
    import importlib
    mod = importlib.import_module("elliptic-curves_amd")
    eng = mod.Engine.__new__(mod.Engine)
    with pytest.raises(mod.EcgpuError) as e:
        eng.mul_xyz(0, b"", b"", constant_time=False)
    assert e.value.code == mod.ERR_ARG
    for meth in ("mul_vartime_xyz", "lincomb_xyz", "mul_by_generator_and_mul_add_xyz", "msm_parts_xyz_dev", "Group.lincomb_xyz"):
        assert meth in str(e.value), meth


# ---- the record codecs of the new kernel --------------------------------------------------------------------------------

def test_xyz_affine_record_codecs_move_whole_words():
    """k_xyz_affine reads 3L-byte records (p521 198, p224 84, p192 72 bytes): tools/wire_codec_isa_check.py on the base group."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wire_codec_isa_check.py"), "--curve", "P521Params", "--curve",
                        "P224Params", "--curve", "P192Params", "--groups", "base"], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    for c in ("P521Params", "P224Params", "P192Params"):
        assert "k_xyz_affine<ecgpu::%s>" % c in r.stdout, c


# ---- the lane body on the CPU -------------------------------------------------------------------------------------------

def build_helper():
    deps = [SRC, os.path.join(ROOT, "tests", "hostcheck", "batchinv_host.h")] + [os.path.join(CSRC, f) for f in (
        "ecgpu_xyz.h", "ecgpu_batchinv.h", "ecgpu_scalar.h", "ecgpu_field.h", "ecgpu_params.h", "ecgpu_field_consts.h", "ecgpu_point.h", "ecgpu_modinv.h")]

    def fresh():
        return os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps)
    if not fresh():
        with open(LIB + ".lock", "w") as lock:             # (pytest-xdist workers: one builds, the others wait)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not fresh():
                tmp = LIB + ".tmp.%d" % os.getpid()
                subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", tmp, SRC])
                os.replace(tmp, LIB)
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def hx():
    return build_helper()


def convert(hx, c, xyz, nthreads=0):
    """nthreads = 0: the lanes of launch_xyz_affine for n records (lane_chains.norm_geometry)"""
    n = len(xyz) // (3 * c.L)
    if nthreads == 0 and n:
        nthreads = lane_chains.norm_geometry(n)[1]
    p = np.frombuffer(xyz, np.uint8).copy()
    out, inf, ok = np.zeros(n * 2 * c.L, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    assert hx.hx_xyz_affine(c.cid, p.ctypes.data_as(_u8p), ctypes.c_size_t(n), ctypes.c_size_t(nthreads), out.ctypes.data_as(_u8p),
                            inf.ctypes.data_as(_u8p), ok.ctypes.data_as(_u8p)) == 0
    return out, inf, ok


def enc_xyz(c, X, Y, Z):
    return X.to_bytes(c.L, c.order) + Y.to_bytes(c.L, c.order) + Z.to_bytes(c.L, c.order)


def rescale(c, P, z):
    if P is None:
        return enc_xyz(c, 0, z % c.p, 0)
    return enc_xyz(c, P[0] * z % c.p, P[1] * z % c.p, z)


def good_records(c, rng, n):
    """random z, Z = 1, a shared z, and Z = 0 records with arbitrary X, Y < p — (0 : 1 : 0) and (0 : 0 : 0) among them —
    interleaved, so that identities and Z = 1 sit inside every lane's product chain"""
    G = pyec.G(c)
    P, recs = G, []
    shared = rng.randrange(2, c.p)
    for i in range(n):
        P = pyec.add(c, P, G) if i % 5 else pyec.mul(c, rng.randrange(1, c.n), G)
        kind = i % 7
        if kind == 0:
            recs.append(enc_xyz(c, rng.randrange(c.p), rng.randrange(c.p), 0))
        elif kind == 1:
            recs.append(rescale(c, P, 1))
        elif kind == 2:
            recs.append(rescale(c, P, shared))
        elif kind == 3 and i % 2:
            recs.append(enc_xyz(c, 0, 1, 0))
        elif kind == 3:
            recs.append(enc_xyz(c, 0, 0, 0))
        else:
            recs.append(rescale(c, P, rng.randrange(1, c.p)))
    return recs


def bad_records(c, rng):
    """the records of test_gpu_xyz_ct.bad_records, plus Z = 0 with Y >= p"""
    P = pyec.mul(c, rng.randrange(1, c.n), pyec.G(c))
    z = rng.randrange(1, c.p)
    X, Y, Z = P[0] * z % c.p, P[1] * z % c.p, z
    return [enc_xyz(c, X, (Y + 1) % c.p, Z), enc_xyz(c, c.p, Y, Z), enc_xyz(c, X, c.p, Z), enc_xyz(c, X, Y, c.p),
            enc_xyz(c, c.p + 1, 0, 0), enc_xyz(c, 0, c.p, 0), enc_xyz(c, 0, 0, 1)]


@pytest.mark.parametrize("name", sorted(pyec.CURVES))
@pytest.mark.parametrize("n,nthreads", [(61, 0), (61, 8), (200, 7), (64, 64), (129, 1)])
def test_lane_body_matches_to_affine(hx, name, n, nthreads):
    """The conversion's output records equal the oracle's `to_affine` of each record, for record counts that are not a multiple
    of the lane stride and lanes of one to tens of records."""
    c = pyec.CURVES[name]
    rng = random.Random(0x7A + 31 * c.cid + n + nthreads)
    xyz = b"".join(good_records(c, rng, n))
    aff, ainf = oracle_lib.batch_normalize(c.cid, np.frombuffer(xyz, np.uint8))
    got, ginf, ok = convert(hx, c, xyz, nthreads)
    assert ok.all()
    assert bytes(got) == bytes(aff) and bytes(ginf) == bytes(ainf)


@pytest.mark.parametrize("name", sorted(pyec.CURVES))
def test_lane_body_verdicts(hx, name):
    """Each bad record, alone inside a run of good ones, is the one flagged; the good records around it convert as before."""
    c = pyec.CURVES[name]
    rng = random.Random(0xBAD1 + c.cid)
    good = good_records(c, rng, 40)
    for bad in bad_records(c, rng):
        j = rng.randrange(len(good))
        recs = good[:j] + [bad] + good[j + 1:]
        _, _, ok = convert(hx, c, b"".join(recs), 6)
        assert list(np.nonzero(ok == 0)[0]) == [j], (name, bad.hex())


def test_rescale_helper_matches_python(hx):
    """The GPU tests' compiled record generator (hx_rescale): (x z : y z : z) with z in [2, p), identities as (0 : z : 0)."""
    for name in ("k256", "p224", "p521", "bign256"):
        c = pyec.CURVES[name]
        rng = random.Random(c.cid)
        pts = [pyec.mul(c, rng.randrange(1, c.n), pyec.G(c)) for _ in range(20)] + [None]
        xy = b"".join(pyec.enc_point(c, P)[0] for P in pts)
        inf = bytes(P is None for P in pts)
        a, f = np.frombuffer(xy, np.uint8).copy(), np.frombuffer(inf, np.uint8).copy()
        out = np.zeros(len(pts) * 3 * c.L, np.uint8)
        assert hx.hx_rescale(c.cid, a.ctypes.data_as(_u8p), f.ctypes.data_as(_u8p), ctypes.c_size_t(len(pts)), ctypes.c_uint64(5), 0,
                             out.ctypes.data_as(_u8p)) == 0
        back, binf = oracle_lib.batch_normalize(c.cid, out)
        assert bytes(back) == bytes(a) and bytes(binf) == bytes(f)
        zs = {bytes(out[(3 * i + 2) * c.L:(3 * i + 3) * c.L]) for i in range(len(pts) - 1)}
        assert len(zs) == len(pts) - 1 and int.from_bytes(min(zs), c.order) > 1
