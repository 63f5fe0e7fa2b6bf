"""Projective (X : Y : Z) inputs of the uniform-schedule entry points (ecgpu_batch_mul_ct_xyz, ecgpu_lincomb_ct_xyz), checked
without a GPU: the ABI surface (header, library, Python and Rust bindings), the ISA of the new kernel (k_xyz_mul_ct) under
tools/ct_isa_check.py, and its lane body compiled for the CPU (tests/hostcheck_xyz) against the oracle's `to_affine`
(ecref_batch_normalize) followed by the affine multiplication."""
import ctypes
import fcntl
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import pyec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "hostcheck_xyz")
SRC = os.path.join(HERE, "hostcheck_xyz.cpp")
LIB = os.path.join(HERE, "libhostcheck_xyz.so")
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")
NEW = ["ecgpu_batch_mul_ct_xyz", "ecgpu_batch_mul_ct_xyz_dev", "ecgpu_lincomb_ct_xyz", "ecgpu_lincomb_ct_xyz_dev"]
_u8p = ctypes.POINTER(ctypes.c_uint8)
CT_FLAG_BAD_SCALAR, CT_FLAG_BAD_POINT = 1, 2


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ---- the ABI surface ----------------------------------------------------------------------------------------------------

def test_header_declares_the_xyz_entry_points():
    src = _strip_comments(open(os.path.join(ROOT, "include", "ecgpu.h")).read())
    for name in NEW:
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, src)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 7 and "points_xyz" in args[3], (name, args)        # one point array, no identity flags


def test_bindings_list_the_xyz_entry_points():
    sys.path.insert(0, ROOT)
    import importlib
    mod = importlib.import_module("elliptic-curves_amd")
    for name in NEW:
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("mul_xyz", "lincomb_ct_xyz", "mul_xyz_dev", "lincomb_ct_xyz_dev"):
        assert callable(getattr(mod.Engine, meth)), meth
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = _strip_comments(open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read())
    assert "ecgpu_batch_mul_ct_xyz(" in shim and "ecgpu_lincomb_ct_xyz(" in shim
    assert "ecgpu_batch_mul_ct(" not in shim and "ecgpu_lincomb_ct(" not in shim      # the projective call sites ship X || Y || Z


def test_library_exports_the_xyz_entry_points():
    so = os.path.join(ROOT, "elliptic-curves_amd", "lib", "libecgpu.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    for name in NEW:
        assert hasattr(lib, name), name


# ---- the ISA of the new kernel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", ["K256Params", "P256Params", "P384Params", "Bign256Params"])
def test_xyz_kernel_has_no_branch_or_address_on_point_data(curve):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ct_isa_check.py"), "--curve", curve, "--kernels", "k_xyz_mul_ct"],
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("-> OK") == 1 and "k_xyz_mul_ct" in r.stdout, r.stdout


def test_xyz_record_codecs_move_whole_words():
    """k_xyz_mul_ct reads 3L-byte records (p521 198, p224 84, p192 72 bytes): tools/wire_codec_isa_check.py on the ct group."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wire_codec_isa_check.py"), "--curve", "P521Params", "--curve",
                        "P224Params", "--curve", "P192Params", "--groups", "ct"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    assert "k_xyz_mul_ct<ecgpu::P521Params>" in r.stdout and "halfword loads" in r.stdout      # the check saw the new kernel


def test_mul_xyz_refuses_the_variable_time_form_without_a_gpu():
    """There is no variable-time entry point for projective records: mul_xyz(constant_time=False) is an argument error, raised
    before the library is called."""
    sys.path.insert(0, ROOT)
    import importlib
    mod = importlib.import_module("elliptic-curves_amd")
    eng = mod.Engine.__new__(mod.Engine)                       # no device needed: the check comes first
    for call in (lambda: eng.mul_xyz(0, b"", b"", constant_time=False),
                 lambda: eng.mul_xyz_dev(0, None, None, 0, None, constant_time=False)):
        with pytest.raises(mod.EcgpuError) as e:
            call()
        assert e.value.code == mod.ERR_ARG


# ---- the lane body on the CPU -------------------------------------------------------------------------------------------

def _build():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("ecgpu_field.h", "ecgpu_params.h", "ecgpu_field_consts.h", "ecgpu_point.h",
                                                     "ecgpu_recode.h", "ecgpu_ctmul.h", "ecgpu_modinv.h", "ecgpu_scalar.h")]

    def fresh():
        return os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps)
    if fresh():
        return
    with open(LIB + ".lock", "w") as lock:             # (pytest-xdist workers: one builds, the others wait)
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            tmp = LIB + ".tmp.%d" % os.getpid()
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, LIB)


@pytest.fixture(scope="module")
def hx():
    _build()
    return ctypes.CDLL(LIB)


def _run(hx, c, mode, ks, xyz):
    n = len(ks)
    s = np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in ks), np.uint8).copy()
    p = np.frombuffer(xyz, np.uint8).copy()
    out, inf, flags = np.zeros(n * 2 * c.L, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    assert hx.hx_mul_ct_xyz(c.cid, mode, s.ctypes.data_as(_u8p), p.ctypes.data_as(_u8p), ctypes.c_size_t(n),
                            out.ctypes.data_as(_u8p), inf.ctypes.data_as(_u8p), flags.ctypes.data_as(_u8p)) == 0
    return out, inf, flags


def enc_xyz(c, X, Y, Z):
    return X.to_bytes(c.L, c.order) + Y.to_bytes(c.L, c.order) + Z.to_bytes(c.L, c.order)


def rescale(c, P, z):
    """(x z : y z : z) for a finite P, (0 : 1 : 0) scaled for the identity"""
    if P is None:
        return enc_xyz(c, 0, z % c.p, 0)
    return enc_xyz(c, P[0] * z % c.p, P[1] * z % c.p, z)


def cases(c, rng):
    """(scalar, record) pairs: random points under random z, z G and z (-G), Z = 0 records with arbitrary X, Y < p, and a
    stretch where every record carries the same z"""
    G = pyec.G(c)
    ks, recs = [], []
    for _ in range(3):
        P = pyec.mul(c, rng.randrange(1, c.n), G)
        ks.append(rng.randrange(c.n)); recs.append(rescale(c, P, rng.randrange(1, c.p)))
    ks += [rng.randrange(c.n), rng.randrange(c.n), 0, c.n - 1]
    recs += [rescale(c, G, rng.randrange(1, c.p)), rescale(c, pyec.neg(c, G), rng.randrange(1, c.p)),
             rescale(c, G, rng.randrange(1, c.p)), rescale(c, G, 1)]
    ks += [rng.randrange(c.n), 1]
    recs += [enc_xyz(c, rng.randrange(c.p), rng.randrange(c.p), 0), enc_xyz(c, 0, 0, 0)]
    z = rng.randrange(1, c.p)
    for P in (G, pyec.neg(c, G), pyec.add(c, G, G)):
        ks.append(rng.randrange(c.n)); recs.append(rescale(c, P, z))
    return ks, b"".join(recs)


@pytest.mark.parametrize("name", sorted(pyec.CURVES))
def test_lane_body_matches_to_affine_then_mul_ct(hx, name):
    c = pyec.CURVES[name]
    rng = random.Random(0x5A17 + c.cid)
    ks, xyz = cases(c, rng)
    n = len(ks)
    aff, ainf = oracle_lib.batch_normalize(c.cid, np.frombuffer(xyz, np.uint8))
    # the loader alone: the point each record stands for is its `to_affine`
    got, ginf, flags = _run(hx, c, 1, ks, xyz)
    assert bytes(flags) == bytes(n) and bytes(got) == bytes(aff) and bytes(ginf) == bytes(ainf)
    # the whole lane: k (X : Y : Z) = k to_affine(X : Y : Z), as the oracle's constant-time multiplication computes it
    scal = np.frombuffer(b"".join(pyec.enc_scalar(c, k) for k in ks), np.uint8)
    want, winf = oracle_lib.batch_mul(c.cid, scal, aff, ainf)
    got, ginf, flags = _run(hx, c, 0, ks, xyz)
    assert bytes(flags) == bytes(n) and bytes(got) == bytes(want) and bytes(ginf) == bytes(winf)


@pytest.mark.parametrize("name", ["k256", "p256", "p384", "p224", "p521", "bp256", "bign256"])
def test_lane_body_verdicts(hx, name):
    c = pyec.CURVES[name]
    rng = random.Random(0xBAD0 + c.cid)
    P = pyec.mul(c, rng.randrange(1, c.n), pyec.G(c))
    z = rng.randrange(1, c.p)
    X, Y, Z = P[0] * z % c.p, P[1] * z % c.p, z
    top = (1 << (8 * c.L)) - 1
    recs = [
        (enc_xyz(c, X, Y, Z), 0),
        (enc_xyz(c, X, (Y + 1) % c.p, Z), CT_FLAG_BAD_POINT),            # off the curve
        (enc_xyz(c, X + c.p if X + c.p <= top else c.p, Y, Z), CT_FLAG_BAD_POINT),   # X >= p
        (enc_xyz(c, X, c.p, Z), CT_FLAG_BAD_POINT),                      # Y >= p
        (enc_xyz(c, X, Y, c.p), CT_FLAG_BAD_POINT),                      # Z >= p (= 0 mod p: still out of range)
        (enc_xyz(c, c.p, 1, 0), CT_FLAG_BAD_POINT),                      # Z = 0 does not excuse X >= p
        (enc_xyz(c, rng.randrange(c.p), rng.randrange(c.p), 0), 0),      # the identity, whatever X, Y < p
        (enc_xyz(c, 0, 0, Z), CT_FLAG_BAD_POINT),                        # (0 : 0 : Z): b Z^3 != 0
    ]
    ks = [rng.randrange(c.n) for _ in recs]
    ks[0] = c.n                                                            # scalar >= n: its own flag bit
    _, _, flags = _run(hx, c, 0, ks, b"".join(r for r, _ in recs))
    assert list(flags) == [CT_FLAG_BAD_SCALAR] + [f for _, f in recs[1:]]
