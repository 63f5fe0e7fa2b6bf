"""The ABI surface of the hash-to-curve entry points, checked without a GPU: the header's declarations, the exported symbols, the
ctypes listing and the Engine methods, the generated Rust declarations and the safe wrappers, the C++ host wrapper, the
translation-unit group of the Makefile, and the argument errors that need no device."""
import importlib
import os
import re
import sys

import pytest

import abi_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHING = ["ecgpu_hash_to_curve_batch", "ecgpu_encode_to_curve_batch", "ecgpu_hash_to_scalar_batch"]
NEW = HASHING + ["ecgpu_map_to_curve_batch"]
HOOK = {"ecgpu_selftest_h2c": ["ctx", "curve", "op", "in", "n", "out"]}


@pytest.fixture(scope="module")
def mod():
    sys.path.insert(0, ROOT)
    return importlib.import_module("elliptic-curves_amd")


def test_header_declares_the_entry_points():
    decls = {name: (ret, args) for name, ret, args in abi_parse.parse_header(os.path.join(ROOT, "include", "ecgpu.h"))}
    for name in NEW:
        assert name in decls, name
        ret, args = decls[name]
        assert ret == "int" and args[0][0] == "ecgpu_ctx *" and args[1] == ("int", "curve"), (name, args)
        names = [a[1] for a in args]
        assert args[2][0] == "const uint8_t *", (name, args)
        if name in HASHING:
            assert names[3:7] == ["msg_len", "n", "dst", "dst_len"], (name, names)
            assert args[5][0] == "const uint8_t *"                                   # one tag per call
        else:
            assert names[3:5] == ["per_point", "n"], (name, names)
        outs = [t for t, a in args if "out" in a]
        assert outs == ["uint8_t *"] * (1 if "scalar" in name else 2), (name, args)


def test_header_declares_the_self_test_hook():
    decls = {name: (ret, args) for name, ret, args in abi_parse.parse_header(os.path.join(ROOT, "include", "ecgpu.h"))}
    for name, want in HOOK.items():
        ret, args = decls[name]
        assert ret == "int" and args[0] == ("ecgpu_ctx *", "ctx"), (name, args)
        assert [a[1] for a in args] == want, (name, args)
        assert [a[0] for a in args[1:]] == ["int", "int", "const uint8_t *", "size_t", "uint8_t *"], (name, args)
    src = open(os.path.join(ROOT, "include", "ecgpu.h")).read()
    hook = src[src.index("Test infrastructure: one lane body of hash-to-curve"):src.index("int ecgpu_selftest_h2c(")]
    for word in ("h2c_reduce_field", "h2c_reduce_scalar", "H2cMap::sswu", "H2cMap::iso_k256", "A kernel of its own", "L = 48 bytes",
                 "72 (ECGPU_P384)", "xn || xd || y", "X || Y || Z", "(0 : 1 : 0)", "ECGPU_K256 only", "ECGPU_ERR_ARG: unknown op",
                 "ECGPU_P521 included", "n = 0 succeeds and touches nothing", "tests/hostcheck_h2c"):
        assert word in hook, word


def test_the_hook_is_a_kernel_of_its_own_beside_the_map():
    hdr = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_h2c.h")).read()
    assert hdr.index("k_h2c_map(") < hdr.index("k_selftest_h2c(")
    body = hdr[hdr.index("k_selftest_h2c("):]
    for word in ("h2c_reduce_field<C>(", "h2c_reduce_scalar<C>(", "M::sswu(", "M::iso_k256("):
        assert word in body, word
    tu = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_inst_h2c.hip")).read()
    assert "k_selftest_h2c<CurveT>" in tu
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`ecgpu_selftest_h2c`" in integ


def test_header_states_scope_departure_and_secrecy():
    src = open(os.path.join(ROOT, "include", "ecgpu.h")).read()
    block = src[src.index("Batch hash-to-curve (RFC 9380)"):src.index("int ecgpu_hash_to_curve_batch(")]
    for word in ("SCOPE", "ECGPU_P521 included, returns ECGPU_ERR_CURVE", "ONE DEPARTURE", "invert().unwrap()", "SECRECY",
                 "H2C-OVERSIZE-DST-", "secp256k1_XMD:SHA-256_SSWU_RO_", "P256_XMD:SHA-256_SSWU_RO_", "P384_XMD:SHA-384_SSWU_RO_"):
        assert word in block, word


def test_library_exports_the_entry_points(mod):
    lib = mod.load_library()
    for name in NEW + sorted(HOOK):
        assert hasattr(lib, name), name


def test_bindings_list_the_entry_points(mod):
    for name in NEW + sorted(HOOK):
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("hash_to_curve", "encode_to_curve", "hash_to_scalar", "map_to_curve", "selftest_h2c"):
        assert callable(getattr(mod.Engine, meth)), meth
    assert (mod.H2C_ST_REDUCE_P, mod.H2C_ST_REDUCE_N, mod.H2C_ST_SSWU, mod.H2C_ST_ISO) == (0, 1, 2, 3)
    assert mod.H2C_DRAW_BYTES == {mod.K256: 48, mod.P256: 48, mod.P384: 72}


def test_rust_declarations_and_wrappers():
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW + sorted(HOOK):
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read()
    for fn, sym in (("batch_hash_from_bytes", "ecgpu_hash_to_curve_batch"), ("batch_encode_from_bytes", "ecgpu_encode_to_curve_batch"),
                    ("batch_hash_to_scalar", "ecgpu_hash_to_scalar_batch")):
        m = re.search(r"pub fn %s\b.*?\n    \}\n" % fn, shim, re.S)
        assert m and sym + "(" in m.group(0), fn


def test_cpp_wrapper_and_build_group():
    hpp = open(os.path.join(ROOT, "elliptic-curves_amd", "host", "ecgpu.hpp")).read()
    assert "hash_from_bytes(" in hpp and "encode_from_bytes(" in hpp
    assert "ecgpu_hash_to_curve_batch" in hpp and "ecgpu_encode_to_curve_batch" in hpp
    mk = open(os.path.join(ROOT, "elliptic-curves_amd", "Makefile")).read()
    groups = re.search(r"^GROUPS := (.*)$", mk, re.M).group(1).split()
    assert "h2c" in groups
    assert os.path.exists(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_inst_h2c.hip"))


def test_refuses_without_a_context(mod):
    """no context, no work: the entry points return ECGPU_ERR_ARG instead of touching a device"""
    lib = mod.load_library()
    assert lib.ecgpu_hash_to_curve_batch(None, 0, None, 0, 0, b"x", 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_encode_to_curve_batch(None, 1, None, 0, 0, b"x", 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_hash_to_scalar_batch(None, 2, None, 0, 0, b"x", 1, None) == mod.ERR_ARG
    assert lib.ecgpu_map_to_curve_batch(None, 0, None, 1, 0, None, None) == mod.ERR_ARG
    assert lib.ecgpu_selftest_h2c(None, 0, 0, None, 1, None) == mod.ERR_ARG
    assert lib.ecgpu_selftest_h2c(None, 0, 0, None, 0, None) == mod.ERR_ARG              # also for n = 0
