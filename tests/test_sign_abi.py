"""The ABI surface of the signing entry points, checked without a GPU: the header's declarations, the exported symbols, the
ctypes listing and the Engine methods, the generated Rust declarations and the safe wrappers that call them."""
import importlib
import os
import re
import sys

import pytest

import abi_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["ecgpu_ecdsa_sign_batch", "ecgpu_ecdsa_sign_rfc6979_batch", "ecgpu_ecdsa_sign_msg_batch", "ecgpu_schnorr_sign_raw_batch"]
NEW = HOST + [n + "_dev" for n in HOST]


@pytest.fixture(scope="module")
def mod():
    sys.path.insert(0, ROOT)
    return importlib.import_module("elliptic-curves_amd")


def test_header_declares_the_signing_entry_points():
    decls = {name: (ret, args) for name, ret, args in abi_parse.parse_header(os.path.join(ROOT, "include", "ecgpu.h"))}
    for name in NEW:
        assert name in decls, name
        ret, args = decls[name]
        assert ret == "int" and args[0][0] == "ecgpu_ctx *", name
        names = [a[1] for a in args]
        ptr = "const void *" if name.endswith("_dev") else "const uint8_t *"
        out = "void *" if name.endswith("_dev") else "uint8_t *"
        assert [t for t, a in args if "sig" in a] == [out] and [t for t, a in args if a.endswith("ok")] == [out], (name, args)
        if "ecdsa" in name:
            assert names[1] == "curve" and "normalize_s" in names and [t for t, a in args if "recid" in a] == [out], (name, args)
            assert args[2][0] == ptr
        else:
            assert "curve" not in names and any("aux" in a for a in names), (name, args)
        if "_msg_" in name or "schnorr" in name:
            assert "msg_len" in names


def test_library_exports_the_signing_entry_points(mod):
    lib = mod.load_library()
    for name in NEW + ["ecgpu_testhook_rfc6979_max_candidates"]:
        assert hasattr(lib, name), name


def test_bindings_list_the_signing_entry_points(mod):
    for name in NEW:
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("ecdsa_sign", "ecdsa_sign_rfc6979", "ecdsa_sign_msg", "schnorr_sign_raw"):
        assert callable(getattr(mod.Engine, meth)) and callable(getattr(mod.Engine, meth + "_dev")), meth


def test_rust_declarations_and_wrappers():
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read()
    for fn, sym in (("batch_sign_prehash", "ecgpu_ecdsa_sign_rfc6979_batch"), ("batch_sign", "ecgpu_ecdsa_sign_msg_batch"),
                    ("batch_sign_prehashed_with_nonce", "ecgpu_ecdsa_sign_batch"), ("schnorr_batch_sign_raw", "ecgpu_schnorr_sign_raw_batch")):
        m = re.search(r"pub fn %s\b.*?\n    \}\n" % fn, shim, re.S)
        assert m and sym + "(" in m.group(0), fn


def test_refuses_without_a_context(mod):
    """no context, no work: the entry points return ECGPU_ERR_ARG instead of touching a device"""
    lib = mod.load_library()
    assert lib.ecgpu_ecdsa_sign_batch(None, 0, None, None, None, 0, 0, None, None, None) == mod.ERR_ARG
    assert lib.ecgpu_ecdsa_sign_rfc6979_batch_dev(None, 0, None, None, 0, 0, None, None, None) == mod.ERR_ARG
    assert lib.ecgpu_schnorr_sign_raw_batch(None, None, None, 0, None, 0, None, None) == mod.ERR_ARG
