"""The ABI surface of the SM2 public-key encryption entry points, checked without a GPU: the header's declarations, the exported
symbols, the ctypes listing and the Engine methods, the generated Rust declarations and the shim functions, the words the header
block must say, that no device-pointer name leaked, and the argument error that needs no device."""
import importlib
import os
import re
import sys

import pytest

import abi_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ecgpu_sm2_pke_encrypt_batch", "ecgpu_sm2_pke_decrypt_batch"]
HEADER = os.path.join(ROOT, "include", "ecgpu.h")


@pytest.fixture(scope="module")
def mod():
    sys.path.insert(0, ROOT)
    return importlib.import_module("elliptic-curves_amd")


def test_header_declares_the_entry_points():
    decls = {name: (ret, args) for name, ret, args in abi_parse.parse_header(HEADER)}
    want = {
        "ecgpu_sm2_pke_encrypt_batch": ["ctx", "pk_xy", "k", "msgs", "msg_len", "n", "out_c1_xy", "out_c2", "out_c3", "ok"],
        "ecgpu_sm2_pke_decrypt_batch": ["ctx", "d", "c1_xy", "c2", "msg_len", "c3", "n", "out_msgs", "ok"],
    }
    for name in NEW:
        assert name in decls, name
        ret, args = decls[name]
        assert ret == "int" and args[0][0] == "ecgpu_ctx *", (name, args)
        assert [a[1] for a in args] == want[name], (name, args)                  # no curve argument: the feature is SM2 only
        for t, a in args[1:]:
            if a in ("msg_len", "n"):
                assert t == "size_t", (name, a, t)
            elif a.startswith("out_") or a == "ok":
                assert t == "uint8_t *", (name, a, t)
            else:
                assert t == "const uint8_t *", (name, a, t)


def test_no_device_pointer_name_leaked():
    names = [name for name, _, _ in abi_parse.parse_header(HEADER)]
    pke = [n for n in names if "ecgpu_sm2_pke" in n]
    assert sorted(pke) == sorted(NEW)
    assert not [n for n in pke if n.endswith("_dev")]
    src = open(HEADER).read()
    assert not re.search(r"ecgpu_sm2_pke\w*_dev\b", src)


def test_header_states_the_departure_and_the_secrecy_rule():
    src = open(HEADER).read()
    block = src[src.index("Batch SM2 public-key encryption and decryption"):src.index("int ecgpu_sm2_pke_encrypt_batch(")]
    for word in ("ONE DEPARTURE", "SECRECY", "msg_len == 0", "ECGPU_ERR_ARG", "0xFFFFFFFF", "C1C3C2", "Scalar::S", "not the identity",
                 "never ECGPU_ERR_POINT", "tools/ct_isa_check.py --unit pke", "host-pointer forms only"):
        assert word in block, word


def test_library_exports_the_entry_points(mod):
    lib = mod.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert not hasattr(lib, name + "_dev"), name


def test_bindings_list_the_entry_points(mod):
    for name in NEW:
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("sm2_pke_encrypt", "sm2_pke_decrypt"):
        assert callable(getattr(mod.Engine, meth)), meth


def test_rust_declarations_and_shim_functions():
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read()
    for fn, sym, words in (("sm2_pke_encrypt_batch", "ecgpu_sm2_pke_encrypt_batch", ("try_generate_from_rng", "Mode::C1C3C2", "Mode::C1C2C3")),
                           ("sm2_pke_decrypt_batch", "ecgpu_sm2_pke_decrypt_batch", ("Mode::C1C3C2", "Mode::C1C2C3"))):
        m = re.search(r"pub fn %s\b.*?\n    \}\n" % fn, shim, re.S)
        assert m and sym + "(" in m.group(0), fn
        for w in words:
            assert w in m.group(0), (fn, w)


def test_kernels_live_in_the_signing_translation_unit():
    """no new Makefile group: the kernels are instantiated from ecgpu_inst_sign.hip, guarded on the sm2 curve"""
    mk = open(os.path.join(ROOT, "elliptic-curves_amd", "Makefile")).read()
    assert re.search(r"^GROUPS := (.*)$", mk, re.M).group(1).split() == ["base", "var", "msm", "ct", "sign", "h2c"]
    inst = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_inst_sign.hip")).read()
    assert '#include "ecgpu_pke.h"' in inst and inst.count("C::ID == CURVE_SM2") == 3
    for k in ("k_pke_load", "k_pke_point", "k_pke_seal", "k_pke_open"):
        assert k + "<C>" in inst, k


def test_refuses_without_a_context(mod):
    """no context, no work: the entry points return ECGPU_ERR_ARG instead of touching a device"""
    lib = mod.load_library()
    assert lib.ecgpu_sm2_pke_encrypt_batch(None, None, None, None, 1, 0, None, None, None, None) == mod.ERR_ARG
    assert lib.ecgpu_sm2_pke_decrypt_batch(None, None, None, None, 0, None, 0, None, None) == mod.ERR_ARG
