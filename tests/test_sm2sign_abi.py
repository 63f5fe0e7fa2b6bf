"""The ABI surface of the SM2DSA signing entry points, checked without a GPU: the header's declarations and argument names, the
exported symbols, the ctypes listing and the Engine methods, the generated Rust declarations and the shim functions, the words the
header block must say, where the kernels live, and the argument error that needs no device."""
import importlib
import os
import re
import sys

import pytest

import abi_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ecgpu.h")
HOST = {
    "ecgpu_sm2dsa_sign_batch": ["ctx", "d", "k", "e", "n", "out_sig", "ok"],
    "ecgpu_sm2dsa_sign_rfc6979_batch": ["ctx", "d", "e", "n", "out_sig", "ok"],
    "ecgpu_sm2dsa_sign_msg_batch": ["ctx", "distid", "distid_len", "d", "msgs", "msg_len", "n", "out_sig", "ok"],
}
SIZES = ("n", "distid_len", "msg_len")
NEW = sorted(HOST)


@pytest.fixture(scope="module")
def mod():
    sys.path.insert(0, ROOT)
    return importlib.import_module("elliptic-curves_amd")


def test_header_declares_the_entry_points():
    decls = {name: (ret, args) for name, ret, args in abi_parse.parse_header(HEADER)}
    for name, want in HOST.items():
        ret, args = decls[name]
        assert ret == "int" and args[0] == ("ecgpu_ctx *", "ctx"), (name, args)
        assert [a[1] for a in args] == want, (name, args)                        # no curve argument: sm2 only
        for t, a in args[1:]:
            assert t == ("size_t" if a in SIZES else "uint8_t *" if a in ("out_sig", "ok") else "const uint8_t *"), (name, a, t)


def test_header_block_states_the_contract():
    """what the header must say: the form with the caller's nonce is ours, the one-candidate rule, the k = 0 difference, no recovery
    id, the randomized form out of scope"""
    src = open(HEADER).read()
    block = src[src.index("batch SM2DSA signing (GB/T 32918.2"):src.index("int ecgpu_sm2dsa_sign_batch(")]
    for word in ("THIS FORM IS OURS", "single `fill_next_k`", "k = 0 is refused", "no recovery id", "`RandomizedPrehashSigner`"):
        assert word in block, word


def test_library_exports_the_entry_points(mod):
    lib = mod.load_library()
    for name in NEW:
        assert hasattr(lib, name), name


def test_bindings_list_the_entry_points(mod):
    for name in NEW:
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("sm2dsa_sign", "sm2dsa_sign_rfc6979", "sm2dsa_sign_msg"):
        assert callable(getattr(mod.Engine, meth)), meth


def test_rust_declarations_and_shim_functions():
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read()
    for fn, sym in (("sm2dsa_sign_prehash_batch", "ecgpu_sm2dsa_sign_rfc6979_batch"), ("sm2dsa_sign_batch", "ecgpu_sm2dsa_sign_msg_batch")):
        m = re.search(r"pub fn %s\b.*?\n    \}\n" % fn, shim, re.S)
        assert m and sym + "(" in m.group(0) and "Zeroizing" in m.group(0), fn
    for text in (shim, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "sm2/src/dsa/signing.rs:122-126,162-174" in text
        assert "sm2dsa_sign_prehash_batch" in text and "sm2dsa_sign_batch" in text


def test_kernels_live_in_the_signing_translation_unit():
    """no new Makefile group; the launchers are guarded by a trait of the header, so that the curve comparison the encryption
    launchers are counted by stays theirs"""
    mk = open(os.path.join(ROOT, "elliptic-curves_amd", "Makefile")).read()
    assert re.search(r"^GROUPS := (.*)$", mk, re.M).group(1).split() == ["base", "var", "msm", "ct", "sign", "h2c"]
    inst = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_inst_sign.hip")).read()
    assert '#include "ecgpu_sm2sign.h"' in inst and inst.count("Sm2Sign<C>::value") == 3
    for k in ("k_sm2_sign_e", "k_sm2_rfc6979", "k_sm2dsa_sign_finish"):
        assert k + "<C>" in inst, k
    hdr = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_sm2sign.h")).read()
    assert "ECGPU_HD bool sm2dsa_sign_finish_words(" in hdr and "struct Sm2Sign" in hdr
    assert "k_rfc6979_retry" not in hdr                                           # one candidate: no retry kernel


def test_documents_name_the_entry_points():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in HOST:
            assert name in text, (doc, name)


def test_refuses_without_a_context(mod):
    """no context, no work: the entry points return ECGPU_ERR_ARG instead of touching a device"""
    lib = mod.load_library()
    assert lib.ecgpu_sm2dsa_sign_batch(None, None, None, None, 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_sm2dsa_sign_rfc6979_batch(None, None, None, 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_sm2dsa_sign_msg_batch(None, None, 0, None, None, 0, 1, None, None) == mod.ERR_ARG
