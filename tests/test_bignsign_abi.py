"""The ABI surface of the bign signing entry points, checked without a GPU: the header's declarations and argument names, the
exported symbols, the ctypes listing and the Engine methods, the generated Rust declarations and the shim functions, the words the
header block must say, where the kernels live, and the argument error that needs no device."""
import importlib
import importlib.util
import os
import re
import sys

import pytest

import abi_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ecgpu.h")
HOST = {
    "ecgpu_bign_sign_batch": ["ctx", "d", "k", "h", "n", "out_sig", "ok"],
    "ecgpu_bign_sign_prehash_batch": ["ctx", "d", "h", "n", "out_sig", "ok"],
    "ecgpu_bign_sign_msg_batch": ["ctx", "d", "msgs", "msg_len", "n", "out_sig", "ok"],
}
HOOK = {"ecgpu_selftest_bign_genk": ["ctx", "d", "h", "bound", "n", "out_k", "out_rounds"]}
SIZES = ("n", "msg_len")
NEW = sorted(HOST)


@pytest.fixture(scope="module")
def mod():
    sys.path.insert(0, ROOT)
    return importlib.import_module("elliptic-curves_amd")


def test_header_declares_the_entry_points():
    decls = {name: (ret, args) for name, ret, args in abi_parse.parse_header(HEADER)}
    for name, want in list(HOST.items()) + list(HOOK.items()):
        ret, args = decls[name]
        assert ret == "int" and args[0] == ("ecgpu_ctx *", "ctx"), (name, args)
        assert [a[1] for a in args] == want, (name, args)                        # no curve argument: bign-curve256v1 only
        for t, a in args[1:]:
            assert t == ("size_t" if a in SIZES else "uint8_t *" if a.startswith("out_") or a == "ok" else "const uint8_t *"), (name, a, t)
    assert not [name for name in decls if "bign_sign" in name and name.endswith("_dev")]      # no public _dev name yet


def test_header_block_states_the_contract():
    """what the header must say: the form with the caller's nonce is ours, which value of the prehash goes where, the retry rule,
    t empty, what is refused, what stays out"""
    src = open(HEADER).read()
    block = src[src.index("batch bign signing (STB 34.101.45"):src.index("int ecgpu_bign_sign_batch(")]
    for word in ("THIS FORM IS OURS", "REDUCED mod q", "RAW 32 bytes", "The retry rule", "k_bign_genk_retry", "t empty",
                 "S0 = 0 or S1 = 0", "Out of scope: additional data t", "tools/ct_isa_check.py --unit bignsign"):
        assert word in block, word
    assert "bign" not in src[src.index("batch SM2DSA signing (GB/T 32918.2"):src.index("int ecgpu_sm2dsa_sign_batch(")].split("Out of scope")[1]
    hook = src[src.index("Test infrastructure: the nonce generator kernels of bign signing"):src.index("int ecgpu_selftest_bign_genk(")]
    assert "in place of q" in hook and "2^254" in hook
    fin = src[src.index("Test infrastructure: the finish kernels"):src.index("int ecgpu_selftest_sign_finish(")]
    assert "k_bign_sign_finish" in fin and "ECGPU_SIGN_SCHEME_BIGN = 4" in fin


def test_library_exports_the_entry_points(mod):
    lib = mod.load_library()
    for name in NEW + sorted(HOOK):
        assert hasattr(lib, name), name


def test_bindings_list_the_entry_points(mod):
    for name in NEW + sorted(HOOK):
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("bign_sign", "bign_sign_prehash", "bign_sign_msg", "selftest_bign_genk"):
        assert callable(getattr(mod.Engine, meth)), meth
    assert mod.SIGN_SCHEME_BIGN == 4


def test_rust_declarations_and_shim_functions():
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW + sorted(HOOK):
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read()
    for fn, sym in (("bign_sign_prehash_batch", "ecgpu_bign_sign_prehash_batch"), ("bign_sign_batch", "ecgpu_bign_sign_msg_batch")):
        m = re.search(r"pub fn %s\b.*?\n    \}\n" % fn, shim, re.S)
        assert m and sym + "(" in m.group(0) and "Zeroizing" in m.group(0), fn
    for text in (shim, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "bignp256/src/ecdsa/signing.rs:110-161,164-176" in text
        assert "bign_sign_prehash_batch" in text and "bign_sign_batch" in text


def test_kernels_live_in_the_signing_translation_unit():
    """no new Makefile group; the launchers are guarded by a trait of the new header, and the counts the SM2DSA and the SM2
    encryption ABI tests pin are what they were"""
    mk = open(os.path.join(ROOT, "elliptic-curves_amd", "Makefile")).read()
    assert re.search(r"^GROUPS := (.*)$", mk, re.M).group(1).split() == ["base", "var", "msm", "ct", "sign", "h2c"]
    inst = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_inst_sign.hip")).read()
    assert '#include "ecgpu_bignsign.h"' in inst and inst.count("BignSign<C>::value") == 3
    assert inst.count("Sm2Sign<C>::value") == 3 and "CURVE_BIGN256" not in inst
    for k in ("k_bign_genk", "k_bign_genk_retry", "k_bign_sign_s0", "k_bign_sign_finish"):
        assert k + "<C>" in inst, k
    hdr = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_bignsign.h")).read()
    for word in ("ECGPU_HD bool bign_sign_finish_words(", "ECGPU_HD bool bign_genk_first_words(", "struct BignSign", "Belt::CtSbox()",
                 "BignBound bound"):
        assert word in hdr, word
    belt = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_belt.h")).read()
    assert "struct CtSbox" in belt and "__builtin_amdgcn_perm" in belt
    api = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_api.hip")).read()
    assert "int bign_sign_dev(" in api and "ecgpu_bign_sign_batch_dev" not in api


def test_the_checker_lists_the_unit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("ct_isa_check", os.path.join(ROOT, "tools", "ct_isa_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tu, kernels = tool.UNITS["bignsign"]
    assert tu == "ecgpu_inst_sign.hip"
    assert [k.rstrip("I") for k in kernels.split(",")] == ["k_bign_genk", "k_bign_sign_finish", "k_sign_nonce_load"]


def test_documents_name_the_entry_points():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in HOST:
            assert name in text, (doc, name)
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "bign signing (its nonce is belt-based)" not in text and "and bign signing are out of scope" not in text
        assert "profiles/bignsign/rates.txt" in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "80 VALU instructions per G" in design and "v_perm_b32" in design        # the S-box network's counts, read off the ISA
    mkf = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert "bign_sign: bign_sign.c" in mkf


def test_refuses_without_a_context(mod):
    """no context, no work: the entry points return ECGPU_ERR_ARG instead of touching a device"""
    lib = mod.load_library()
    assert lib.ecgpu_bign_sign_batch(None, None, None, None, 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_bign_sign_prehash_batch(None, None, None, 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_bign_sign_msg_batch(None, None, None, 0, 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_selftest_bign_genk(None, None, None, None, 1, None, None) == mod.ERR_ARG
