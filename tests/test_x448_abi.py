"""The ABI surface of the X448 entry points, checked without a GPU: the header's declarations and argument names, the exported
symbols, the ctypes listing and the Engine methods, the generated Rust declarations and the shim functions, the words the header
block must say, where the kernels live, and the argument error that needs no device."""
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
    "ecgpu_x448_batch": ["ctx", "scalars", "points_u", "n", "out_u", "ok"],
    "ecgpu_x448_unchecked_batch": ["ctx", "scalars", "points_u", "n", "out_u"],
    "ecgpu_x448_base_batch": ["ctx", "scalars", "n", "out_u"],
}
HOOK = {"ecgpu_selftest_fe448": ["ctx", "op", "a", "b", "n", "out"]}
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
        assert [a[1] for a in args] == want, (name, args)                        # no curve argument
        for t, a in args[1:]:
            want_t = "size_t" if a == "n" else "int" if a == "op" else "uint8_t *" if a.startswith("out") or a == "ok" else "const uint8_t *"
            assert t == want_t, (name, a, t)
    assert not [name for name in decls if "x448" in name and name.endswith("_dev")]           # no public _dev name yet
    src = open(HEADER).read()
    assert "ECGPU_X448" not in src and "ECGPU_CURVE448" not in src                            # and no id in the curve enum


def test_header_block_states_the_contract():
    src = open(HEADER).read()
    block = src[src.index("batch X448 (RFC 7748)"):src.index("int ecgpu_x448_batch(")]
    for word in ("The clamp", "bytes[0] &= 252", "bytes[55] |= 128", "never reduced modulo the group order", "There is no unclamped form",
                 "The low-order rule is byte-wise", "LOW_A (0), LOW_B (1), LOW_C (p - 1)", "p (= 0) and p + 1 (= 1) are NOT refused",
                 "the zero record", "NOT an error", "u in [p, 2^448) is legal input", "Secrecy", "tools/ct_isa_check.py --unit x448",
                 "ecgpu_wipe", "n = 0 succeeds and touches nothing", "NULL array with n > 0 is ECGPU_ERR_ARG",
                 "Host-pointer forms only, no `_dev` name yet", "x448/src/lib.rs:122-126", "lib.rs:152-156", "lib.rs:159-163", "lib.rs:25-31",
                 "no `curve` argument"):
        assert word in block, word
    hook = src[src.index("Test infrastructure: one op of the Goldilocks field"):src.index("int ecgpu_selftest_fe448(")]
    for word in ("RAW limbs", "16 little-endian 32-bit words", "mul_small(a, 39082)", "canon", "invert", "from_bytes -> to_bytes"):
        assert word in hook, word


def test_library_exports_the_entry_points(mod):
    lib = mod.load_library()
    for name in NEW + sorted(HOOK):
        assert hasattr(lib, name), name


def test_bindings_list_the_entry_points(mod):
    for name in NEW + sorted(HOOK):
        assert name in mod.ABI_SYMBOLS, name
    for meth in ("x448", "x448_unchecked", "x448_public_keys", "selftest_fe448"):
        assert callable(getattr(mod.Engine, meth)), meth
    assert mod.X448_BYTES == 56 and (mod.FE448_MUL, mod.FE448_BYTES) == (0, 8)
    assert len(mod.FIELD_BYTES) == 12                                             # the curve table is what it was


def test_rust_declarations_and_shim_functions():
    rs = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_sys.rs")).read()
    for name in NEW + sorted(HOOK):
        assert re.search(r"pub fn %s\(" % name, rs), name
    shim = open(os.path.join(ROOT, "elliptic-curves_amd", "rust", "ecgpu_shim.rs")).read()
    for fn, sym in (("x448_batch", "ecgpu_x448_batch"), ("x448_unchecked_batch", "ecgpu_x448_unchecked_batch"),
                    ("x448_public_keys_batch", "ecgpu_x448_base_batch")):
        m = re.search(r"pub fn %s\b.*?\n    \}\n" % fn, shim, re.S)
        assert m and sym + "(" in m.group(0) and "Zeroizing" in m.group(0), fn
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for site in ("x448::x448", "EphemeralSecret::diffie_hellman", "From<&EphemeralSecret> for PublicKey"):
        assert site in integ, site
    for fn in ("x448_batch", "x448_unchecked_batch", "x448_public_keys_batch"):
        assert fn in integ, fn


def test_kernels_live_in_a_translation_unit_of_their_own():
    mk = open(os.path.join(ROOT, "elliptic-curves_amd", "Makefile")).read()
    assert re.search(r"^GROUPS := (.*)$", mk, re.M).group(1).split() == ["base", "var", "msm", "ct", "sign", "h2c"]
    assert re.search(r"^OBJS := .*\$\(OBJDIR\)/x448\.o", mk, re.M) and re.search(r"^INST_OBJS := .*\$\(OBJDIR\)/x448\.o", mk, re.M)
    assert re.search(r"^\$\(OBJDIR\)/x448\.o: csrc/ecgpu_x448\.hip\n(.*\n)*?.*-Rpass-analysis=kernel-resource-usage.*x448\.log", mk, re.M)
    tu = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_x448.hip")).read()
    assert '#include "ecgpu_x448.h"' in tu and "ECGPU_CURVE" not in tu
    for mode in ("X448_CHECKED", "X448_UNCHECKED", "X448_BASE"):
        assert "k_x448_ladder<%s>" % mode in tu, mode
    hdr = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_x448.h")).read()
    for word in ("ECGPU_HD uint32_t x448_lane_words(", "ECGPU_HD void x448_step(", "ECGPU_HD uint32_t x448_low_order_words(",
                 "#pragma unroll 1", "cswap(m, x0.U, x1.U)"):
        assert word in hdr, word
    fe = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_fe448.h")).read()
    for word in ("static_assert(A * B <= 4", "ECGPU_BOUNDS_CHECK", "ECGPU_HD Gf1 invert(", "ECGPU_HD Gf1 canon("):
        assert word in fe, word
    assert "ecgpu_modinv.h" not in fe and "ecgpu_field.h" not in fe and "Field<" not in fe
    api = open(os.path.join(ROOT, "elliptic-curves_amd", "csrc", "ecgpu_api.hip")).read()
    assert "int x448_dev(" in api and "ecgpu_x448_batch_dev" not in api


def test_the_checker_lists_the_unit():
    spec = importlib.util.spec_from_file_location("ct_isa_check", os.path.join(ROOT, "tools", "ct_isa_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.UNITS["x448"] == ("ecgpu_x448.hip", "k_x448_ladder")


def test_documents_name_the_entry_points():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in HOST:
            assert name in text, (doc, name)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ct_isa_check.py --unit x448" in readme and "examples/x448_dh.c" in readme and "ecgpu_fe448.h" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ecgpu_fe448.h" in design and "38" in design and "2^448 - 2^224 - 1" in design
    survey = open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "X448 in; Ed448 / Decaf448 not yet" in survey
    mkf = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert "x448_dh: x448_dh.c" in mkf
    ignore = open(os.path.join(ROOT, ".gitignore")).read()
    assert "tests/hostcheck_x448/hostcheck_x448_san" in ignore and "examples/x448_dh" in ignore


def test_refuses_without_a_context(mod):
    """no context, no work: the entry points return ECGPU_ERR_ARG instead of touching a device"""
    lib = mod.load_library()
    assert lib.ecgpu_x448_batch(None, None, None, 1, None, None) == mod.ERR_ARG
    assert lib.ecgpu_x448_unchecked_batch(None, None, None, 1, None) == mod.ERR_ARG
    assert lib.ecgpu_x448_base_batch(None, None, 1, None) == mod.ERR_ARG
    assert lib.ecgpu_selftest_fe448(None, 0, None, None, 1, None) == mod.ERR_ARG
    assert lib.ecgpu_x448_batch(None, None, None, 0, None, None) == mod.ERR_ARG          # also for n = 0
