"""Batch X448 on gfx950 (csrc/ecgpu_x448.h), byte for byte against tests/x448_model.py: the reference's vectors through the three
calls, the first 100 values of the iterated vector, batch sizes around the wave and the block, the low-order verdicts and the
aliases inside a batch, scalar patterns that show a missing clamp, DH agreement, edge arguments, the wipe and the C example.

A lane owns exactly one record (k_x448_ladder: element i is lane i, 64 lanes per block), so there is no record chain inside a lane
to plant specials in; the sizes 63 / 64 / 65 and 255 / 256 / 257 are the wave's and four blocks' edges."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import x448_model as m
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
ERR_ARG = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "x448.json")))
SIZES = [1, 2, 63, 64, 65, 255, 256, 257]
SPOTS = [0, 63, 64, 255, 256]
NREF = 257


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


def rand_rec(rng):
    return bytes(rng.getrandbits(8) for _ in range(56))


@pytest.fixture(scope="module")
def ref():
    """NREF random (scalar, point) pairs and the model's answers, computed once and never changed"""
    rng = random.Random("gpu-x448-ref")
    ks, us = [rand_rec(rng) for _ in range(NREF)], [rand_rec(rng) for _ in range(NREF)]
    return {"ks": ks, "us": us, "dh": [m.x448_unchecked(k, u) for k, u in zip(ks, us)], "pub": [m.public_key(k) for k in ks]}


def cut(arr, n):
    b = bytes(arr)
    return [b[56 * i:56 * i + 56] for i in range(n)]


def three(eng, ks, us):
    """-> (checked records, ok, unchecked records, base records)"""
    n = len(ks)
    out, ok = eng.x448(b"".join(ks), b"".join(us))
    return cut(out, n), list(ok), cut(eng.x448_unchecked(b"".join(ks), b"".join(us)), n), cut(eng.x448_public_keys(b"".join(ks)), n)


def test_the_references_vectors_through_the_three_calls(eng):
    ab = {k: bytes.fromhex(v) for k, v in VEC["alice_bob"].items()}
    ks = [bytes.fromhex(v["scalar"]) for v in VEC["fixed"]] + [ab["alice_private"], ab["bob_private"]]
    us = [bytes.fromhex(v["point"]) for v in VEC["fixed"]] + [ab["bob_public"], ab["alice_public"]]
    want = [bytes.fromhex(v["expected"]) for v in VEC["fixed"]] + [ab["shared"], ab["shared"]]
    chk, ok, unc, pub = three(eng, ks, us)
    assert chk == want and ok == [1] * 4 and unc == want
    assert pub[2:] == [ab["alice_public"], ab["bob_public"]] and pub[:2] == [m.public_key(k) for k in ks[:2]]
    five = bytes.fromhex(VEC["iterated"]["start"])
    assert three(eng, [five], [five])[0] == [bytes.fromhex(VEC["iterated"]["after_1"])]
    for rec in VEC["low_order"]:
        chk, ok, unc, _ = three(eng, [ab["alice_private"]], [bytes.fromhex(rec)])
        assert (chk, ok, unc) == ([m.ZERO], [0], [m.ZERO])


def test_the_first_hundred_values_of_the_iterated_vector(eng):
    """n = 1 calls, each against the model's chain value (the 1,000th value is pinned on the CPU: tests/test_hostcheck_x448.py)"""
    k = u = bytes.fromhex(VEC["iterated"]["start"])
    for i in range(100):
        want, ok = m.x448(k, u)
        out, gok = eng.x448(k, u)
        assert (bytes(out), int(gok[0])) == (want, ok == 1 and 1), i
        k, u = want, k
        if i == 0:
            assert want == bytes.fromhex(VEC["iterated"]["after_1"])


@pytest.mark.parametrize("order", ["forwards", "reversed"])
@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(eng, ref, n, order):
    idx = list(range(n)) if order == "forwards" else list(range(NREF - 1, NREF - 1 - n, -1))
    ks, us = [ref["ks"][i] for i in idx], [ref["us"][i] for i in idx]
    chk, ok, unc, pub = three(eng, ks, us)
    want = [ref["dh"][i] for i in idx]
    assert chk == want and ok == [1] * n and unc == want
    assert pub == [ref["pub"][i] for i in idx]


@pytest.mark.parametrize("shift", range(7))
def test_verdicts_inside_a_batch(eng, ref, shift):
    """the three low-order records, the aliases p and p + 1, a twist point and 2^448 - 1 at elements 0, 63, 64, 255, 256 between
    random neighbours; every kind visits every spot over the seven shifts"""
    rng = random.Random("gpu-x448-verdicts")
    kinds = [("0", m.SPECIAL_U["0"]), ("1", m.SPECIAL_U["1"]), ("p-1", m.SPECIAL_U["p-1"]), ("p", m.SPECIAL_U["p"]),
             ("p+1", m.SPECIAL_U["p+1"]), ("twist", m.twist_u(rng)), ("2^448-1", m.SPECIAL_U["2^448-1"])]
    ks, us = list(ref["ks"]), list(ref["us"])
    want, want_ok, want_unc = list(ref["dh"]), [1] * NREF, list(ref["dh"])
    planted = {}
    for j, spot in enumerate(SPOTS):
        name, u = kinds[(j + shift) % 7]
        planted[spot] = name
        us[spot] = u
        rec, ok = m.x448(ks[spot], u)
        want[spot], want_ok[spot], want_unc[spot] = rec, ok, m.x448_unchecked(ks[spot], u)
        assert ok == (0 if name in ("0", "1", "p-1") else 1)
        assert (want_unc[spot] == m.ZERO) == (name in m.ZERO_PRODUCT), name       # the five zero-product inputs, and only they
        if name == "2^448-1":
            assert rec == m.x448_unchecked(ks[spot], m.SPECIAL_U["2^224"]) != m.ZERO
    chk, ok, unc, _ = three(eng, ks, us)
    assert ok == want_ok, planted                                                  # ok is exact
    assert chk == want, planted                                                    # refused elements: zero records; neighbours untouched
    assert unc == want_unc, planted


def scalar_patterns():
    out = [("all-zero", bytes(56)), ("all-ones", b"\xff" * 56), ("0x55", b"\x55" * 56), ("0xaa", b"\xaa" * 56)]
    for bit in (0, 1, 2, 31, 32, 223, 224, 446, 447):
        out.append(("bit %d" % bit, (1 << bit).to_bytes(56, "little")))
    for lo, hi in ((0, 31), (0, 63), (31, 32), (32, 63), (28, 35), (223, 224), (192, 255), (416, 447), (440, 447), (2, 446)):
        out.append(("run %d..%d" % (lo, hi), (((1 << (hi + 1)) - 1) ^ ((1 << lo) - 1)).to_bytes(56, "little")))
    return out


def test_scalar_patterns_before_the_clamp(eng, ref):
    pats = scalar_patterns()
    ks = [k for _, k in pats]
    us = [ref["us"][i] for i in range(len(ks))]
    chk, ok, unc, pub = three(eng, ks, us)
    for i, (label, k) in enumerate(pats):
        assert chk[i] == m.x448_unchecked(k, us[i]) == unc[i], label
        assert pub[i] == m.public_key(k), label
    assert ok == [1] * len(ks)
    # what a clamp that is not applied would give differs from the model on these (the model without its clamp)
    raw = m.le(m.ladder(int.from_bytes(b"\xff" * 56, "little") >> 1 << 1, 5))
    assert raw != m.public_key(b"\xff" * 56) and m.ladder(0, 5) == 0 != int.from_bytes(m.public_key(bytes(56)), "little")


def test_dh_agreement(eng):
    rng = random.Random("gpu-x448-dh")
    n = 64
    a, b = [rand_rec(rng) for _ in range(n)], [rand_rec(rng) for _ in range(n)]
    pa, pb = eng.x448_public_keys(b"".join(a)), eng.x448_public_keys(b"".join(b))
    sa, oka = eng.x448(b"".join(a), pb)
    sb, okb = eng.x448(b"".join(b), pa)
    assert bytes(sa) == bytes(sb) and list(oka) == list(okb) == [1] * n
    for i in (0, 31, 63):
        assert cut(sa, n)[i] == m.x448(a[i], m.public_key(b[i]))[0] != m.ZERO


def test_edge_arguments(eng):
    mod = ecgpu_module()
    lib = eng._lib
    buf = np.full(64, 0xEE, np.uint8)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    one, zero = ctypes.c_size_t(1), ctypes.c_size_t(0)
    assert lib.ecgpu_x448_batch(eng._ctx, p, p, zero, p, p) == 0 and lib.ecgpu_x448_batch(eng._ctx, None, None, zero, None, None) == 0
    assert lib.ecgpu_x448_unchecked_batch(eng._ctx, None, None, zero, None) == 0 and lib.ecgpu_x448_base_batch(eng._ctx, None, zero, p) == 0
    assert bytes(buf) == b"\xee" * 64                                          # n = 0 touches nothing
    for args in ((None, p, one, p, p), (p, None, one, p, p), (p, p, one, None, p), (p, p, one, p, None)):
        assert lib.ecgpu_x448_batch(eng._ctx, *args) == ERR_ARG
    for args in ((None, p, one, p), (p, None, one, p), (p, p, one, None)):
        assert lib.ecgpu_x448_unchecked_batch(eng._ctx, *args) == ERR_ARG
    assert lib.ecgpu_x448_base_batch(eng._ctx, None, one, p) == ERR_ARG and lib.ecgpu_x448_base_batch(eng._ctx, p, one, None) == ERR_ARG
    out, ok = eng.x448(b"", b"")
    assert out.size == 0 and ok.size == 0 and eng.x448_unchecked(b"", b"").size == 0 and eng.x448_public_keys(b"").size == 0
    with pytest.raises(mod.EcgpuError):
        eng.x448(bytes(56), bytes(55))
    with pytest.raises(mod.EcgpuError):
        eng.x448_public_keys(bytes(57))
    # the generic entry points know no thirteenth curve
    assert lib.ecgpu_field_bytes(12) == 0


def test_wipe(eng, ref):
    """the staged scalars and the staged results read back zero behind each call and after ecgpu_wipe, through the library's
    read-back hook (which a variable-time call, which wipes nothing, must show as not zero)"""
    mod = ecgpu_module()
    e = mod.Engine(0)
    try:
        hook = e._lib.ecgpu_testhook_wiped_scratch_nonzero
        hook.restype = ctypes.c_longlong
        n = NREF
        ks, us = b"".join(ref["ks"]), b"".join(ref["us"])
        e.mul_by_generator(mod.K256, bytes(31) + b"\x05")
        assert hook(e._ctx) > 0
        e.wipe()
        assert hook(e._ctx) == 0
        out, ok = e.x448(ks, us)
        assert cut(out, n) == ref["dh"] and hook(e._ctx) == 0
        assert cut(e.x448_unchecked(ks, us), n) == ref["dh"] and hook(e._ctx) == 0
        assert cut(e.x448_public_keys(ks), n) == ref["pub"] and hook(e._ctx) == 0
        e.wipe()
        assert hook(e._ctx) == 0
    finally:
        e.close()


def test_c_x448_dh_example_runs():
    """examples/x448_dh.c: the Alice / Bob exchange of RFC 7748 section 6.2 from plain C, and a refused low-order point"""
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["make", "-s", "-C", ex, "x448_dh"])
    out = subprocess.run([os.path.join(ex, "x448_dh")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": yes") == 4 and "NO" not in out.stdout
    assert VEC["alice_bob"]["shared"] in out.stdout
