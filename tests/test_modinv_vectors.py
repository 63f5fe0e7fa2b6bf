"""The adversarial inversion inputs of tests/modinv_vectors.py (families L, T, S; both moduli of all twelve parameter sets) through
tools/modinv_model.py — the statement-level model of csrc/ecgpu_modinv.h, which asserts every interval the header states — and through
the g++ twin of the device code: tests/hostcheck ops 4, 17, scalar op 1 and the raw-domain ops 46 and 47, on the plain build and on
the -DECGPU_BOUNDS_CHECK build, where ecgpu_modinv.h traps on the same intervals; and once through a stand-alone program built with
AddressSanitizer + UBSan.  Expected values are Python integers (pow(x, -1, m)); equality is exact.
tests/test_gpu_modinv_vectors.py runs the same vectors on gfx950.

What the model shows and these tests pin (none of it a fault):
  * in the branch-free form d >= 0 always enters normalize: every input runs at least one batch on g = 0, and such a batch (u = 2^30,
    md = 2^30 for d < 0) adds p to a negative d.  The first pass's `cond_add` and the second pass of normalize work for invert_var
    only, which normalises right after the batch that brought g to 0 — ops 17 and 47, and on the device the lanes that finish last.
  * the documented intervals hold: d, e in (-2p, p) (the search reaches -1.50 p), |md| < 2^31 (1.61e9 reached), accumulators
    below 2^62."""
import fcntl
import os
import random
import subprocess

import numpy as np
import pytest

import hostcheck_lib as hc
import modinv_vectors as mv
import pyec
from test_field_adversarial import twin                                      # noqa: F401  (the plain / bounds fixture)

mm = mv.mm
HERE = os.path.dirname(os.path.abspath(__file__))
SAN_SRC = os.path.join(HERE, "hostcheck_modinv", "hostcheck_modinv.cpp")
SAN_PROG = os.path.join(HERE, "hostcheck_modinv", "hostcheck_modinv_san")
MODULI_IDS = ["%s-%s" % m for m in mv.MODULI]


def test_model_states_the_headers_constants():
    mm.check_header_constants()


def _pad(xs, wave=64):
    return xs + [xs[i % len(xs)] for i in range(-len(xs) % wave)]


@pytest.mark.parametrize("name,which", mv.MODULI, ids=MODULI_IDS)
def test_model_on_every_vector(name, which):
    """Both forms of the model against pow(x, -1, m) with every assertion of the model on; the matrices and zeta of the branch-free
    form must not depend on the upper halves of the 64-bit pairs; the variable form as a wave of 64 (a lane that is done goes on
    with its wave and keeps its value) and lane by lane."""
    m = mv.modulus(name, which)
    xs = _pad(mv.all_vectors(name, which))
    res, tr, _ = mm.garbage_identity(xs, m, seed=mv.seed(name, which, 7))
    assert not tr.dneg.any(), "a negative d enters normalize in the branch-free form: the module docstring says it cannot"
    assert tr.batches.max() < mm.BATCHES[mv.nw(name)]
    rv, trv = mm.invert_var(xs, m, wave=64)
    assert rv == res
    assert (trv.took.reshape(-1, 64) == trv.took.reshape(-1, 64).max(axis=1, keepdims=True)).all()      # a wave leaves as one
    assert (trv.took > trv.batches).any(), "no lane waited for its wave"
    # the earliest and the latest beside each other
    order = np.argsort(trv.batches, kind="stable")
    mixed = [xs[j] for j in list(order[:32]) + list(order[-32:])]
    r1, t1 = mm.invert_var(mixed, m, wave=64)
    r2, _ = mm.invert_var(mixed, m, wave=1)
    assert r1 == r2 and t1.took.min() == t1.batches.max()


@pytest.mark.parametrize("name,which", mv.MODULI, ids=MODULI_IDS)
def test_family_s_reaches_its_extremes_and_beats_random_inputs(name, which):
    mv.check_coverage(name, which)


def test_search_reproduces_the_constants_of_one_modulus():
    """tools/modinv_search.py on the smallest modulus (the whole search takes minutes: `python tools/modinv_search.py --check`)"""
    import modinv_search
    _, _, got = modinv_search.search(("p192", "p"))
    assert got == mv.s_constants("p192", "p")


def test_family_sizes():
    """a refactoring must not thin the families silently"""
    for name, which in mv.MODULI:
        nl = mm.NLIMBS[mv.nw(name)]
        m = mv.modulus(name, which)
        L = mv.family_l(name, which)
        assert len(L) >= 2 * m.bit_length() + 250, (name, which, len(L))
        assert {1, 2, 64, m - 1, m - 2, (m + 1) // 2, 1 << 30, 1 << (30 * (nl - 2))} <= set(L)
        for k in range(1, nl - 1):
            assert any(v % (1 << (30 * k)) == 0 and v % (1 << (30 * k + 30)) for v in L), (name, which, k)
        for tz in range(1, 30):
            assert any(v % (1 << tz) == 0 and v % (1 << (tz + 1)) for v in L)
        assert len(mv.family_t(name, which)) >= 100 and len(mv.family_s(name, which)) >= 12
        assert all(0 <= v < m for v in mv.all_vectors(name, which))


# ---- the g++ twin -------------------------------------------------------------------------------------------------------------------

def _field(c, op, vals):
    return mv.dec(c, hc.field_op_batch(c.cid, op, mv.enc(c, vals)))


@pytest.mark.parametrize("name", mv.CURVES)
def test_raw_inversion_ops_are_what_f_inv_computes(twin, name):
    """ops 46 / 47 = pack(F::inv(unpack(w))): w^-1 (k256) or w^-1 R^2 (Montgomery) mod p, derived from F::inv in
    modinv_vectors.want_raw_inv — on random values first, below p and in the second representative."""
    c = pyec.CURVES[name]
    rng = random.Random("raw-inv-%d" % c.cid)
    lim = mv.raw_lim(name)
    ws = [rng.randrange(c.p) for _ in range(40)] + [rng.randrange(c.p, lim) for _ in range(40)] + [0, c.p, 1, c.p + 1, lim - 1]
    want = [mv.want_raw_inv(name, w) for w in ws]
    for op in (46, 47):
        msg = mv.first_mismatch(name, "op %d" % op, ws, _field(c, op, ws), want)
        assert msg is None, msg
    # the same through the canonical ops: F::inv(from_canonical(a)) -> to_canonical
    a = [mv.canonical_operand(name, w % c.p) for w in ws]
    assert _field(c, 4, a) == [pow(x, -1, c.p) if x else 0 for x in a]


@pytest.mark.parametrize("name", mv.CURVES)
def test_twin_field_inversions_on_every_vector(twin, name):
    """ops 4 and 17 on the canonical operand that hands each vector to ModInv::invert, ops 46 and 47 on the vector itself and on
    the vector + p where the raw limit allows (the second representative, p itself included)."""
    c = pyec.CURVES[name]
    xs = mv.all_vectors(name, "p")
    a = [mv.canonical_operand(name, v) for v in xs]
    want = [mv.want_field_inv(name, v) for v in xs]
    for op in (4, 17):
        msg = mv.first_mismatch(name, "op %d" % op, xs, _field(c, op, a), want)
        assert msg is None, msg
    lim = mv.raw_lim(name)
    ws = xs + [0, c.p] + [v + c.p for v in xs if v + c.p < lim]
    assert len(ws) >= len(xs) + 2 + 64                  # (k256: only what is below 2^256 - p)
    want = [mv.want_raw_inv(name, w) for w in ws]
    for op in (46, 47):
        msg = mv.first_mismatch(name, "op %d" % op, ws, _field(c, op, ws), want)
        assert msg is None, msg


@pytest.mark.parametrize("name", mv.CURVES)
def test_twin_scalar_inversion_on_every_vector(twin, name):
    c = pyec.CURVES[name]
    xs = mv.all_vectors(name, "n")
    got = mv.dec(c, hc.scalar_op_batch(c.cid, 1, mv.enc(c, xs)))
    msg = mv.first_mismatch(name, "scalar op 1", xs, got, [pow(x, -1, c.n) if x else 0 for x in xs])
    assert msg is None, msg


# ---- the stand-alone program under the sanitizers -----------------------------------------------------------------------------------

def _build_san():
    csrc = os.path.join(os.path.dirname(HERE), "elliptic-curves_amd", "csrc")
    deps = [SAN_SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    with open(SAN_PROG + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(SAN_PROG) or os.path.getmtime(SAN_PROG) < max(os.path.getmtime(d) for d in deps):
            tmp = SAN_PROG + ".tmp.%d" % os.getpid()
            # (the runtimes linked into the program itself: it needs no preload)
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=undefined,address",
                                   "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", tmp, SAN_SRC])
            os.replace(tmp, SAN_PROG)


def test_sanitized_standalone_program(tmp_path):
    """AddressSanitizer + UBSan (signed overflow, shifts, bounds of the limb arrays) on all five inversion entry points, once over
    families L, T and S of every modulus."""
    _build_san()
    lines, want = [], []
    for name in mv.CURVES:
        c = pyec.CURVES[name]

        def put(op, operand, result):
            lines.append("%d %d %s" % (c.cid, op, mv.enc(c, [operand]).hex()))
            want.append(mv.enc(c, [result]).hex())
        lim = mv.raw_lim(name)
        for v in mv.all_vectors(name, "p"):
            a = mv.canonical_operand(name, v)
            for op in (4, 17):
                put(op, a, mv.want_field_inv(name, v))
            for w in (v, v + c.p):
                if w < lim:
                    for op in (46, 47):
                        put(op, w, mv.want_raw_inv(name, w))
        for x in mv.all_vectors(name, "n"):
            put(1, x, pow(x, -1, c.n) if x else 0)
    path = tmp_path / "vectors.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([SAN_PROG, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), lines[bad[0]], got[bad[0]], want[bad[0]])
