"""-m gpu: the generator's comb table at the widths the library runs by default (tests/comb_vectors.py has the scalars and the
build's geometry).

Every case pins its width on an engine of its own, closed at its end (the table is shared per device and freed with its last
user: at most one wide table lives at a time), and asserts base_table_info()["window_bits"] after its first call.

  (a) comb_corner_scalars + edge_scalars at every width in use (16, 22, the widest), through mul_by_generator, its compressed form
      and mul_by_generator_and_mul_add; 5 / 15 / 17 for the brainpool-256 sets (COMB_NEEDS_CHECK's detour)
  (b) the structured entry sample with both signed forms against the oracle
  (c) EVERY reachable entry of a window by two identities computed on the device: sum_e P_e and sum_e e P_e for P_e = the output
      of mul_by_generator on e 2^(w j), against the oracle on one scalar each
  (d) one batch gives the same bytes at every width
  (e) every entry of the uniform-schedule generator LUTs, through mul_by_generator(constant_time=True) and ecdsa_sign
  (f) the adaptive steps 16 -> 22 -> widest, in processes of their own (tests/gpu_table_tiers_check.py)

All comparisons are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import comb_vectors as cv
import oracle_lib
import pyec
import sign_model as sm
from gpu_common import comb_corner_scalars, edge_scalars, ecgpu_module, rand_scalars

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EVERY_SET = cv.CURVES
ALL_WIDTHS_OF = ("k256", "p256", "p384", "p224", "p521", "bign256")         # section (c): the other six at 16 bits only
CASES = [(name, w) for name in EVERY_SET for w in cv.WIDTHS[name]]
DETOUR = [(name, w) for name in ("bp256", "bp256t1") for w in (5, 15, 17)]   # w (nwin - 1) = 255
SWEEP = [(name, w) for name, w in CASES if name in ALL_WIDTHS_OF or w == 16]
SWEEP_ALL_WINDOWS_UP_TO = 1 << 26                                            # reachable entries of a table swept window by window
BLOCK = 4096                                                                 # a failing range is bisected down to this many entries


@pytest.fixture
def eng():
    e = ecgpu_module().Engine(0)          # raises without the HIP extension / a gfx950 device: no fallback
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def pinned(eng, c, w):
    eng.set_base_window(c.cid, w)


def assert_width(eng, c, w):
    """after the case's first generator call: the table in use is the one the case is about"""
    info = eng.base_table_info(c.cid)
    assert info["window_bits"] == w, (c.name, w, info)
    half = 1 << (w - 1)
    assert info["bytes"] == half * cv.window_count(c, w) * 2 * cv.words(c) * 4, (c.name, w, info)
    print("%s: window_bits == %d asserted (%d bytes, built in %.1f ms)" % (c.name, w, info["bytes"], info["build_ms"]))


def rows(c, data, width=None):
    return np.asarray(data, np.uint8).reshape(-1, width or 2 * c.L)


def first_bad(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return (int(bad[0]), int(bad.size)) if bad.size else None


# ---- (a) -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve,w", CASES + DETOUR)
def test_corner_scalars_at_the_widths_in_use(eng, curve, w):
    c = pyec.CURVES[curve]
    pinned(eng, c, w)
    ks = comb_corner_scalars(c, w) + edge_scalars(c)
    n = len(ks)
    scal = cv.enc(c, ks)
    want, winf = oracle_lib.batch_mul_base(c.cid, scal)
    out, inf = eng.mul_by_generator(c.cid, scal)
    assert_width(eng, c, w)
    assert first_bad(rows(c, out), rows(c, want)) is None and bytes(inf) == bytes(winf), (curve, w, first_bad(rows(c, out), rows(c, want)))
    # the compressed form: x and the SEC1 tag by the parity of y, 0 for the identity
    x, tag = eng.mul_by_generator_compressed(c.cid, scal)
    W = rows(c, want)
    ylow = W[:, c.L] if c.le else W[:, 2 * c.L - 1]
    assert bytes(x) == bytes(np.ascontiguousarray(W[:, : c.L])), (curve, w)
    assert bytes(tag) == bytes(np.where(winf == 1, 0, 2 + (ylow & 1)).astype(np.uint8)), (curve, w)
    # as the `a` of a G + b Q: b = 0, and b = 1 with Q = -G (the result is (a - 1) G)
    negG = pyec.enc_point(c, pyec.neg(c, pyec.G(c)))[0] * n
    out, inf = eng.mul_by_generator_and_mul_add(c.cid, scal, bytes(n * c.L), negG)
    assert first_bad(rows(c, out), rows(c, want)) is None and bytes(inf) == bytes(winf), (curve, w, "b = 0")
    out, inf = eng.mul_by_generator_and_mul_add(c.cid, scal, cv.enc(c, [1] * n), negG)
    want1, winf1 = oracle_lib.batch_mul_base(c.cid, cv.enc(c, [(k - 1) % c.n for k in ks]))
    assert first_bad(rows(c, out), rows(c, want1)) is None and bytes(inf) == bytes(winf1), (curve, w, "b = 1, Q = -G")
    assert eng.base_table_info(c.cid)["window_bits"] == w


# ---- (b) -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve,w", CASES)
def test_entry_sample_against_the_oracle(eng, curve, w):
    c = pyec.CURVES[curve]
    pinned(eng, c, w)
    vecs = cv.sample_vectors(c, w)
    scal = np.frombuffer(cv.enc(c, [v.k for v in vecs]), np.uint8)
    out, inf = eng.mul_by_generator(c.cid, scal)
    assert_width(eng, c, w)
    want, winf = oracle_lib.batch_mul_base_mt(c.cid, scal)
    bad = first_bad(rows(c, out), rows(c, want))
    if bad is None and (inf != winf).any():
        bad = (int(np.flatnonzero(inf != winf)[0]), int((inf != winf).sum()))
    if bad is not None:
        v = vecs[bad[0]]
        pytest.fail("%s w = %d: %d of %d vectors differ from the oracle, first: window %d, entry %d, form %s, k = %#x" % (
            curve, w, bad[1], len(vecs), v.j, v.e, v.form, v.k))


# ---- (c) -------------------------------------------------------------------------------------------------------------------------

def shifted_range(c, lo, hi, shift):
    """The scalars e * 2^shift, e = lo..hi, as an (hi - lo + 1, L) byte array in the set's wire order."""
    e = np.arange(lo, hi + 1, dtype=np.uint64)
    q, r = divmod(shift, 8)
    v = e << np.uint64(r)                                         # e < 2^26, r < 8
    a = np.zeros((e.size, c.L), np.uint8)                          # little-endian columns first
    for b in range(5):
        if q + b < c.L:
            a[:, q + b] = (v >> np.uint64(8 * b)) & np.uint64(0xFF)
        else:
            assert not (v >> np.uint64(8 * b)).any()
    return a if c.le else np.ascontiguousarray(a[:, ::-1])


def one_point(c, k):
    xy, inf = oracle_lib.batch_mul_base(c.cid, cv.enc(c, [k % c.n]))
    return bytes(xy), int(inf[0])


class Sweep:
    """The identities over e = lo..hi of one window, and the hunt for the entry behind a failure."""

    def __init__(self, eng, c, w, j):
        self.eng, self.c, self.w, self.j = eng, c, w, j

    def identities(self, lo, hi):
        """(sum identity holds, weighted identity holds) for the entries lo..hi of the window"""
        eng, c, sh = self.eng, self.c, self.w * self.j
        m = hi - lo + 1
        d_k = eng.to_device(shifted_range(c, lo, hi, sh).reshape(-1))
        d_p, d_f = eng.dev_alloc(m * 2 * c.L), eng.dev_alloc(max(m, 16))
        d_e = d_o = d_i = None
        try:
            eng.mul_by_generator_dev(c.cid, d_k, m, d_p, d_f)
            d_k.free()
            d_o, d_i = eng.dev_alloc(2 * c.L + 64), eng.dev_alloc(16)
            got = []
            eng.point_sum_dev(c.cid, d_p, d_f, m, d_o, d_i)
            got.append((bytes(eng.to_host(d_o, 2 * c.L)), int(eng.to_host(d_i, 1)[0])))
            d_e = eng.to_device(shifted_range(c, lo, hi, 0).reshape(-1))
            eng.lincomb_dev(c.cid, d_e, d_p, d_f, m, d_o, d_i)
            got.append((bytes(eng.to_host(d_o, 2 * c.L)), int(eng.to_host(d_i, 1)[0])))
        finally:
            for b in (d_k, d_p, d_f, d_e, d_o, d_i):
                if b is not None:
                    b.free()
        s1 = (hi * (hi + 1) - (lo - 1) * lo) // 2
        s2 = (hi * (hi + 1) * (2 * hi + 1) - (lo - 1) * lo * (2 * lo - 1)) // 6
        return got[0] == one_point(c, s1 << sh), got[1] == one_point(c, s2 << sh)

    def first_wrong_entry(self, lo, hi):
        """bisects a failing range with the same identities, then compares a block with the oracle: e, or None"""
        while hi - lo + 1 > BLOCK:
            mid = (lo + hi) // 2
            if not all(self.identities(lo, mid)):
                hi = mid
            elif not all(self.identities(mid + 1, hi)):
                lo = mid + 1
            else:
                return None
        scal = shifted_range(self.c, lo, hi, self.w * self.j).reshape(-1)
        out, inf = self.eng.mul_by_generator(self.c.cid, scal)
        want, winf = oracle_lib.batch_mul_base_mt(self.c.cid, scal)
        bad = first_bad(rows(self.c, out), rows(self.c, want))
        return None if bad is None else lo + bad[0]


def swept_windows(c, w):
    R = cv.reachable(c, w)
    live = [j for j, E in enumerate(R) if E]
    if sum(R) <= SWEEP_ALL_WINDOWS_UP_TO:
        return live
    full = [j for j in live if R[j] == 1 << (w - 1)]
    return sorted({0, full[-1], live[-1]})                       # window 0, the last full window, the top window


@pytest.mark.parametrize("curve,w", SWEEP)
def test_every_reachable_entry_by_device_identities(eng, curve, w):
    c = pyec.CURVES[curve]
    pinned(eng, c, w)
    R = cv.reachable(c, w)
    windows = swept_windows(c, w)
    if (curve, w) == ("k256", 26):
        # window 8 is where the word offset (window * half + index) * 2 N reaches 2^32
        assert windows == [0, 8, 9] and 8 * (1 << 25) * 16 == 1 << 32
    first = True
    for j in windows:
        sweep = Sweep(eng, c, w, j)
        ok_sum, ok_weighted = sweep.identities(1, R[j])
        if first:
            assert_width(eng, c, w)
            first = False
        if ok_sum and ok_weighted:
            continue
        e = sweep.first_wrong_entry(1, R[j])
        where = "entry %s" % e if e is not None else "no single entry found by bisection"
        if ok_sum:
            pytest.fail("%s w = %d window %d: sum_e e P_e differs while sum_e P_e holds (%s) — a lone failure of the weighted "
                        "identity points at the MSM (lincomb_dev), not at the table" % (curve, w, j, where))
        pytest.fail("%s w = %d window %d: sum_e P_e over e = 1..%d differs from the oracle (weighted identity %s): %s" % (
            curve, w, j, R[j], "holds" if ok_weighted else "differs too", where))
    print("%s w = %d: every reachable entry of windows %s" % (curve, w, windows))


# ---- (d) -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", EVERY_SET)
def test_results_do_not_depend_on_the_width(curve):
    c = pyec.CURVES[curve]
    n = (1 << 16) + 37
    head = [k for w in cv.WIDTHS[curve] for k in comb_corner_scalars(c, w)]
    scal = rand_scalars(c.cid, n, 0xC03BD000 + c.cid).copy()
    scal[: len(head) * c.L] = np.frombuffer(cv.enc(c, head), np.uint8)
    assert len(head) < n
    results = []
    for w in cv.WIDTHS[curve]:
        eng = ecgpu_module().Engine(0)
        try:
            pinned(eng, c, w)
            out, inf = eng.mul_by_generator(c.cid, scal)
            assert_width(eng, c, w)
        finally:
            eng.close()
        results.append((bytes(out), bytes(inf)))
    assert all(r == results[0] for r in results[1:]), curve
    pick = np.arange(0, n, 16)
    want, winf = oracle_lib.batch_mul_base(c.cid, scal.reshape(n, c.L)[pick].reshape(-1))
    got = rows(c, np.frombuffer(results[0][0], np.uint8))[pick]
    assert first_bad(got, rows(c, want)) is None and bytes(np.frombuffer(results[0][1], np.uint8)[pick]) == bytes(winf), curve


# ---- (e) -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", EVERY_SET)
def test_every_entry_of_the_constant_time_luts(eng, curve):
    c = pyec.CURVES[curve]
    ks = cv.ct_lut_scalars(c)
    scal = cv.enc(c, ks)
    want, winf = oracle_lib.batch_mul_base(c.cid, scal)
    out, inf = eng.mul_by_generator(c.cid, scal, constant_time=True)
    bad = first_bad(rows(c, out), rows(c, want))
    assert bad is None and not inf.any() and not winf.any(), (curve, bad and hex(ks[bad[0]]))
    if curve not in sm.ECDSA_SETS:
        return
    # the same scalars as the caller's nonce: r = x(k G) mod n
    d, z = 0x1F2E3D4C5B6A7988 + c.cid, int.from_bytes(bytes(range(1, c.L + 1)), "big")
    W = rows(c, want)
    model = [sm.ecdsa_sign(c, d, k, z, False, R=(int.from_bytes(bytes(W[i, : c.L]), "big"), int.from_bytes(bytes(W[i, c.L:]), "big")))
             for i, k in enumerate(ks)]
    enc = lambda v: v.to_bytes(c.L, "big")
    sig, recid, ok = eng.ecdsa_sign(c.cid, enc(d) * len(ks), scal, enc(z) * len(ks), normalize_s=False)
    S = rows(c, sig)
    for i, (msig, mrecid, mok) in enumerate(model):
        assert int(ok[i]) == mok == 1 and bytes(S[i]) == msig and int(recid[i]) == mrecid, (curve, hex(ks[i]))
        assert int.from_bytes(bytes(S[i, : c.L]), "big") == int.from_bytes(bytes(W[i, : c.L]), "big") % c.n


# ---- (f) -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiers_oracle(tmp_path_factory):
    """the oracle's result for the walk's batch, computed once and shared by the child processes through a file"""
    import gpu_table_tiers_check as tiers
    path = str(tmp_path_factory.mktemp("tiers") / "want.npy")
    want, winf = oracle_lib.batch_mul_base_mt(tiers.CURVE.cid, tiers.batch())
    assert not winf[len(tiers.head()):].any()
    np.save(path, np.concatenate([want, winf]))
    return path


@pytest.mark.parametrize("mode", ["sync", "async", "second_context", "verifier"])
def test_adaptive_tiers_in_a_fresh_process(mode, tiers_oracle):
    """include/ecgpu.h "the generator (comb) tables and their footprint": a device walks 16 -> 22 -> 26 bits with the number of
    multiplications it has seen.  That count is per device and process, so each scenario runs once in a child process:
    tests/gpu_table_tiers_check.py."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_table_tiers_check.py"), mode, tiers_oracle],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-1500:])
