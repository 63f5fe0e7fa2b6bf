"""The vectors of tests/sign_vectors.py ("s chosen first") against everything that runs without a GPU.

The models check themselves: every construction lands on the value it names, every ok signature verifies under tests/pyec.py with
Q = d G, and sign_model.ecdsa_sign / sm2sign_model.sign give the construction's record.  Then the g++ twins of the finish steps
(tests/hostcheck_sign, tests/hostcheck_sm2sign) run every family — the plain build and the -DECGPU_BOUNDS_CHECK build, where
ecgpu_modinv.h traps on its stated intervals — with normalize_s 0 and 1, and one stand-alone program per twin runs the vectors under
AddressSanitizer + UBSan as a child process (nothing sanitised is loaded into Python).  The coverage test holds the list of what the
generator could not build to exactly the expected one.  tests/test_gpu_sign_vectors.py runs the same vectors on gfx950;
profiles/sign_vectors/mutations.txt records which statements of the finish code these tests hold in place."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np
import pytest

import pyec
import sign_model as sm
import sign_vectors as sv
import sm2sign_model
import test_hostcheck_sign as ths
import test_hostcheck_sm2sign as ths2

BOUNDS_LIB = os.path.join(ths.HERE, "libhostcheck_sign_bounds.so")
SAN_PROG = os.path.join(ths.HERE, "hostcheck_sign_san")
_u8p = ctypes.POINTER(ctypes.c_uint8)
_bounds = None


def _build(target, flags):
    deps = [ths.SRC] + [os.path.join(ths.CSRC, f) for f in os.listdir(ths.CSRC) if f.endswith(".h")]

    def fresh():
        return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)
    with open(target + ".lock", "w") as lock:               # pytest-xdist workers arrive together: one builds, the others wait
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not fresh():
            tmp = target + ".tmp.%d" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + flags + ["-o", tmp, ths.SRC])
            os.replace(tmp, target)


def bounds_lib():
    global _bounds
    if _bounds is None:
        _build(BOUNDS_LIB, ["-O2", "-fPIC", "-shared", "-DECGPU_BOUNDS_CHECK"])
        _bounds = ctypes.CDLL(BOUNDS_LIB)
    return _bounds


def enc(c, values):
    return b"".join(int(v).to_bytes(c.L, "big") for v in values)


def twin_ecdsa(lib, c, ds, ks, flags, zs, Rs, rinfs, normalize_s):
    """hs_ecdsa_sign_finish of `lib` on the stages given -> [(sig, recid, ok)]"""
    n = len(ds)
    args = [ths._a(v) for v in (enc(c, ds), enc(c, ks), bytes(flags), enc(c, zs), enc(c, [v for R in Rs for v in R]), bytes(rinfs))]
    sig, recid, ok = np.full(n * 2 * c.L, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data_as(_u8p)
    assert lib.hs_ecdsa_sign_finish(c.cid, *[p(a) for a in args], ctypes.c_size_t(n), int(normalize_s), p(sig), p(recid), p(ok)) == 0
    return [(bytes(sig[2 * c.L * i:2 * c.L * (i + 1)]), int(recid[i]), int(ok[i])) for i in range(n)]


def twin_ecdsa_vectors(lib, name, vec, normalize_s, oracle):
    """the twin on entry-point vectors: the nonce as k_sign_nonce_load hands it on (1 and a cleared flag for an unusable one)"""
    c = pyec.CURVES[name]
    pts = sv.Points(c, oracle)
    ok_k = [1 <= v.k < c.n for v in vec]
    ks = [v.k if g else 1 for v, g in zip(vec, ok_k)]
    pts.prefetch(ks)
    return twin_ecdsa(lib, c, [v.d for v in vec], ks, [int(g) for g in ok_k], [v.z for v in vec], [pts(k) for k in ks], [0] * len(vec), normalize_s)


def twin_schnorr(vec):
    n = len(vec)
    msg_len = len(vec[0].msg)
    assert all(len(v.msg) == msg_len for v in vec)
    c = pyec.K256
    dp, k, flag, rxy, rinf, M = (ths._a(b) for b in (
        b"".join(enc(c, [v.d, v.px]) for v in vec), enc(c, [v.k for v in vec]), bytes(v.flag for v in vec),
        b"".join(enc(c, [v.x, v.y]) for v in vec), bytes(v.r_inf for v in vec), b"".join(v.msg for v in vec)))
    sig, ok = np.full(64 * n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    p = ths._p
    assert ths.lib().hs_schnorr_sign_finish(p(dp), p(k), p(flag), p(rxy), p(rinf), p(M), ctypes.c_size_t(msg_len), ctypes.c_size_t(n), p(sig), p(ok)) == 0
    return [(bytes(sig[64 * i:64 * i + 64]), int(ok[i])) for i in range(n)]


def schnorr_by_length(vec):
    groups = {}
    for v in vec:
        groups.setdefault(len(v.msg), []).append(v)
    return groups


# ---- the models check themselves ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_constructions_land_and_verify(oracle, name):
    c = pyec.CURVES[name]
    n = c.n
    vec, missing, _ = sv.ecdsa_vectors(name, oracle)
    pts = sv.Points(c, oracle)
    pts.prefetch([v.k for v in vec] + [v.d for v in vec])
    W = 1 << (32 * sv.words(c))
    enc_q = lambda vs: b"".join(enc(c, pts(v.d)) for v in vs)
    for normalize_s in (0, 1):                                                                  # every record under the oracle's verifier ...
        want = sv.ecdsa_expected(name, vec, normalize_s, oracle)
        r, s = (b"".join(w[0][i * c.L:(i + 1) * c.L] for w in want) for i in (0, 1))
        ver = oracle.ecdsa_verify(c.cid, enc(c, [v.z % n for v in vec]), r, s, enc_q(vec), bool(normalize_s))
        assert [int(x) for x in ver] == [w[2] for w in want], (name, normalize_s)
    slow_ones = sv.thin([v for v in vec if v.family in ("S+n", "A", "Z") or (v.family == "S" and "operand" not in v.label)], 24)
    for v in vec:
        R = pts(v.k)
        r = R[0] % n
        kinv = pow(v.k, -1, n)
        assert 1 <= v.d < n and 1 <= v.k < n and 0 <= v.z < 1 << (8 * c.L), (name, v.label)
        assert kinv * (v.z % n + r * v.d) % n == v.s, (name, v.family, v.label)                  # the definition gives the chosen s
        if v.family in ("S", "S+n"):
            assert v.s == v.target
        elif v.family == "A":
            assert v.z < n and v.z + r * v.d % n == v.target and v.target in (n - 1, n, n + 1, 2 * n - 2, W - 1, W, W + 1)
        elif v.family == "M":
            assert (kinv, (v.z + r * v.d) % n) == v.target                                      # both operands of the last product
        elif v.family == "I":
            assert v.k == v.target
        elif v.family == "Z":
            assert v.z == v.target and (v.z % n in (0, 1, 2, n - 1) or v.z == (1 << 528) - 1)
        for normalize_s in (0, 1):
            want = sv.expect_ecdsa(c, v.s, R, normalize_s)
            assert sm.ecdsa_sign(c, v.d, v.k, v.z, normalize_s, R=R) == want, (name, v.family, v.label)
            sig, recid, ok = want
            assert ok == (v.s != 0)
            # ... and two dozen of those with no shared list behind them under the big-integer model (forty milliseconds a call and more)
            slow = v in slow_ones
            if ok and slow and (normalize_s == 0 or want != sv.expect_ecdsa(c, v.s, R, 0)):
                rr, ss = int.from_bytes(sig[:c.L], "big"), int.from_bytes(sig[c.L:], "big")
                Q = pts(v.d)
                assert pyec.ecdsa_verify(c, Q, v.z % n, rr, ss, bool(normalize_s)), (name, v.family, v.label)
                if v.family == "S":
                    assert pyec.ecdsa_recover(c, v.z % n, rr, ss, recid, bool(normalize_s)) == Q, (name, v.family, v.label)
            elif not ok:
                assert want == (bytes(2 * c.L), 0, 0)
    # the two sides of the low-S boundary: the record changes on one side only
    by = {v.label: v for v in vec}
    lo, hi = by["s = (n - 1) / 2"], by["s = (n + 1) / 2"]
    assert sv.expect_ecdsa(c, lo.s, pts(lo.k), 1) == sv.expect_ecdsa(c, lo.s, pts(lo.k), 0)
    assert sv.expect_ecdsa(c, hi.s, pts(hi.k), 1)[:2] == (enc(c, [pts(hi.k)[0] % n, (n - 1) // 2]), sv.expect_ecdsa(c, hi.s, pts(hi.k), 0)[1] ^ 1)
    # a twin is its original's signature
    for v in vec:
        if v.family == "S+n":
            o = by[v.label.split(" | ")[0]]
            assert (o.d, o.k, o.s) == (v.d, v.k, v.s) and (v.z - o.z) % n == 0 and v.z > o.z


def test_coverage_and_what_could_not_be_built(oracle):
    for name in sm.ECDSA_SETS:
        c = pyec.CURVES[name]
        vec, missing, thinned = sv.ecdsa_vectors(name, oracle)
        cnt = sv.counts(vec)
        want_missing = []
        if name not in sv.TWIN_SETS:
            want_missing.append(("S+n", "z + n"))
        if name == "p521":
            want_missing += [("A", "z + r d = 2^(32 N) - 1"), ("A", "z + r d = 2^(32 N)"), ("A", "z + r d = 2^(32 N) + 1")]
        assert [(f, w) for f, w, _ in missing] == want_missing, (name, missing)
        for fam in sv.ECDSA_FAMILIES:
            empty_by_design = (fam == "Z" and name != "p521") or (fam == "S+n" and name not in sv.TWIN_SETS)
            assert (cnt[fam] == 0) == empty_by_design, (name, fam, cnt[fam])
        assert set(cnt) <= set(sv.ECDSA_FAMILIES)
        assert 400 <= len(vec) <= 600, (name, len(vec))                                         # a few hundred: a GPU test runs in seconds
        labels = [v.label for v in vec]
        named = [l for l, _ in sv.named_s_targets(c)]
        assert all(l in labels for l in named) and len(named) == (9 if name == "p521" else 12)
        assert cnt["A"] == (13 if name == "p521" else 25) and cnt["M"] == sv.CAP_PAIRS and cnt["I"] >= 180
        assert all(a == b or a >= 60 for a, b in thinned.values())
        if name == "p521":
            zl = [v.label for v in vec if v.family == "Z"]
            assert "z = 128 n +1" in zl and "z = 127 n +1" in zl and "z = 2^528 - 1" in zl and "z = 128 n +2, r d = n - 1" in zl and len(zl) == 19
            assert any("z + 127 n" in l for l in labels) and any("z + 2 n" in l for l in labels)
        good, fails, layouts = sv.position_batches(name)
        assert len(good) == sv.BATCH == 257 and len(fails) == 7 and len(layouts) == 7
        hv, hmiss = sv.hook_ecdsa(name)
        assert hmiss == [] and c.n < c.p                                                        # every set has an x in [n, p) to forge
        assert len(hv) == 4 * len(named) + 3
    vec, missing, _ = sv.sm2_vectors(oracle)
    cnt = sv.counts(vec)
    assert missing == [] and set(cnt) == set(sv.SM2_FAMILIES) and all(cnt[f] for f in sv.SM2_FAMILIES)
    assert {v.label for v in vec if not v.ok} >= {"s = 0", "k - r d = 0, k = k0", "r = n - k"}          # s = 0 twice over, r + k = 0
    assert len(sv.sm2_failures()) == 10 and len(sv.hook_schnorr()) == 26
    assert sv.report(oracle).count("\n") >= 2 * len(sm.ECDSA_SETS) + 3


def test_sm2_constructions_land_and_verify(oracle):
    c, n = pyec.SM2, pyec.SM2.n
    vec, _, _ = sv.sm2_vectors(oracle)
    pts = sv.Points(c, oracle)
    pts.prefetch([v.k for v in vec] + [v.d for v in vec])
    for v in vec:
        R = pts(v.k)
        assert 1 <= v.d < n - 1 and 1 <= v.k < n and 0 <= v.e < 2 ** 256
        assert (v.e + R[0]) % n == v.r                                                          # r as chosen
        inv, num = pow(1 + v.d, -1, n), (v.k - v.r * v.d) % n
        assert inv * num % n == v.s
        if v.family in ("S", "E+n"):
            assert v.target == (v.s if v.family == "S" else v.e)
        elif v.family == "M":
            assert (inv, num) == v.target
        elif v.family == "B":
            assert num == v.target
        elif v.family == "R":
            assert v.r == v.target
        want = sv.expect_sm2(v)
        assert sm2sign_model.sign(v.d, v.k, v.e, R=R) == want, (v.family, v.label)
        if v.ok and (v.family not in ("S", "M") or "operand" not in v.label and v.family == "S"):   # (forty milliseconds a call)
            assert pyec.sm2dsa_verify(c, pts(v.d), v.e % n, v.r, v.s), (v.family, v.label)
    e32 = lambda vals: b"".join(int(x).to_bytes(32, "big") for x in vals)
    ver = oracle.sm2dsa_verify(e32(v.e % n for v in vec), e32(v.r for v in vec), e32(v.s for v in vec), b"".join(enc(c, pts(v.d)) for v in vec))
    assert [int(x) for x in ver] == [int(v.ok) for v in vec]                                     # every record under the oracle's verifier
    fails = {v.label for v in vec if not v.ok}
    assert {"k - r d = 0, k = 1", "k - r d = 0, k = k0", "k - r d = 0, k = n - 1", "r = n - k", "s = 0"} <= fails
    assert all(v.ok == (v.s != 0 and (v.r + v.k) % n != 0 and v.r != 0) for v in vec)


def test_schnorr_hook_vectors_land():
    c, n = pyec.K256, pyec.K256.n
    vec = sv.hook_schnorr()
    seen = set()
    for v in vec:
        if v.target is None:
            continue
        e = sv.schnorr_challenge(v.x, v.px, v.msg)
        kp = n - v.k if v.y & 1 else v.k
        assert 1 <= v.k < n and kp + e * v.d % n == v.target and v.s == v.target % n
        seen.add((v.target, v.y & 1))
    assert len(seen) == 12 and sum(1 for v in vec if v.s == 0) == 4
    for v in vec:                                                                               # an ok record verifies: s G - e P = R needs a
        assert sv.expect_schnorr(v)[1] == int(v.s not in (None, 0))                             # real R, which a forged x is not: the model is the check


# ---- the g++ twins ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", ["plain", "bounds"])
@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_twin_on_every_family(oracle, name, build):
    lib = ths.lib() if build == "plain" else bounds_lib()
    vec, _, _ = sv.ecdsa_vectors(name, oracle)
    for normalize_s in (0, 1):
        got = twin_ecdsa_vectors(lib, name, vec, normalize_s, oracle)
        bad = sv.first_mismatch(name, "twin (%s), normalize_s = %d" % (build, normalize_s), vec, got, sv.ecdsa_expected(name, vec, normalize_s, oracle))
        assert bad is None, bad


@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_twin_positions(oracle, name):
    good, fails, layouts = sv.position_batches(name)
    for normalize_s in (0, 1):
        base = twin_ecdsa_vectors(ths.lib(), name, good, normalize_s, oracle)
        assert sv.first_mismatch(name, "neighbours", good, base, sv.ecdsa_expected(name, good, normalize_s, oracle)) is None
        zero = (bytes(2 * pyec.CURVES[name].L), 0, 0)
        for lay in layouts:
            batch = sv.placed(good, fails, lay)
            got = twin_ecdsa_vectors(ths.lib(), name, batch, normalize_s, oracle)
            want = list(base)
            for p, _ in lay:
                want[p] = zero
            bad = sv.first_mismatch(name, "positions %r, normalize_s = %d" % (lay, normalize_s), batch, got, want)
            assert bad is None, bad


@pytest.mark.parametrize("name", sm.ECDSA_SETS)
def test_ecdsa_twin_hook_vectors(name):
    c = pyec.CURVES[name]
    vec, _ = sv.hook_ecdsa(name)
    for lib in (ths.lib(), bounds_lib()):
        for normalize_s in (0, 1):
            got = twin_ecdsa(lib, c, [v.d for v in vec], [v.k for v in vec], [v.flag for v in vec], [v.z for v in vec], [(v.x, v.y) for v in vec],
                             [v.r_inf for v in vec], normalize_s)
            bad = sv.first_mismatch(name, "hook twin, normalize_s = %d" % normalize_s, vec, got, sv.hook_ecdsa_expected(name, vec, normalize_s))
            assert bad is None, bad
    # recid bit 1 and the flip together: a forged x >= n beside an s above the boundary
    want = {v.label: w for v, w in zip(vec, sv.hook_ecdsa_expected(name, vec, 1))}
    assert want["x = n + 1, s = (n + 1) / 2, y odd"][1:] == (2, 1) and want["x = n + 1, s = (n - 1) / 2, y even"][1:] == (2, 1)
    assert want["x = n - 1, s = n - 1, y odd"][1:] == (0, 1) and want["x = n, s = 1, y odd"] == (bytes(2 * c.L), 0, 0)


def test_sm2_twin_on_every_family(oracle):
    vec, _, _ = sv.sm2_vectors(oracle)
    pts = sv.Points(pyec.SM2, oracle)
    pts.prefetch([v.k for v in vec])
    got = ths2.twin_finish([(v.d, v.k, 1, v.e, pts(v.k)[0], 0) for v in vec])
    bad = sv.first_mismatch("sm2", "twin", vec, got, [sv.expect_sm2(v) for v in vec])
    assert bad is None, bad


def test_sm2_twin_positions_and_hook(oracle):
    good, fails, layouts = sv.sm2_position_batches()
    x_of = {}

    def rows(batch):
        out = []
        for v in batch:
            k = v.k if 1 <= v.k < pyec.SM2.n else 1
            if k not in x_of:
                x_of[k] = sm.mul_g(pyec.SM2, k)[0]
            out.append((v.d, k, int(k == v.k), v.e, x_of[k], 0))
        return out
    base = ths2.twin_finish(rows(good))
    assert sv.first_mismatch("sm2", "neighbours", good, base, [sv.expect_sm2(v) for v in good]) is None
    for lay in layouts:
        batch = sv.placed(good, fails, lay)
        want = list(base)
        for p, _ in lay:
            want[p] = sm2sign_model.ZERO
        bad = sv.first_mismatch("sm2", "positions %r" % (lay,), batch, ths2.twin_finish(rows(batch)), want)
        assert bad is None, bad
    hook = sv.hook_sm2()
    got = ths2.twin_finish([r for _, r in hook])
    for (label, r), g in zip(hook, got):
        assert g == sm2sign_model.finish(*r), label
    # r = e + x(R) mod n = 0 at (x, e) = (n, 0), (n + 1, n - 1) and (n - 1, 1): x is reduced once, then the sum
    assert [ok for _, ok in got] == [0, 1, 1, 1] + [1, 1, 0, 1] + [1, 1, 1, 1] + [1, 0, 1, 1] + [0, 0]


def test_schnorr_twin_hook_vectors():
    for msg_len, vec in sorted(schnorr_by_length(sv.hook_schnorr()).items()):
        bad = sv.first_mismatch("k256", "schnorr hook twin, msg_len = %d" % msg_len, vec, twin_schnorr(vec), [sv.expect_schnorr(v) for v in vec])
        assert bad is None, bad


# ---- the stand-alone programs under the sanitizers ------------------------------------------------------------------------------

def test_sanitized_standalone_program(oracle, tmp_path):
    """AddressSanitizer + UBSan on the ECDSA and BIP340 finish steps, every buffer exactly its record's size: the named targets, the
    sums, the twins, the p521 prehashes and every hook vector of every set (the operand, pair and nonce families on k256)"""
    # (the runtimes linked into the program itself: it needs no preload and does not mind what else the process environment loads)
    _build(SAN_PROG, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                      "-DHOSTCHECK_SIGN_MAIN"])
    lines, want = [], []
    hx = lambda c, *v: enc(c, v).hex()
    for name in sm.ECDSA_SETS:
        c = pyec.CURVES[name]
        vec, _, _ = sv.ecdsa_vectors(name, oracle)
        if name != "k256":
            vec = [v for v in vec if v.family in ("S+n", "A", "Z") or (v.family == "S" and "operand" not in v.label)]
        pts = sv.Points(c, oracle)
        pts.prefetch([v.k for v in vec])
        hv, _ = sv.hook_ecdsa(name)
        for normalize_s in (0, 1):
            for v, w in zip(vec, sv.ecdsa_expected(name, vec, normalize_s, oracle)):
                lines.append("E %d %d %s %s 1 %s %s 0" % (c.cid, normalize_s, hx(c, v.d), hx(c, v.k), hx(c, v.z), hx(c, *pts(v.k))))
                want.append(w)
            for v, w in zip(hv, sv.hook_ecdsa_expected(name, hv, normalize_s)):
                lines.append("E %d %d %s %s %d %s %s %d" % (c.cid, normalize_s, hx(c, v.d), hx(c, v.k), v.flag, hx(c, v.z), hx(c, v.x, v.y), v.r_inf))
                want.append(w)
    want = [" sig=%s recid=%02x ok=%02x" % (s.hex(), r, o) for s, r, o in want]
    c = pyec.K256
    for v in sv.hook_schnorr():
        lines.append("S %s %s %d %s %d %s" % (hx(c, v.d, v.px), hx(c, v.k), v.flag, hx(c, v.x, v.y), v.r_inf, v.msg.hex() or "-"))
        sig, ok = sv.expect_schnorr(v)
        want.append(" sig=%s ok=%02x" % (sig.hex(), ok))
    path = tmp_path / "rows.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([SAN_PROG, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, lines[i][:40])


def test_sm2_sanitized_standalone_program(oracle, tmp_path):
    """the SM2DSA vectors through the sanitised program tests/hostcheck_sm2sign already has"""
    ths2._build(ths2.PROG, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                            "-DHOSTCHECK_SM2SIGN_MAIN"])
    vec, _, _ = sv.sm2_vectors(oracle)
    pts = sv.Points(pyec.SM2, oracle)
    pts.prefetch([v.k for v in vec])
    rows = [(v.d, v.k, 1, v.e, pts(v.k)[0], 0) for v in vec] + [r for _, r in sv.hook_sm2()]
    want = [sv.expect_sm2(v) for v in vec] + [sm2sign_model.finish(*r) for _, r in sv.hook_sm2()]
    pa = pyec.enc_point(pyec.SM2, (pyec.SM2.gx, pyec.SM2.gy))[0].hex()
    path = tmp_path / "rows.txt"
    path.write_text("".join("%064x %064x %d %064x %064x %d - - %s\n" % (d, k, kf, e, x, ri, pa) for d, k, kf, e, x, ri in rows))
    r = subprocess.run([ths2.PROG, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, (sig, ok)) in enumerate(zip(got, want)):
        assert " sig=%s ok=%02x " % (sig.hex(), ok) in g, i
