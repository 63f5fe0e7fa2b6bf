#!/usr/bin/env python3
"""Model of csrc/ecgpu_modinv.h — ModInv<NW>, Bernstein-Yang division steps on signed 30-bit limbs — statement for statement, for
NW = 6, 7, 8, 12 and 17.

Every function below is the function of the same name in the header.  A "register" is one numpy array: the axis is the LANE, so one
call runs the statements on many inputs at once, the way a wave does, and invert_var's ballot is a reduction over groups of 64
neighbouring lanes.  Registers are modelled at their widths: the pairs of step_a / step_b are uint64 (products and sums wrap modulo
2^64, as v_mad_u64_u32 and the b64 shifts do), a value the header keeps in an int32_t is asserted to fit one wherever it is written,
and the accumulators of the matrix updates are shown to stay inside an int64_t at every multiply-add (Acc.settle).  What the header's comments claim is asserted
where they claim it:
  * the low 30 bits of cd, ce, cf, cg are zero before the first shift of an update;
  * the entries of a transition matrix lie in [-2^30, 2^30];
  * md, me fit an int32_t and every accumulator an int64_t;
  * d, e lie in (-2p, p) after every batch;
  * at the end g = 0 and f = +-1, the output lies in [0, p) with limbs in [0, 2^30) and equals pow(x, -1, p) (0 for x = 0 mod p).
The device form of a division step only ever reads the LOWER halves of its pairs (header, "Device: ..."): `garbage` re-draws the
upper halves of all six pairs before every step from a random generator, and the matrices and zeta must come out as they do with
the halves the arithmetic leaves there (garbage_identity).
invert_var: a lane whose g is 0 keeps taking batches until every lane of its wave is done (wave = 64) or stops on its own
(wave = 1: the host twin); the value it would return is taken when its g first becomes 0 and must equal what it returns at the end.

Each run returns a Trace (per lane): batches until g = 0 and division steps used, min / max of d / p and e / p, max |md| (and
|me|), the largest accumulator, whether a batch had |u| = 2^30 while g != 0, the signs of d and f entering normalize and whether
d < -p there, and for the variable form the iterations per batch, the set of `limit` values taken and the batches that swapped.

    python tools/modinv_model.py            (no GPU; a self-test on structured and random inputs for the five widths)
"""
import os
import re
import sys

import numpy as np

U64 = np.uint64
I64 = np.int64
M30 = (1 << 30) - 1
M32 = 0xFFFFFFFF

NLIMBS = {6: 7, 7: 8, 8: 9, 12: 13, 17: 19}
BATCHES = {6: 15, 7: 18, 8: 20, 12: 31, 17: 42}
MAXB_VAR = {6: 19, 7: 22, 8: 25, 12: 37, 17: 52}
LIMIT_CAP = 6                             # divsteps_30_var clears at most this many bits per addition (the mask `& 63u`)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "elliptic-curves_amd", "csrc", "ecgpu_modinv.h")


def check_header_constants(path=HEADER):
    """NL, BATCHES and MAXB_VAR as the header states them: a changed count cannot leave the model on the old one."""
    src = open(path).read()

    def table(name):
        line = re.search(r"ECGPU_CONST int %s = ([^;]*);" % name, src).group(1)
        pairs = re.findall(r"NW == (\d+) \? (\d+)", line)
        last = re.search(r": (\d+)\s*$", line).group(1)
        return dict([(int(k), int(v)) for k, v in pairs] + [(17, int(last))])
    assert table("NL") == NLIMBS, table("NL")
    assert table("BATCHES") == BATCHES, table("BATCHES")
    assert table("MAXB_VAR") == MAXB_VAR, table("MAXB_VAR")
    assert "& 63u;" in src and "eta + 1) > i ? i : (eta + 1)" in src


def nw_of(modulus):
    nw = (modulus.bit_length() + 31) // 32
    assert nw in NLIMBS, nw
    return nw


# ---- registers ------------------------------------------------------------------------------------------------------------------

def u32(x):
    """the low 32 bits of an int64 / uint64 register, as uint64"""
    return x.astype(U64) & U64(M32)


def s32(x):
    """(int32_t)(uint32_t)x: the low 32 bits of a uint64 register as a signed value (int64)"""
    return ((x & U64(M32)) ^ U64(1 << 31)).astype(I64) - I64(1 << 31)


def fits32(x, what):
    assert ((x >= -(1 << 31)) & (x < (1 << 31))).all(), "%s does not fit an int32_t: %s" % (what, x[(x < -(1 << 31)) | (x >= (1 << 31))][:4])
    return x


class Trace:
    def __init__(self, n, maxb):
        self.batches = np.zeros(n, I64)              # batches until g = 0 (0 for x = 0)
        self.steps = np.zeros(n, I64)                # division steps until g = 0: 30 per batch (the branch-free form counts whole batches)
        self.dmin = np.zeros(n)
        self.dmax = np.zeros(n)
        self.emin = np.zeros(n)
        self.emax = np.zeros(n)
        self.md = np.zeros(n, I64)                   # max |md|, |me|
        self.acc = np.zeros(n, I64)                  # largest accumulator magnitude
        self.full_u = np.zeros(n, bool)              # a batch had |u| = 2^30 while g != 0
        self.dneg = np.zeros(n, bool)                # entering normalize: d < 0, f < 0, d < -p
        self.fneg = np.zeros(n, bool)
        self.dlow = np.zeros(n, bool)
        self.iters = np.zeros((maxb, n), I64)        # variable form: loop iterations of each batch
        self.limits = np.zeros(n, I64)               # bit k set: limit = k was taken
        self.limits_batch = np.zeros((maxb, n), I64)
        self.swaps = np.zeros((maxb, n), bool)       # the swap branch was taken in this batch
        self.working = np.zeros((maxb, n), bool)     # g != 0 entering this batch

    def lane(self, i):
        return {k: (v[:, i] if v.ndim == 2 else v[i]) for k, v in self.__dict__.items()}


class Acc:
    """The int64_t accumulators: the largest magnitude after any multiply-add is kept per lane; settle() turns it into `none wrapped`."""

    def __init__(self, n, check=True):
        self.max = np.zeros(n, I64)
        self.check = check

    def mad(self, a, b, acc):
        """acc + a b on signed 32-bit factors (v_mad_i64_i32; smad, and each line of smad4 / smad6)"""
        s = acc + a * b                               # |a| <= 2^30, |b| < 2^31: the product is below 2^61 in magnitude
        if self.check:
            np.maximum(self.max, np.abs(s), out=self.max)
        return s

    def settle(self):
        """Once per batch.  Every factor pair is (matrix entry or limb of p, limb or md): a product below 2^61.  While every sum
        so far stayed below 2^62 the next one is below 2^62 + 2^61 < 2^63, so `all sums below 2^62` rules out that any of them
        wrapped: the first to wrap would have had to start from a sum of 2^62 or more."""
        assert int(self.max.max()) < (1 << 62), "an accumulator reaches 2^62: int64_t is no longer certain"


# ---- the header's functions -------------------------------------------------------------------------------------------------------

def to_limb_array(values, nw):
    """Python integers below 2^(32 NW) -> the uint32 words x[NW] of each lane, as a (NW, n) uint64 array"""
    w = np.zeros((nw, len(values)), U64)
    for j, x in enumerate(values):
        assert 0 <= x < (1 << (32 * nw)), hex(x)
        for i in range(nw):
            w[i, j] = (x >> (32 * i)) & M32
    return w


def from_words(w, nw):
    nl = NLIMBS[nw]
    r = np.zeros((nl, w.shape[1]), I64)
    for l in range(nl):
        bit = 30 * l
        i, sh = bit // 32, bit % 32
        x = (w[i] >> U64(sh)) if i < nw else np.zeros(w.shape[1], U64)
        if i + 1 < nw:
            x = x | (w[i + 1] << U64(32 - sh))
        r[l] = (x & U64(M32) & U64(M30)).astype(I64)
    return r


def to_words(a, nw):
    nl = NLIMBS[nw]
    assert ((a >= 0) & (a <= M30)).all(), "to_words: a limb outside [0, 2^30)"
    w = np.zeros((nw, a.shape[1]), U64)
    for i in range(nw):
        bit = 32 * i
        l, sh = bit // 30, bit % 30
        x = u32(a[l]) >> U64(sh)
        if l + 1 < nl:
            x = x | (u32(a[l + 1]) << U64(30 - sh))
        if l + 2 < nl:
            x = x | (u32(a[l + 2]) << U64(60 - sh))       # (60 - sh >= 32: never reaches the word; as written)
        w[i] = x & U64(M32)
    return w


def inv30(p0):
    x = p0 & M32
    for _ in range(4):
        x = (x * ((2 - p0 * x) & M32)) & M32
    x &= M30
    assert (p0 * x) & M30 == 1
    return x


def limbs_value(a):
    """the integers a (NL, n) array of signed limbs stands for (Python integers: exact)"""
    out = [0] * a.shape[1]
    for l in range(a.shape[0] - 1, -1, -1):
        col = a[l].tolist()
        out = [(o << 30) + c for o, c in zip(out, col)]
    return out


def limbs_ratio(a, modulus):
    """a / modulus per lane as float64 (for the traces and a first look at the intervals)"""
    acc = np.zeros(a.shape[1])
    for l in range(a.shape[0] - 1, -1, -1):
        acc = acc * float(1 << 30) + a[l]
    return acc / float(modulus)


def divsteps_30(zeta, f0, g0, garbage=None):
    """30 half-delta division steps on the 64-bit pairs.  zeta: int64 holding an int32_t; f0, g0: uint64 holding a uint32_t.
    garbage: a numpy Generator that re-draws the upper halves of f, g, u, v, q, r before every step."""
    n = len(f0)
    one, zero = np.ones(n, U64), np.zeros(n, U64)
    u, v, q, r, f, g = one.copy(), zero.copy(), zero.copy(), one.copy(), f0.copy(), g0.copy()
    lo = U64(M32)
    for i in range(30):
        if garbage is not None:
            u, v, q, r, f, g = ((x & lo) | (garbage.integers(0, 1 << 32, n, dtype=U64) << U64(32)) for x in (u, v, q, r, f, g))
        neg = u32(zeta >> I64(31))
        c2 = (U64(0) - (g & U64(1))) & lo
        m1 = (neg | U64(1)) & c2
        fl, ul, vl = f & lo, u & lo, v & lo
        g = g + fl * m1                                    # step_a: three v_mad_u64_u32
        q = q + ul * m1
        r = r + vl * m1
        c1 = neg & c2
        zeta = s32(u32(zeta) ^ c1) - I64(1)
        m2 = c1 & U64(1)
        gl, ql, rl = g & lo, q & lo, r & lo
        f = f + gl * m2                                    # step_b: three v_mad_u64_u32, v_lshrrev_b64, two v_lshlrev_b64
        u = u + ql * m2
        v = v + rl * m2
        g = g >> U64(1)
        u = u << U64(1)
        v = v << U64(1)
    fits32(zeta, "zeta")                                   # (it moves by one per step: checked once per batch)
    return zeta, (s32(u), s32(v), s32(q), s32(r))


def check_trans(t):
    for name, x in zip("uvqr", t):
        assert ((x >= -(1 << 30)) & (x <= (1 << 30))).all(), "matrix entry %s outside [-2^30, 2^30]" % name


def umul24(a, b):
    return ((a & U64(0xFFFFFF)) * (b & U64(0xFFFFFF))) & U64(M32)


def ctz32(x):
    low = x & ((~x) + U64(1))
    return np.log2(low.astype(np.float64)).astype(I64)     # exact: a power of two below 2^32


def divsteps_30_var(eta, f0, g0, limit_cap=LIMIT_CAP):
    """The variable-time batch: every lane runs its own loop; a lane that has left the loop (i = 0) is masked.
    Returns eta, the matrix, and (iterations, limit bits, swapped) per lane."""
    n = len(f0)
    lo = U64(M32)
    u, v, q, r = np.ones(n, U64), np.zeros(n, U64), np.zeros(n, U64), np.ones(n, U64)
    f, g = f0.copy(), g0.copy()
    i = np.full(n, 30, I64)
    eta = eta.copy()
    iters, limits, swapped = np.zeros(n, I64), np.zeros(n, I64), np.zeros(n, bool)
    while True:
        live = i > 0
        zeros = ctz32(g | ((U64(M32) << i.astype(U64)) & lo))
        assert (zeros <= i).all()
        zeros = np.where(live, zeros, 0)
        zu = zeros.astype(U64)
        g = g >> zu
        u = (u << zu) & lo
        v = (v << zu) & lo
        eta = eta - zeros
        i = i - zeros
        live = i > 0
        if not live.any():
            break
        iters += live
        assert ((g & U64(1)) == 1)[live].all() and ((f & U64(1)) == 1).all()
        sw = live & (eta < 0)
        swapped |= sw
        eta = np.where(sw, -eta, eta)
        f, g = np.where(sw, g, f), np.where(sw, (U64(0) - f) & lo, g)
        u, q = np.where(sw, q, u), np.where(sw, (U64(0) - u) & lo, q)
        v, r = np.where(sw, r, v), np.where(sw, (U64(0) - v) & lo, r)
        limit = np.where(live, np.minimum(eta + 1, i), 1)
        assert (limit >= 1).all()
        limits |= np.where(live, I64(1) << np.minimum(limit, limit_cap), 0)
        m = (U64(M32) >> (U64(32) - limit.astype(U64))) & U64((1 << limit_cap) - 1)
        fl, gl = f & U64(63), g & U64(63)
        w_host = ((fl * gl * ((fl * fl - U64(2)) & lo)) & lo) & m
        w = umul24(umul24(fl, gl), (umul24(fl, fl) - U64(2)) & lo) & m
        assert (w == w_host).all(), "the 24-bit multiplies and the 32-bit ones disagree on w"
        w = np.where(live, w, U64(0))
        g = (f * w + g) & lo                               # mad_lo
        q = (u * w + q) & lo
        r = (v * w + r) & lo
        assert (((g & m) == 0) | ~live).all(), "the addition did not clear the low `limit` bits of g"
    fits32(eta, "eta")
    return eta, (s32(u), s32(v), s32(q), s32(r)), (iters, limits, swapped)


def update_de(d, e, t, p, pinv30, acc, tr=None, drop_sign_term=False):
    """p: the modulus's limbs as Python integers.  drop_sign_term: the mutation `md = 0, me = 0 at the start` (for the tests)."""
    nl = d.shape[0]
    u, v, q, r = t
    sd, se = d[nl - 1] >> I64(31), e[nl - 1] >> I64(31)
    md = fits32((u & sd) + (v & se), "md")
    me = fits32((q & sd) + (r & se), "me")
    if drop_sign_term:
        md, me = md * 0, me * 0
    di, ei = d[0], e[0]
    zero = np.zeros_like(di)
    cd = acc.mad(u, di, acc.mad(v, ei, zero))
    ce = acc.mad(q, di, acc.mad(r, ei, zero))
    md = fits32(md - ((u32(cd) * U64(pinv30) + u32(md)) & U64(M32) & U64(M30)).astype(I64), "md")
    me = fits32(me - ((u32(ce) * U64(pinv30) + u32(me)) & U64(M32) & U64(M30)).astype(I64), "me")
    if tr is not None:
        np.maximum(tr.md, np.maximum(np.abs(md), np.abs(me)), out=tr.md)
    cd = acc.mad(I64(p[0]), md, cd)
    ce = acc.mad(I64(p[0]), me, ce)
    assert ((cd & I64(M30)) == 0).all() and ((ce & I64(M30)) == 0).all(), "update_de: the low 30 bits of cd / ce are not zero"
    cd = cd >> I64(30)
    ce = ce >> I64(30)
    for i in range(1, nl):
        di, ei = d[i], e[i]
        cd = acc.mad(u, di, cd)                            # smad6, in the order of its six instructions
        ce = acc.mad(q, di, ce)
        cd = acc.mad(v, ei, cd)
        ce = acc.mad(r, ei, ce)
        cd = acc.mad(I64(p[i]), md, cd)
        ce = acc.mad(I64(p[i]), me, ce)
        d[i - 1] = cd & I64(M30)
        cd = cd >> I64(30)
        e[i - 1] = ce & I64(M30)
        ce = ce >> I64(30)
    d[nl - 1] = fits32(cd, "the top limb of d")
    e[nl - 1] = fits32(ce, "the top limb of e")


def update_fg(f, g, t, acc):
    nl = f.shape[0]
    u, v, q, r = t
    fi, gi = f[0], g[0]
    zero = np.zeros_like(fi)
    cf = acc.mad(u, fi, acc.mad(v, gi, zero))
    cg = acc.mad(q, fi, acc.mad(r, gi, zero))
    assert ((cf & I64(M30)) == 0).all() and ((cg & I64(M30)) == 0).all(), "update_fg: the low 30 bits of cf / cg are not zero"
    cf = cf >> I64(30)
    cg = cg >> I64(30)
    for i in range(1, nl):
        fi, gi = f[i], g[i]
        cf = acc.mad(u, fi, cf)                            # smad4
        cg = acc.mad(q, fi, cg)
        cf = acc.mad(v, gi, cf)
        cg = acc.mad(r, gi, cg)
        f[i - 1] = cf & I64(M30)
        cf = cf >> I64(30)
        g[i - 1] = cg & I64(M30)
        cg = cg >> I64(30)
    f[nl - 1] = fits32(cf, "the top limb of f")
    g[nl - 1] = fits32(cg, "the top limb of g")


def normalize(d, fsign, p, second_pass=True):
    """Returns the normalised copy of d (the header works in place).  second_pass=False: the mutation, for the tests."""
    nl = d.shape[0]
    d = d.copy()
    cond_add = d[nl - 1] >> I64(31)
    cond_neg = fsign >> I64(31)
    carry = np.zeros_like(cond_add)
    for i in range(nl):
        x = fits32(d[i] + (I64(p[i]) & cond_add), "normalize")
        x = fits32((x ^ cond_neg) - cond_neg, "normalize")
        x = fits32(x + carry, "normalize")
        if i + 1 < nl:
            carry = x >> I64(30)
            x = x & I64(M30)
        d[i] = x
    if second_pass:
        cond_add = d[nl - 1] >> I64(31)
        carry = np.zeros_like(cond_add)
        for i in range(nl):
            x = fits32(d[i] + (I64(p[i]) & cond_add) + carry, "normalize")
            if i + 1 < nl:
                carry = x >> I64(30)
                x = x & I64(M30)
            d[i] = x
    return d


# ---- the intervals --------------------------------------------------------------------------------------------------------------

def check_interval(a, modulus, lo, hi, what):
    """lo p < a < hi p for every lane: by float64 where that is clear, by Python integers within 1e-9 of an end.  The ratio."""
    ratio = limbs_ratio(a, modulus)
    near = (ratio < lo + 1e-9) | (ratio > hi - 1e-9)
    if near.any():
        idx = np.nonzero(near)[0]
        for j, val in zip(idx, limbs_value(a[:, idx])):
            assert lo * modulus < val < hi * modulus, "%s = %d leaves (%d p, %d p)" % (what, val, lo, hi)
    return ratio


def _track(tr, d, e, modulus):
    rd = check_interval(d, modulus, -2, 1, "d")
    re_ = check_interval(e, modulus, -2, 1, "e")
    np.minimum(tr.dmin, rd, out=tr.dmin)
    np.maximum(tr.dmax, rd, out=tr.dmax)
    np.minimum(tr.emin, re_, out=tr.emin)
    np.maximum(tr.emax, re_, out=tr.emax)


def _finish(tr, d, f, g, p, modulus, xs, nw, check_result, second_pass=True):
    nl = d.shape[0]
    assert (g == 0).all(), "g != 0 after the last batch (lanes %s)" % np.nonzero((g != 0).any(axis=0))[0][:8]
    plus = (f[0] == 1) & (f[1:] == 0).all(axis=0)
    minus = (f[: nl - 1] == M30).all(axis=0) & (f[nl - 1] == -1)
    zero_in = np.array([x % modulus == 0 for x in xs])
    fp = (f == np.array(p, dtype=I64)[:, None]).all(axis=0)            # x = 0 mod p: gcd = p, f = +-p, d = 0
    fm = np.array([v == -modulus for v in limbs_value(f[:, zero_in])], dtype=bool) if zero_in.any() else np.zeros(0, bool)
    assert (plus | minus)[~zero_in].all(), "f != +-1 at the end"
    if zero_in.any():
        assert (fp[zero_in] | fm).all(), "f != +-p at the end of the inversion of 0"
    tr.dneg = d[nl - 1] < 0
    tr.fneg = f[nl - 1] < 0
    tr.dlow = limbs_ratio(d, modulus) < -1.0
    out = normalize(d, f[nl - 1], p, second_pass)
    words = to_words(out, nw)
    if check_result:
        got = limbs_value(out)
        for j, x in enumerate(xs):
            want = pow(x, -1, modulus) if x % modulus else 0
            assert got[j] == want, "x = %#x: the model returns %#x, pow(x, -1, p) is %#x" % (x, got[j], want)
    return out, words


def words_value(w):
    out = [0] * w.shape[1]
    for i in range(w.shape[0] - 1, -1, -1):
        out = [(o << 32) + c for o, c in zip(out, w[i].tolist())]
    return out


def _setup(xs, modulus, nw):
    nw = nw or nw_of(modulus)
    nl = NLIMBS[nw]
    n = len(xs)
    pw = to_limb_array([modulus], nw)
    p = [int(v) for v in from_words(pw, nw)[:, 0]]
    assert sum(v << (30 * i) for i, v in enumerate(p)) == modulus
    pinv30 = inv30(int(pw[0, 0]))
    f = np.repeat(np.array(p, dtype=I64)[:, None], n, axis=1)
    g = from_words(to_limb_array(xs, nw), nw)
    d = np.zeros((nl, n), I64)
    e = np.zeros((nl, n), I64)
    e[0] = 1
    return nw, nl, n, p, pinv30, f, g, d, e


def invert(xs, modulus, nw=None, garbage=None, batches=None, check=True, check_result=True, drop_sign_term=False, second_pass=True):
    """ModInv<NW>::invert on the integers xs (each below 2^(32 NW); the header's callers pass x < 2p at most).
    Returns (results as Python integers, Trace, the matrices of every batch).  batches / drop_sign_term / second_pass: mutations."""
    nw, nl, n, p, pinv30, f, g, d, e = _setup(xs, modulus, nw)
    nb = BATCHES[nw] if batches is None else batches
    tr = Trace(n, nb)
    acc = Acc(n, check)
    zeta = np.full(n, -1, I64)
    mats = []
    for it in range(nb):
        work = (g != 0).any(axis=0)
        tr.working[it] = work
        tr.batches = np.where(work, it + 1, tr.batches)
        zeta, t = divsteps_30(zeta, u32(f[0]), u32(g[0]), garbage)
        check_trans(t)
        tr.full_u |= work & (np.abs(t[0]) == (1 << 30))
        mats.append((zeta.copy(),) + t)
        update_de(d, e, t, p, pinv30, acc, tr, drop_sign_term)
        update_fg(f, g, t, acc)
        if check:
            acc.settle()
            _track(tr, d, e, modulus)
    tr.steps = 30 * tr.batches
    tr.acc = acc.max
    out, words = _finish(tr, d, f, g, p, modulus, xs, nw, check_result, second_pass)
    return words_value(words), tr, mats


def invert_var(xs, modulus, nw=None, wave=64, maxb=None, check=True, check_result=True, per_lane_break=False, limit_cap=LIMIT_CAP):
    """ModInv<NW>::invert_var.  wave = 64: the device (a lane goes on until the ballot of its wave is empty; len(xs) must be a
    multiple of 64), wave = 1: the host twin.  per_lane_break: the mutation in which a lane of a wave stops on its own g — the
    model then has to find nothing wrong with it, which is the point: see tests/test_modinv_vectors.py."""
    nw, nl, n, p, pinv30, f, g, d, e = _setup(xs, modulus, nw)
    assert n % wave == 0, "whole waves only"
    nb = MAXB_VAR[nw] if maxb is None else maxb
    tr = Trace(n, nb)
    acc = Acc(n, check)
    eta = np.full(n, -1, I64)
    running = np.ones(n, bool)                    # the lane's wave is still in the loop
    first = [None] * n                            # the value each lane would return when its g first became 0
    took = np.zeros(n, I64)                       # batches the lane ran through
    for it in range(nb):
        if not running.any():
            break
        work = (g != 0).any(axis=0) & running
        tr.working[it] = work
        tr.batches = np.where(work, it + 1, tr.batches)
        eta2, t, (iters, limits, swapped) = divsteps_30_var(eta, u32(f[0]), u32(g[0]), limit_cap)
        check_trans(t)
        d2, e2, f2, g2 = d.copy(), e.copy(), f.copy(), g.copy()
        update_de(d2, e2, t, p, pinv30, acc, tr)
        update_fg(f2, g2, t, acc)
        keep = ~running                           # lanes whose wave has left the loop do nothing any more
        eta = np.where(keep, eta, eta2)
        for old, new in ((d, d2), (e, e2), (f, f2), (g, g2)):
            old[:, running] = new[:, running]
        took += running
        tr.iters[it] = np.where(running, iters, 0)
        tr.limits |= np.where(work, limits, 0)
        tr.limits_batch[it] = np.where(work, limits, 0)
        tr.swaps[it] = swapped & work
        tr.full_u |= work & (np.abs(t[0]) == (1 << 30))
        if check:
            acc.settle()
            _track(tr, d, e, modulus)
        done = ~(g != 0).any(axis=0)
        fresh = [j for j in np.nonzero(done & running)[0] if first[j] is None]
        if fresh:
            vals = limbs_value(normalize(d[:, fresh], f[nl - 1, fresh], p))
            for j, val in zip(fresh, vals):
                first[j] = val
        if per_lane_break:
            running &= ~done
        else:
            busy = (~done).reshape(-1, wave).any(axis=1)                 # the ballot: any lane of the wave with g != 0
            running &= np.repeat(busy, wave)
    tr.steps = tr.iters.sum(axis=0)
    tr.acc = acc.max
    tr.took = took
    out, words = _finish(tr, d, f, g, p, modulus, xs, nw, check_result)
    res = words_value(words)
    for j in range(n):
        assert first[j] == res[j], "lane %d: %#x when its g became 0, %#x after the batches it took along with its wave" % (j, first[j], res[j])
    return res, tr


def garbage_identity(xs, modulus, seed=1):
    """The claim of the header's "Device:" paragraph: with the upper halves of the six pairs re-drawn before every step, every batch
    gives the same matrix and the same zeta as with the halves the arithmetic leaves there."""
    a = invert(xs, modulus)
    b = invert(xs, modulus, garbage=np.random.default_rng(seed))
    assert a[0] == b[0]
    assert len(a[2]) == len(b[2])
    for it, (ma, mb) in enumerate(zip(a[2], b[2])):
        for name, x, y in zip(("zeta", "u", "v", "q", "r"), ma, mb):
            assert (x == y).all(), "batch %d: %s depends on the upper halves" % (it, name)
    return a


# ---- self-test ------------------------------------------------------------------------------------------------------------------

SELFTEST_MODULI = {
    6: 2 ** 192 - 2 ** 64 - 1,
    7: 2 ** 224 - 2 ** 96 + 1,
    8: 2 ** 256 - 2 ** 32 - 977,
    12: 2 ** 384 - 2 ** 128 - 2 ** 96 + 2 ** 32 - 1,
    17: 2 ** 521 - 1,
}


def main():
    import random
    check_header_constants()
    for nw, m in sorted(SELFTEST_MODULI.items()):
        rnd = random.Random(30 + nw)
        xs = [0, 1, 2, m - 1, m - 2, (m + 1) // 2, (m - 1) // 2, 1 << 30, 1 << 60, m >> 30 << 30]
        xs += [1 << k for k in range(0, m.bit_length() - 1, 7)] + [m - (1 << k) for k in range(0, m.bit_length() - 1, 7)]
        xs += [rnd.randrange(m) for _ in range(256 - len(xs) % 64 + 64)]
        xs = xs[: len(xs) // 64 * 64]
        res, tr, _ = garbage_identity(xs, m)
        rv, trv = invert_var(xs, m, wave=64)
        r1, _ = invert_var(xs[:64], m, wave=1)
        assert res == rv and r1 == rv[:64]
        print("NW = %2d: %d inputs; branch-free form: g = 0 after at most %d of %d batches, d / p in [%.3f, %.3f], e / p in [%.3f, %.3f], "
              "max |md| %d, largest accumulator 2^%.2f; variable form: at most %d of %d batches, %d iterations in a batch at most; "
              "matrices and zeta independent of the upper halves" % (
                  nw, len(xs), tr.batches.max(), BATCHES[nw], tr.dmin.min(), tr.dmax.max(), tr.emin.min(), tr.emax.max(), tr.md.max(),
                  np.log2(float(tr.acc.max())), trv.batches.max(), MAXB_VAR[nw], trv.iters.max()))
    print("modinv model selftest: True")
    return 0


if __name__ == "__main__":
    sys.exit(main())
