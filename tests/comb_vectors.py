"""Scalars that aim at single entries of the generator's signed comb table, shared by tests/test_comb_vectors.py (the Python model,
the g++ twin) and tests/test_gpu_comb_table.py (gfx950).  Plain module: deterministic, seeded per curve id; every comparison made
with these vectors is exact.

`recode(c, w, k)` restates what fixed_base_mul (csrc/ecgpu_fixedmul.h) does with a scalar: fold_scalar on the 32 N-bit word array,
then signed_window_step per window, nwin = signed_window_count(32 N - 1, w).  Window j with digit d adds (sign d) * entry
(j, |d|) = |d| * 2^(w j) * G, table index |d| - 1.

A scalar k = e * 2^(w j) with e <= 2^(w-1), k < n and k < 2^(32 N - 1) recodes to the one digit +e in window j without a fold, so
mul_by_generator returns that table entry itself (state == 1 in fixed_base_mul: no addition touches it).  `reachable(c, w)` gives
the largest such e per window.  The entries of the top window above that bound (and every entry of a window that starts above the
order's top bit: p521 holds 521 bits in 544) cannot be selected by any valid scalar through the ABI; they are out of scope here.

`entry_sample(c, w)` is the structured sample of (j, e): window edges, powers of two, the wraps of the build's lane chains and
2,048 random e per window.  The build's geometry (lanes of k_table_entries, records per lane of launch_normalize, the slab rule of
build_table, the widest width per set, the tier thresholds, the number of generator LUTs) is read from the sources by regular
expression and the expressions found are asserted, so a changed build cannot leave the sample aiming at the old boundaries.

Every scalar this module emits is run through `recode` and must decode to what its record says (`Vec.digits`)."""
import functools
import os
import random
import re
from collections import namedtuple

import pyec
from field_vectors import CSRC, CURVES, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RANDOM_PER_WINDOW = 2048
EDGE = 64

# k: the scalar; (j, e): the entry it aims at; form: "pos" e 2^(w j), "neg" (2^w - e) 2^(w j), "nk" n - e 2^(w j);
# flip: whether fold_scalar replaces it by n - k; digits: {window: digit} of all its non-zero digits, or None where the form
# promises nothing but a valid scalar (n - k below the fold: a many-digit string)
Vec = namedtuple("Vec", "k j e form flip digits")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- the build's geometry, read from the sources ---------------------------------------------------------------------------------

@functools.lru_cache(None)
def _geometry():
    base = _src("ecgpu_inst_base.hip")
    api = _src("ecgpu_api.hip")
    field = _src("ecgpu_field.h")
    ctmul = _src("ecgpu_ctmul.h")
    params = _src("ecgpu_params.h")
    kernels = _src("ecgpu_kernels.h")
    g = {}
    # k_table_entries: lane t of a window owns e = t + 1, t + 1 + T, ..; T = 2^tlog
    m = re.search(r"launch_table_entries<CurveT>\(.*?\{\s*int tlog = ([^;]+);[^\n]*\n\s*if \(tlog > (\d+)\) tlog = (\d+);", base, re.S)
    assert m and m.group(1) == "w - 1 > 6 ? w - 1 - 6 : 0" and m.group(2) == m.group(3) == "17", m and m.groups()
    assert "for (size_t e = e0; e <= half; e += T)" in kernels and "const uint32_t e0 = t + 1;" in kernels
    g["tlog_cap"] = int(m.group(2))
    # launch_normalize: K = min(64, ceil(n / 65536)) records per lane, lane t owns records t, t + nthreads, ..
    m = re.search(r"void launch_normalize<CurveT>\(.*?\{\s*if \(n == 0\) return;\s*size_t k = ([^;]+);\s*if \(k > (\d+)\) k = (\d+);"
                  r".*?size_t nthreads = ([^;]+);", base, re.S)
    assert m and m.group(1) == "(n + 65535) / 65536" and m.group(2) == m.group(3) == "64" and m.group(4) == "(n + k - 1) / k", m and m.groups()
    assert "for (size_t j = t; j < n; j += nthreads)" in kernels
    g["norm_per"], g["norm_k"] = 65536, 64
    # build_table: whole windows per slab, one k_table_entries + one normalisation per slab
    m = re.search(r"size_t slab = ([^;]+);\s*if \(slab < 1\) slab = 1;\s*if \(slab > \(size_t\)nwin\) slab = nwin;", api)
    assert m and m.group(1) == "((size_t)2 << 30) / (half * (4 * NS) * 4)", m and m.group(1)
    assert "const int nwin = signed_window_count(bits - 1, w);" in api and "const size_t half = (size_t)1 << (w - 1);" in api
    assert re.search(r"launch_normalize<C>\(ctx->stream, true, [^;]*ws \* half, nullptr,\s*nullptr, d \+ j0 \* half \* \(2 \* N\)\);", api)
    assert "ECGPU_CONST int NS = (C::NL / 4 + 1) * 4;" in field
    # the widest table per set and the adaptive tiers
    m = re.search(r"int want_w\[12\] = \{([0-9, ]+)\};", api)
    g["widest"] = tuple(int(x) for x in m.group(1).split(","))
    assert len(g["widest"]) == 12
    m = re.search(r"constexpr int TABLE_TIER1_LOG2 = (\d+), TABLE_TIER2_LOG2 = (\d+);", api)
    g["tier_log2"] = (int(m.group(1)), int(m.group(2)))
    m = re.search(r"inline int table_tier\(uint64_t seen, int wmax\) \{\s*int w = ([^;]+);\s*return w < wmax \? w : wmax;", api)
    assert m and m.group(1) == "seen < ((uint64_t)1 << TABLE_TIER1_LOG2) ? 16 : seen < ((uint64_t)1 << TABLE_TIER2_LOG2) ? 22 : wmax", m and m.group(1)
    g["tier_w"] = (16, 22)
    # the generator LUTs of the uniform-schedule path
    assert re.search(r"constexpr int CT_BASE_W = 6;", params) and "CT_BASE_ENTRIES = 1 << (CT_BASE_W - 1);" in params
    assert "constexpr int CT_BASE_LUTS = ct_scalar_bits<C>() / CT_BASE_W + 1;" in ctmul
    g["ct_w"] = 6
    return g


def words(c):
    """N: 32-bit words of a scalar (C::N)."""
    return (8 * c.L + 31) // 32


def window_count(c, w):
    """signed_window_count(32 N - 1, w)"""
    return (32 * words(c) - 1) // w + 1


def widest(c):
    return _geometry()["widest"][c.cid]


def widths_in_use(c):
    """The three tables the default (adaptive) policy takes a device through."""
    t1, t2 = _geometry()["tier_w"]
    return tuple(sorted({min(t1, widest(c)), min(t2, widest(c)), widest(c)}))


WIDTHS = {name: widths_in_use(pyec.CURVES[name]) for name in CURVES}


def table_tier(seen, wmax):
    """csrc/ecgpu_api.hip table_tier (its expression is asserted in _geometry)."""
    l1, l2 = _geometry()["tier_log2"]
    t1, t2 = _geometry()["tier_w"]
    return min(t1 if seen < (1 << l1) else t2 if seen < (1 << l2) else wmax, wmax)


def tier_thresholds():
    l1, l2 = _geometry()["tier_log2"]
    return 1 << l1, 1 << l2


def entry_lanes(w):
    """T of k_table_entries at width w."""
    return 1 << min(max(w - 1 - 6, 0), _geometry()["tlog_cap"])


def normalize_lanes(npoints):
    """(K, lanes) of launch_normalize for a call on npoints records."""
    g = _geometry()
    k = min(g["norm_k"], (npoints + g["norm_per"] - 1) // g["norm_per"])
    return k, (npoints + k - 1) // k


def slab_windows(c, w):
    """Windows per slab of build_table."""
    ns = (layout(c.name).nl // 4 + 1) * 4
    half = 1 << (w - 1)
    return max(1, min(window_count(c, w), (2 << 30) // (half * (4 * ns) * 4)))


def ct_base_luts(c):
    return c.n.bit_length() // _geometry()["ct_w"] + 1


# ---- the recoding model ----------------------------------------------------------------------------------------------------------

def recode(c, w, k):
    """(flip, digits): what fixed_base_mul does with the valid scalar k at width w — fold_scalar (k -> n - k when bit 32 N - 1 is
    set), then one signed_window_step per window, least significant first.  A carry out of the top window would be dropped by the
    kernel; it is an error here."""
    assert 0 <= k < c.n
    bits = 32 * words(c)
    flip = bool(k >> (bits - 1))
    if flip:
        k = c.n - k
    half, full, mask = 1 << (w - 1), 1 << w, (1 << w) - 1
    digits = []
    carry = 0
    nwin = window_count(c, w)
    while k or carry:
        v = (k & mask) + carry
        k >>= w
        if v > half:
            digits.append(v - full)
            carry = 1
        else:
            digits.append(v)
            carry = 0
    assert len(digits) <= nwin, "the top window must absorb what is left"
    return flip, digits + [0] * (nwin - len(digits))                 # nothing left and no carry: the windows above are zero


def decode(c, w, flip, digits):
    """The scalar a digit string stands for."""
    v = sum(d << (w * j) for j, d in enumerate(digits))
    return (-v if flip else v) % c.n


def check_vec(c, w, v):
    """A vector decodes to what its record says."""
    flip, digits = recode(c, w, v.k)
    assert flip == v.flip, (c.name, w, v)
    if v.digits is None:
        assert decode(c, w, flip, digits) == v.k
    else:
        assert {j: d for j, d in enumerate(digits) if d} == v.digits, (c.name, w, v, digits)


# ---- which entries a scalar can select -------------------------------------------------------------------------------------------

def unfolded_limit(c):
    """Scalars below this are valid and not folded."""
    return min(c.n, 1 << (32 * words(c) - 1))


def reachable(c, w):
    """Per window j the largest e <= 2^(w-1) with e * 2^(w j) valid and unfolded (0: no entry of that window)."""
    lim = unfolded_limit(c)
    return [min(1 << (w - 1), (lim - 1) >> (w * j)) for j in range(window_count(c, w))]


def forms(c, w, j, e):
    """The vectors that aim at entry (j, e): the entry itself, and its two signed forms where they exist."""
    lim = unfolded_limit(c)
    k = e << (w * j)
    assert 0 < k < lim and e <= 1 << (w - 1)
    out = [Vec(k, j, e, "pos", False, {j: e})]
    if e < 1 << (w - 1):
        k2 = ((1 << w) - e) << (w * j)                           # digit -e, carry +1 into window j + 1
        if k2 < lim and j + 1 < window_count(c, w):
            out.append(Vec(k2, j, e, "neg", False, {j: -e, j + 1: 1}))
        k3 = c.n - k                                             # folded back to k where its top bit is set
        if k3 >> (32 * words(c) - 1):
            out.append(Vec(k3, j, e, "nk", True, {j: e}))
        else:
            out.append(Vec(k3, j, e, "nk", False, None))
    return out


@functools.lru_cache(None)
def _sample(name, w):
    c = pyec.CURVES[name]
    rng = random.Random(0xC03B0000 + 64 * c.cid + w)
    half = 1 << (w - 1)
    T = entry_lanes(w)
    slab = slab_windows(c, w)
    out = {}
    for j, E in enumerate(reachable(c, w)):
        if E == 0:
            continue
        es = set(range(1, min(EDGE, E) + 1)) | set(range(max(1, E - EDGE + 1), E + 1))
        for i in range(w):
            es.update((1 << i) + d for d in (-1, 0, 1))
        # k_table_entries: e = m T is the last lane's, m T + 1 lane 0's next record
        for m in sorted({1, 2, E // T}):
            es.update(m * T + d for d in (-1, 0, 1, 2))
        # the slab's normalisation: record (j - j0) half + e - 1 of ws * half, lane = record mod lanes
        j0 = j - j % slab
        ws = min(slab, window_count(c, w) - j0)
        _, lanes = normalize_lanes(ws * half)
        off = (j - j0) * half
        m_lo, m_hi = -(-off // lanes), (off + E - 1) // lanes
        for m in sorted({m_lo, m_lo + 1, m_hi}):
            if m >= 1:
                es.update(m * lanes - off + d for d in (-1, 0, 1, 2))
        # slab edges are window edges (a slab is whole windows): the first and the last entries above cover them
        es = {e for e in es if 1 <= e <= E}
        want = min(RANDOM_PER_WINDOW, E)
        picks = set()
        while len(picks) < want:
            picks.add(rng.randint(1, E))
        out[j] = tuple(sorted(es | picks))
    return out


def entry_sample(c, w):
    """{window: sorted e} — the structured sample described in the module docstring."""
    return _sample(c.name, w)


def sample_vectors(c, w, entries=None):
    """Every form of every sampled (or given: {j: iterable of e}) entry, each checked against `recode`."""
    entries = entry_sample(c, w) if entries is None else entries
    out = []
    for j in sorted(entries):
        for e in entries[j]:
            out += forms(c, w, j, e)
    for v in out:
        check_vec(c, w, v)
    return out


def all_entries(c, w):
    """{window: range of every reachable e}"""
    return {j: range(1, E + 1) for j, E in enumerate(reachable(c, w)) if E}


def check_sample_coverage(c, w):
    """The sample's own minimum contents (a refactoring must not thin it silently)."""
    s = entry_sample(c, w)
    R = reachable(c, w)
    half = 1 << (w - 1)
    T = entry_lanes(w)
    slab = slab_windows(c, w)
    assert sorted(s) == [j for j, E in enumerate(R) if E], (c.name, w)
    assert R[0] == half and all(E == half for E in R[: len(s) - 1]), (c.name, w)        # only the top reachable window is cut
    for j, es in s.items():
        E = R[j]
        have = set(es)
        assert 1 in have and E in have and all(1 <= e <= E for e in es), (c.name, w, j)
        assert len(es) >= min(E, RANDOM_PER_WINDOW), (c.name, w, j, len(es))
        assert have >= set(range(1, min(EDGE, E) + 1)) | set(range(max(1, E - EDGE + 1), E + 1))
        assert have >= {1 << i for i in range(w) if (1 << i) <= E}
        if T + 1 <= E:
            assert {T, T + 1} <= have                            # the first wrap of k_table_entries' lanes
        if j % slab == 0 and j:
            assert half in set(s[j - 1])                         # the slab before ends on its window's last entry
    if half > RANDOM_PER_WINDOW + 4 * EDGE:
        assert sum(len(es) for es in s.values()) >= (len(s) - 1) * (RANDOM_PER_WINDOW + EDGE)


# ---- the generator LUTs of the uniform-schedule path -----------------------------------------------------------------------------

def ct_lut_scalars(c):
    """e * 2^(6 i) for every LUT i and e = 1..32 that stay below n, and n minus each: every entry of every LUT is selected, with
    both signs (fixed_base_mul_ct recentres its digits to [-32, 31]: e = 32 arrives as -32 with a carry)."""
    w = _geometry()["ct_w"]
    ks = []
    for i in range(ct_base_luts(c)):
        for e in range(1, (1 << (w - 1)) + 1):
            k = e << (w * i)
            if k < c.n:
                ks += [k, c.n - k]
    return ks


def enc(c, ks):
    return b"".join(k.to_bytes(c.L, c.order) for k in ks)
