"""Adversarial scalars for the MSM digit recodings (csrc/ecgpu_recode.h: fold_scalar, signed_window_step, msm_digit /
MsmDigitStream, the top window's sub-bucket), the k256 GLV split (K256Scalar::decompose_signed) and the ladders' radix-16
recoding (Radix16Msb), shared by tests/test_scalar_vectors.py (the g++ twin) and tests/test_gpu_scalar_vectors.py (gfx950).
Plain module like tests/field_vectors.py: deterministic, seeded per curve id; every expected value is a Python integer.

Models (restatements on big integers, nothing shared with the C++):
  fold(c, k)                      fold_scalar: k -> n - k when the top bit of the 32 N-bit word array is set
  signed_digits / msm_digits      signed_window_step, the unsigned top window, the sub-bucket rule
  glv_split(k)                    the reference's split as exact integers: c_i = round(k g_i / 2^384), r2 = c1 (-b1) + c2 (-b2),
                                  r1 = k - r2 lambda (mod n), as signed halves and as canonical residues
  radix16(v, words)               Radix16Msb: the nibbles of v + 0x88..8

Families:
  D  digit strings, one set per (parameter set, split, c): all twelve sets plain, k256 also on its GLV halves, c = 4 .. 16.
     Every pattern is built in the sub-scalar domain (kbits bits, cut to the `value_bits` a canonical scalar can hold) and
     enters as k = v and, where that is a canonical scalar that folds back to v, as k = n - v.  The model, not the intention,
     says what digits a vector has; `check_coverage` asserts the events from the model's digits.
  G  the k256 split itself: structured halves, structured k, the rounding boundary of both quotients, the corners of the
     lattice's fundamental cell (where the halves are largest), random.
  X  radix-16 words: 0x77777778 / 0x78888888 / 0xFFFFFFFF / 0x88888888 in every word of the recoded value (a carry of
     k + 0x88..8 across every word boundary separately), a lone 7 / 8 / 9 in every nibble.

The constants and the window geometry are read from the sources and asserted (`source_facts`), so a retuned source fails here
instead of leaving the vectors aimed at the old one.  Nothing is dropped by try / skip."""
import os
import random
import re

import pyec
from field_vectors import CURVES, structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elliptic-curves_amd", "csrc")

WIDTHS = tuple(range(4, 17))
N_K256 = pyec.K256.n
LAMBDA = pyec.K256_LAMBDA
# k256/src/arithmetic/mul/glv.rs:10-37 as integers (asserted against csrc/ecgpu_recode.h below)
G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
MINUS_B1 = 0xE4437ED6010E88286F547FA90ABFE4C3
MINUS_B2 = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFE8A280AC50774346DD765CDA83DB1562C
GLV_KBITS = 128
GLV_VALUE_BITS = 126           # halves below 2^126 in magnitude come back from the split unchanged (asserted per vector)
MSM_GLV_MAX_TERMS = 13 << 17

# the reduced lattice basis v1 = (A1, B1), v2 = (A2, B2): a + b lambda = 0 (mod n)
B1 = -MINUS_B1
B2 = N_K256 - MINUS_B2
A1 = B2
A2 = (-B2 * LAMBDA) % N_K256
assert A2 < 1 << 129 and (A1 + B1 * LAMBDA) % N_K256 == 0 and (A2 + B2 * LAMBDA) % N_K256 == 0

_facts_checked = False


def source_facts():
    """Assert what the vectors aim at against the sources: the GLV constants, KBITS of both splits, signed_window_count, the
    widths ecgpu_set_msm_window accepts, MSM_GLV_MAX_TERMS and the words per scalar of every parameter set."""
    global _facts_checked
    if _facts_checked:
        return
    rec = open(os.path.join(CSRC, "ecgpu_recode.h")).read()

    def words(name):
        m = re.search(r"ECGPU_CONST uint32_t %s\[8\] = \{([^}]*)\}" % name, rec)
        w = [int(x.strip().rstrip("u"), 0) for x in m.group(1).split(",")]
        assert len(w) == 8, name
        return sum(x << (32 * i) for i, x in enumerate(w))
    assert words("G1") == G1 and words("G2") == G2
    assert words("MINUS_B1") == MINUS_B1 and words("MINUS_B2") == MINUS_B2
    assert words("MINUS_LAMBDA") == N_K256 - LAMBDA

    def limbs29(name, count):                       # what decompose_signed actually reads: the same integers on 29-bit limbs
        m = re.search(r"ECGPU_CONST uint32_t %s\[%d\] = \{([^}]*)\}" % (name, count), rec)
        w = [int(x.strip().rstrip("u"), 0) for x in m.group(1).split(",")]
        assert len(w) == count and all(x < 1 << 29 for x in w), name
        return sum(x << (29 * i) for i, x in enumerate(w))
    assert limbs29("G1_L29", 9) == G1 and limbs29("G2_L29", 9) == G2
    assert limbs29("MINUS_B1_L29", 5) == MINUS_B1 == -B1
    assert limbs29("B2_L29", 5) == B2 == A1 and limbs29("A2_L29", 5) == A2
    assert re.search(r"static constexpr int KBITS = 32 \* C::N - 1;", rec)
    assert re.search(r"static constexpr int KBITS = %d;" % GLV_KBITS, rec)
    assert re.search(r"int signed_window_count\(int bits, int w\) \{ return bits / w \+ 1; \}", rec)
    assert re.search(r"int msm_top_shift\(int kbits, int c\) \{ return c - 1 - kbits % c; \}", rec)
    api = open(os.path.join(CSRC, "ecgpu_api.hip")).read()
    assert re.search(r"window_bits != 0 && \(window_bits < %d \|\| window_bits > %d\)" % (WIDTHS[0], WIDTHS[-1]), api)
    msm = open(os.path.join(CSRC, "ecgpu_msm.h")).read()
    m = re.search(r"constexpr size_t MSM_GLV_MAX_TERMS = \(size_t\)(\d+) << (\d+);", msm)
    assert int(m.group(1)) << int(m.group(2)) == MSM_GLV_MAX_TERMS
    par = open(os.path.join(CSRC, "ecgpu_params.h")).read()
    stated = sorted(int(x) for x in re.findall(r"ECGPU_CONST int N = (\d+);", par))
    assert stated == sorted({c.name: scalar_words(c) for c in pyec.CURVES.values() if not c.name.endswith("t1")}.values()), stated
    _facts_checked = True


# ---- models ---------------------------------------------------------------------------------------------------------------

def scalar_words(c):
    return (8 * c.L + 31) // 32


def geometry(name, glv):
    """(kbits, value_bits): the width the windows are laid over, and how many low bits of it a sub-scalar of the D patterns uses
    (plain: every canonical folded scalar fits kbits, except p521 whose order has 521 bits in 17 words)."""
    c = pyec.CURVES[name]
    if glv:
        assert name == "k256"
        return GLV_KBITS, GLV_VALUE_BITS
    kbits = 32 * scalar_words(c) - 1
    return kbits, min(kbits, c.n.bit_length() - 1)


def window_count(kbits, cbits):
    return kbits // cbits + 1


def top_shift(kbits, cbits):
    return cbits - 1 - kbits % cbits


def fold(c, k):
    """(sub-scalar, flip) of the plain split."""
    assert 0 <= k < c.n
    if (k >> (32 * scalar_words(c) - 1)) & 1:
        return c.n - k, True
    return k, False


def signed_digits(sub, kbits, cbits):
    """The signed windows, least significant first: digits in (-2^(c-1), 2^(c-1)] and the unsigned top digit in [0, 2^rem]."""
    nwin = window_count(kbits, cbits)
    half = 1 << (cbits - 1)
    carry = 0
    out = []
    for w in range(nwin - 1):
        v = ((sub >> (w * cbits)) & ((1 << cbits) - 1)) + carry
        if v > half:
            out.append(v - (1 << cbits))
            carry = 1
        else:
            out.append(v)
            carry = 0
    rem = kbits % cbits
    out.append(((sub >> ((nwin - 1) * cbits)) & ((1 << rem) - 1)) + carry)
    assert sub >> kbits == 0
    return out


def buckets(digs, kbits, cbits, term_index, flip):
    """(bucket, neg, nonzero) per window from the signed digits: bucket = |d| - 1, and in the top window the sub-bucket
    ((d - 1) << shift) | (term_index mod 2^shift)."""
    shift = top_shift(kbits, cbits)
    out = []
    for w, d in enumerate(digs):
        if d == 0:
            out.append((0, 0, False))
        elif w < len(digs) - 1:
            out.append((abs(d) - 1, int((d < 0) != flip), True))
        else:
            out.append((((d - 1) << shift) | (term_index & ((1 << shift) - 1)), int(flip), True))
    return out


def msm_digits(sub, kbits, cbits, term_index, flip):
    return buckets(signed_digits(sub, kbits, cbits), kbits, cbits, term_index, flip)


def bucket_weight(w, nwin, bucket, kbits, cbits):
    return (bucket >> top_shift(kbits, cbits)) + 1 if w == nwin - 1 else bucket + 1


def glv_quotients(k):
    return (k * G1 + (1 << 383)) >> 384, (k * G2 + (1 << 383)) >> 384


def _signed(r):
    return r if r <= N_K256 // 2 else r - N_K256


def glv_split(k):
    """(r1, r2, residue1, residue2): the signed halves and what the reference returns."""
    c1, c2 = glv_quotients(k)
    r2 = (c1 * MINUS_B1 + c2 * MINUS_B2) % N_K256
    r1 = (k - r2 * LAMBDA) % N_K256
    return _signed(r1), _signed(r2), r1, r2


def glv_k(x, y):
    return (x + y * LAMBDA) % N_K256


def subs(name, glv, k):
    """[(sub-scalar, flip)] of a term's scalar, as MsmSplit<C, GLV>::split leaves them."""
    if glv:
        r1, r2, _, _ = glv_split(k)
        return [(abs(r1), r1 < 0), (abs(r2), r2 < 0)]
    return [fold(pyec.CURVES[name], k)]


def radix16(v, words):
    """Radix16Msb<words>: 8 words + 1 digits, least significant first."""
    kp = v + sum(0x88888888 << (32 * i) for i in range(words))
    return [((kp >> (4 * i)) & 15) - (8 if i < 8 * words else 0) for i in range(8 * words + 1)]


# ---- family D -------------------------------------------------------------------------------------------------------------

def d_patterns(kbits, cbits, value_bits, rng):
    """The target sub-scalars of one window layout, each below 2^value_bits (a pattern that reaches higher is cut there)."""
    c = cbits
    nwin = window_count(kbits, c)
    full = nwin - 1
    rem = kbits % c
    half = 1 << (c - 1)
    ones = (1 << c) - 1
    cut = (1 << value_bits) - 1
    top = full * c
    out = []
    # uniform digit strings (a negative sum wraps modulo 2^value_bits: the digits below stay, the top takes the carry)
    for d in (half, half - 1, -(half - 1), 1, -1):
        out.append(sum(d << (c * j) for j in range(full)) & cut)
    out.append(sum((half if j % 2 == 0 else -(half - 1)) << (c * j) for j in range(full)) & cut)
    # carry runs: raw windows 0 .. j all ones; the last one also fills the top window
    for j in range(full):
        out.append(((1 << (c * (j + 1))) - 1) & cut)
    out.append((1 << kbits) - 1 & cut)
    # one live window
    for j in range(nwin):
        w = c if j < full else rem
        if w == 0:
            continue
        raws = {1, 1 << (w - 1), (1 << (w - 1)) + 1, (1 << w) - 1}
        b = (c * j + w - 1) // 32 * 32              # a word boundary inside the window: the first bit of the high word, alone and with bit 0
        if c * j < b:
            raws |= {1 << (b - c * j), (1 << (b - c * j)) | 1}
        for raw in sorted(raws):
            out.append((raw << (c * j)) & cut)
    # the tie raw == half / half - 1 with the carry in 0 and 1
    for j in range(1, full):
        for raw in (half, half - 1):
            for below in (0, ones):
                out.append(((raw << (c * j)) | (below << (c * (j - 1)))) & cut)
    # the top window: digit 1, 2^rem - 1, 2^rem (through the carry), the carry alone; lower windows zero / as few as the carry
    # needs / random
    low_rand = [rng.randrange(1 << (c * (full - 1))) for _ in range(3)]
    carry_in = [ones << (c * (full - 1)), ((half + 1) << (c * (full - 1))) | low_rand[0], (ones << (c * (full - 1))) | low_rand[1]]
    no_carry = [0, (1 << (c * (full - 1))) | low_rand[2], low_rand[0]]
    for t in sorted({0, 1, (1 << rem) - 1}):
        for low in carry_in + no_carry:
            out.append(((t << top) | low) & cut)
    out += [rng.randrange(1 << value_bits) for _ in range(300)]
    return out


_d_cache = {}


def family_d(name, glv, cbits):
    """The scalars (canonical integers below n) of the D set of (parameter set, split, c), distinct, in a fixed order."""
    key = (name, glv, cbits)
    if key in _d_cache:
        return _d_cache[key]
    source_facts()
    c = pyec.CURVES[name]
    kbits, value_bits = geometry(name, glv)
    rng = random.Random(0xD161 + 1000 * c.cid + 16 * cbits + int(glv))
    pats = d_patterns(kbits, cbits, value_bits, rng)
    ks = []
    if not glv:
        for v in pats:
            assert v < c.n
            ks.append(v)
            if 0 < v and fold(c, c.n - v) == (v, True):
                ks.append(c.n - v)
    else:
        lim = 1 << GLV_VALUE_BITS
        structured_part = pats[:-300]
        others = ("zero", "one", "minus_one", "same", "random")
        turn = 0
        for m in structured_part:
            for h in (0, 1):
                for sign in (1, -1):
                    o = others[turn % len(others)]
                    osign = 1 if (turn // len(others)) % 2 == 0 else -1
                    turn += 1
                    other = {"zero": 0, "one": 1, "minus_one": -1, "same": osign * m, "random": osign * rng.randrange(lim)}[o]
                    pair = (sign * m, other) if h == 0 else (other, sign * m)
                    ks.append(_glv_checked(pair))
        for m in pats[-300:]:
            ks.append(_glv_checked((rng.choice((1, -1)) * m, rng.randrange(-lim + 1, lim))))
        ks += family_g()["corners"]
    seen = set()
    out = [k for k in ks if not (k in seen or seen.add(k))]
    _d_cache[key] = out
    return out


def _glv_checked(pair):
    k = glv_k(*pair)
    got = glv_split(k)[:2]
    if got != pair:
        raise AssertionError("the split model does not return the intended halves: %r -> k = %#x -> %r" % (pair, k, got))
    return k


def straddling_windows(kbits, cbits, value_bits):
    """[(window, boundary bit)] of the windows of the layout that straddle a 32-bit word boundary below value_bits (a window
    that ends above value_bits counts with the bits it has below it)."""
    out = []
    nwin = window_count(kbits, cbits)
    for j in range(nwin):
        lo = j * cbits
        hi = lo + (cbits if j < nwin - 1 else kbits % cbits)
        b = (hi - 1) // 32 * 32
        if lo < b < min(hi, value_bits):
            out.append((j, b))
    return out


# ---- family G -------------------------------------------------------------------------------------------------------------

_g_cache = None


def family_g():
    """{'halves', 'structured_k', 'boundary', 'corners', 'random'}: lists of k256 scalars; 'boundary' also as the quadruples
    'boundary_quads' = [(g index, t, [k - 1, k, k + 1, k + 2])]."""
    global _g_cache
    if _g_cache is not None:
        return _g_cache
    source_facts()
    n = N_K256
    rng = random.Random(0x61F5)
    lim = 1 << GLV_VALUE_BITS
    mags = {0, 1}
    for j in range(GLV_VALUE_BITS + 1):
        mags |= {1 << j, (1 << j) - 1}
    mags |= {v for v in structured(29, 5, 16, 1 << 125, lim)}
    mags = sorted(mags)
    S = sorted({s * m for m in mags for s in (1, -1)})
    halves = []
    for x in S:
        for y in [0, 1, -1, x, -x] + rng.sample(S, 3):
            halves.append((x, y))
            halves.append((y, x))
    halves = sorted(set(halves))
    halves_k = [_glv_checked(p) for p in halves]

    structured_k = sorted(set(structured(29, 9, 32, n, n) + structured(32, 8, 32, n, n)))

    quads = []
    for gi, g in enumerate((G1, G2)):
        tmax = (((n - 3) * g - (1 << 383)) >> 384) - 1
        ts = {(1 << (29 * i)) - 1 for i in range(1, 5) if (1 << (29 * i)) - 1 <= tmax}
        ts |= {t for t in structured(29, 5, 16, tmax // 2, tmax + 1) if t >= 1}
        ts = sorted(ts) + [rng.randrange(1, tmax + 1) for _ in range(250)]
        for t in ts:
            k0 = ((t << 384) + (1 << 383)) // g
            quad = [k0 + d for d in (-1, 0, 1, 2)]
            assert all(0 <= k < n for k in quad), (gi, t)
            quads.append((gi, t, quad))
    boundary = [k for _, _, q in quads for k in q]

    corners = []
    for s1 in (1, -1):
        for s2 in (1, -1):
            bx, by = (s1 * A1 + s2 * A2) // 2, (s1 * B1 + s2 * B2) // 2
            for d1 in range(-40, 41, 5):
                for d2 in range(-40, 41, 5):
                    corners.append(glv_k(bx + d1, by + d2))
    corners = list(dict.fromkeys(corners))

    rand = [rng.randrange(n) for _ in range(2000)]
    _g_cache = {"halves": halves_k, "halves_pairs": halves, "structured_k": structured_k, "boundary": boundary, "boundary_quads": quads,
                "corners": corners, "random": rand}
    return _g_cache


def g_all():
    g = family_g()
    return g["halves"] + g["structured_k"] + g["boundary"] + g["corners"] + g["random"]


# ---- family X -------------------------------------------------------------------------------------------------------------

X_WORDS = (0x77777778, 0x78888888, 0xFFFFFFFF, 0x88888888)
X_K256_BITS = 127              # a half of the X vectors: below 2^127 (word 3 of a pattern is cut there)

_x_cache = {}


def _x_values(words, value_bits, rng):
    cut = (1 << value_bits) - 1
    out = []
    for i in range(words):
        for pat in X_WORDS:
            out.append((pat << (32 * i)) & cut)
            out.append(((rng.getrandbits(32 * words) & ~(0xFFFFFFFF << (32 * i))) | (pat << (32 * i))) & cut)
    for nib in range((value_bits + 3) // 4):
        for d in (8, 7, 9):
            out.append((d << (4 * nib)) & cut)
    return out


def family_x(name):
    """Scalars whose recoded value (the scalar itself; for k256 each five-word half of the split) holds the X words."""
    if name in _x_cache:
        return _x_cache[name]
    source_facts()
    c = pyec.CURVES[name]
    rng = random.Random(0x8888 + c.cid)
    if name != "k256":
        ks = _x_values(scalar_words(c), c.n.bit_length() - 1, rng)
    else:
        ks = []
        small = 1 << 100
        for turn, m in enumerate(_x_values(4, X_K256_BITS, rng)):
            sign = 1 if turn % 2 == 0 else -1
            other = (0, 1, -1, rng.randrange(-small, small))[turn % 4]
            ks.append(glv_k(sign * m, other))
            ks.append(glv_k(other, -sign * m))
    out = list(dict.fromkeys(ks))
    assert all(0 <= k < c.n for k in out)
    _x_cache[name] = out
    return out


def x_recoded(name, k):
    """[(value, words)] that Radix16Msb sees for scalar k."""
    if name != "k256":
        return [(k, scalar_words(pyec.CURVES[name]))]
    r1, r2, _, _ = glv_split(k)
    return [(abs(r1), 5), (abs(r2), 5)]


# ---- coverage -------------------------------------------------------------------------------------------------------------

def check_coverage_d(name, glv, cbits, ks=None):
    """The events the D set of (set, split, c) must contain, read off the model's digits."""
    c = pyec.CURVES[name]
    ks = family_d(name, glv, cbits) if ks is None else ks
    kbits, value_bits = geometry(name, glv)
    nwin = window_count(kbits, cbits)
    full = nwin - 1
    rem = kbits % cbits
    half = 1 << (cbits - 1)
    assert len(ks) == len(set(ks)) >= 500, (name, glv, cbits, len(ks))
    assert all(0 <= k < c.n for k in ks)
    live = min(full, value_bits // cbits)            # full windows that lie wholly below value_bits
    uniform = {d: False for d in (half, half - 1, -(half - 1), 1, -1)}
    tie_by_carry = tie_plain = False
    longest_run = 0
    top_seen = set()
    top_with_low_zero = set()
    top_with_low_nonzero = set()
    alternating = False
    flips = {}                                       # half -> the sign flags seen
    strad = straddling_windows(kbits, cbits, value_bits)
    ways = {}                                        # (window, boundary bit) -> {"low", "high", "both"}
    for k in ks:
        for h, (sub, flip) in enumerate(subs(name, glv, k)):
            flips.setdefault(h, set()).add(flip)
            digs = signed_digits(sub, kbits, cbits)
            assert sum(d << (cbits * j) for j, d in enumerate(digs)) == sub
            assert all(-half < d <= half for d in digs[:-1]) and 0 <= digs[-1] <= 1 << rem
            for d in uniform:
                if all(x == d for x in digs[:live]):
                    uniform[d] = True
            if all(x == (half if j % 2 == 0 else -(half - 1)) for j, x in enumerate(digs[:live])):
                alternating = True
            raws = [(sub >> (cbits * j)) & ((1 << cbits) - 1) for j in range(full)]
            carry = 0
            run = 0
            for j in range(full):
                v = raws[j] + carry
                if v == half and carry:
                    tie_by_carry = True
                if v == half and not carry:
                    tie_plain = True
                carry = 1 if v > half else 0
                run = run + 1 if carry else 0
                longest_run = max(longest_run, run)
            top_seen.add(digs[-1])
            if digs[-1]:
                (top_with_low_nonzero if any(digs[:-1]) else top_with_low_zero).add(digs[-1])
            for j, b in strad:
                wbits = cbits if j < full else rem
                raw = (sub >> (cbits * j)) & ((1 << wbits) - 1)
                if raw and sub == raw << (cbits * j):
                    lo = raw & ((1 << (b - cbits * j)) - 1)
                    hi = raw >> (b - cbits * j)
                    ways.setdefault((j, b), set()).add("both" if lo and hi else "low" if lo else "high")
    assert all(uniform.values()) and alternating, (name, glv, cbits, uniform, alternating)
    assert tie_by_carry and tie_plain
    assert longest_run >= live, (name, glv, cbits, longest_run, live)      # a carry out of every full window in use, in one vector
    for key in strad:
        assert ways.get(key) == {"low", "high", "both"}, (name, glv, cbits, key, ways.get(key))
    if glv:
        assert flips == {0: {False, True}, 1: {False, True}}
        # (the top window of a half is reached through family G's corners only; how often is asserted in check_coverage_g)
        if rem == 0:
            assert 1 in top_seen
    elif value_bits == kbits:
        assert flips == {0: {False, True}}
        assert {0, 1, (1 << rem) - 1, 1 << rem} <= top_seen, (name, cbits, sorted(top_seen)[:5])
        assert {1, (1 << rem) - 1, 1 << rem} - {0} <= top_with_low_nonzero, (name, cbits)
        assert rem == 0 or {1, (1 << rem) - 1} <= top_with_low_zero, (name, cbits)
    else:
        assert top_seen == {0} and flips == {0: {False}}      # p521: 521 bits in a 543-bit layout, the top window stays empty


def check_coverage_g(g=None):
    g = family_g() if g is None else g
    lim = 1 << GLV_VALUE_BITS
    assert len(g["halves"]) >= 5000 and len(g["structured_k"]) >= 150 and len(g["random"]) == 2000
    pairs = g["halves_pairs"]
    assert any(x == 0 and y != 0 for x, y in pairs) and any(y == 0 and x != 0 for x, y in pairs)
    assert any(x < 0 and (-x) % (1 << 58) == 0 and -x >= 1 << 58 for x, _ in pairs)         # the two's-complement carry ripples
    assert any(y < 0 and (-y) % (1 << 116) == 0 and -y >= 1 << 116 for _, y in pairs)
    assert all(abs(x) <= lim and abs(y) <= lim for x, y in pairs)
    assert any(abs(x) == lim for x, _ in pairs) and any(abs(y) == lim for _, y in pairs)
    assert len(g["boundary_quads"]) >= 600
    for gi, t, quad in g["boundary_quads"]:
        q = [glv_quotients(k)[gi] for k in quad]
        assert q[1] == t and q[2] == t + 1, (gi, t, q)           # the rounded quotient steps inside every quadruple
    ts = {t for _, t, _ in g["boundary_quads"]}
    assert all((1 << (29 * i)) - 1 in ts for i in range(1, 5))   # the + carry after the shift ripples through 1 .. 4 limbs of t
    split = [glv_split(k)[:2] for k in g["corners"]]
    m1 = max(abs(a) for a, _ in split)
    m2 = max(abs(b) for _, b in split)
    assert m1 >= 0.63 * 2 ** 128 and m2 >= 0.54 * 2 ** 128, (m1 / 2 ** 128, m2 / 2 ** 128)
    assert all(abs(a) < 1 << 128 and abs(b) < 1 << 128 for k in g_all() for a, b in [glv_split(k)[:2]])
    for half in (0, 1):
        for sign in (1, -1):
            big = sum(1 for p in split if sign * p[half] >= 1 << 127)
            assert big >= 50, (half, sign, big)


def check_coverage_x(name, ks=None):
    ks = family_x(name) if ks is None else ks
    c = pyec.CURVES[name]
    if name != "k256":
        words, bits = scalar_words(c), c.n.bit_length() - 1
    else:
        words, bits = 4, X_K256_BITS
    lone = set()
    alone = set()
    among = set()
    for k in ks:
        for v, _ in x_recoded(name, k):
            for i in range(words):
                wv = (v >> (32 * i)) & 0xFFFFFFFF
                if wv and v == wv << (32 * i):
                    alone.add((i, wv))
                elif wv:
                    among.add((i, wv))
            if v:
                nib = (v.bit_length() - 1) // 4
                if v >> (4 * nib) in (7, 8, 9) and v == (v >> (4 * nib)) << (4 * nib):
                    lone.add((nib, v >> (4 * nib)))
    for i in range(words):
        for pat in X_WORDS:
            want = ((pat << (32 * i)) & ((1 << bits) - 1)) >> (32 * i)
            assert (i, want) in alone and (i, want) in among, (name, i, hex(want))
    for nib in range(bits // 4):
        assert {(nib, 7), (nib, 8), (nib, 9)} <= lone, (name, nib)


def check_coverage(name):
    """Every family of one parameter set: D at every width (k256: both splits), X, and for k256 G."""
    for glv in ((False, True) if name == "k256" else (False,)):
        for cbits in WIDTHS:
            check_coverage_d(name, glv, cbits)
    check_coverage_x(name)
    if name == "k256":
        check_coverage_g()


def first_digit_mismatch(name, glv, cbits, k, term_index, npad, got):
    """None, or a message: `got` is [(bucket, neg, nonzero)] per (half, window) of scalar k at the given term index."""
    kbits, _ = geometry(name, glv)
    for h, (sub, flip) in enumerate(subs(name, glv, k)):
        want = msm_digits(sub, kbits, cbits, h * npad + term_index, flip)
        if list(got[h]) != want:
            w = next(i for i in range(len(want)) if tuple(got[h][i]) != want[i])
            return "%s %s c = %d, k = %#x, half %d (sub %#x, flip %d), term %d: window %d is %r, the model says %r" % (
                name, "GLV" if glv else "plain", cbits, k, h, sub, flip, h * npad + term_index, w, tuple(got[h][w]), want[w])
    return None
