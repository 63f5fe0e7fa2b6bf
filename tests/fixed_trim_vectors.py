"""Scalars for the two forms of the comb walk in fixed_base_mul (csrc/ecgpu_fixedmul.h), shared by tests/test_gpu_fixed_trim.py
(gfx950) and tests/test_hostcheck_fixed_trim.py (the g++ twin).  Plain module, seeded, every comparison made with it is exact.

A wave stays on the fast path (load, affine + affine, then xyzz_madd in a loop) while every active lane has a non-zero digit; the
first zero digit on any lane sends the whole wave to the state machine at that window.  The scalars are therefore built from their
signed digit strings (tests/comb_vectors.py `recode` is the model of the recoding and every scalar emitted here is checked against
it), and the batches are laid out in groups of 64 consecutive scalars — the lanes of one wave."""
import random

import comb_vectors as cv
from gpu_common import comb_corner_scalars

WAVE = 64
CURVES = ("k256", "p256", "p384", "bp256")                 # bp256: COMB_NEEDS_CHECK
FIXED_WIDTHS = (5, 15, 17)


def widths(name):
    return tuple(sorted(set(FIXED_WIDTHS) | set(cv.WIDTHS[name])))


def scalar_of(c, w, digits):
    """The unfolded scalar with exactly this signed digit string."""
    k = sum(d << (w * j) for j, d in enumerate(digits))
    assert 0 < k < cv.unfolded_limit(c), (c.name, w, digits)
    assert cv.recode(c, w, k) == (False, list(digits)), (c.name, w, digits)
    return k


def _settle(c, w, d):
    """Makes the digit string of a valid unfolded scalar out of d by touching only the signs / sizes of its top non-zero digits:
    the value must be positive and below min(n, 2^(32 N - 1))."""
    nwin = len(d)
    reach = cv.reachable(c, w)[nwin - 1]
    live = [j for j in range(nwin) if d[j]]
    assert live
    t = live[-1]
    if t == nwin - 1:
        if reach >= 2:
            d[t] = 1 + abs(d[t]) % (reach - 1)             # 1 .. reach - 1: whatever lies below, the sum stays under the limit
        else:
            assert len(live) >= 2
            d[t] = 1                                        # the carry alone: the digit below must be negative
            d[live[-2]] = -abs(d[live[-2]])
            if abs(d[live[-2]]) == 1 << (w - 1):
                d[live[-2]] += 1                            # -2^(w-1) is not a digit
    else:
        d[t] = abs(d[t])
    return d


def digit_string(c, w, rng, zeros=(), magnitude=None):
    """A digit string without zero digits except at the windows `zeros`."""
    nwin, half = cv.window_count(c, w), 1 << (w - 1)
    d = [rng.choice((-1, 1)) * (magnitude or rng.randrange(1, half)) for _ in range(nwin)]
    for z in zeros:
        d[z] = 0
    return _settle(c, w, d)


def carry_every_window(c, w, alternate_with_zero=False):
    """Raw windows equal to 2^(w-1) above a window 0 of 2^(w-1) + 1: window 0 starts a carry and every window above, 2^(w-1) plus
    the carry, hands it on (digit 2^(w-1) + 1 - 2^w < 0) up to the first window that holds nothing but the carry.  With
    alternate_with_zero every other raw window is 2^w - 1: that one plus the carry is 2^w, a ZERO digit that still carries."""
    nwin, half, full = cv.window_count(c, w), 1 << (w - 1), 1 << w
    lim = cv.unfolded_limit(c)
    k = 0
    for j in range(nwin - 1):
        raw = full - 1 if (alternate_with_zero and j % 2) else half + (j == 0)
        k |= raw << (w * j)
    while k >= lim:
        k >>= w                                             # drop top windows until the value is a valid unfolded scalar
    k |= 1                                                  # (window 0 again after a drop)
    flip, digits = cv.recode(c, w, k)
    live = [j for j, x in enumerate(digits) if x]
    assert not flip and len(live) >= 2 and digits[live[-1]] == 1 and all(digits[j] < 0 for j in live[:-1]), (c.name, w, digits)
    if alternate_with_zero:
        assert all(digits[j] == 0 for j in range(1, live[-1], 2)), (c.name, w, digits)
    else:
        assert live == list(range(live[-1] + 1)), (c.name, w, digits)
    return k


def half_digits(c, w, alternate_with_zero=False):
    """Digits equal to +2^(w-1), the largest digit: a raw window of 2^(w-1) is the last value that is NOT carried."""
    nwin, half = cv.window_count(c, w), 1 << (w - 1)
    d = [0 if (alternate_with_zero and j % 2) else half for j in range(nwin - 1)] + [0]
    return scalar_of(c, w, d)


def special_scalars(c, w, brief=False):
    """k = 0, 1, n - 1, one non-zero window only (every window; digits 1, 2^(w-1) - 1, 2^(w-1) and their negatives through n - k,
    or 2^(w-1) alone if `brief`), the comb's corner scalars, and the carry patterns."""
    nwin, half = cv.window_count(c, w), 1 << (w - 1)
    ks = [0, 1, c.n - 1]
    R = cv.reachable(c, w)
    for j in range(nwin):
        for e in ((half,) if brief else (1, half - 1, half)):
            if e <= R[j]:
                k = e << (w * j)
                ks += [k] if brief else [k, c.n - k]
    ks += comb_corner_scalars(c, w)
    ks += [carry_every_window(c, w), carry_every_window(c, w, True), half_digits(c, w), half_digits(c, w, True)]
    ks += [c.n - k for k in ks[-4:]]
    return ks


def zero_sets(c, w):
    """The windows that hold the zero digit(s) of one scalar: every single position, and windows 0 and 1 together."""
    nwin = cv.window_count(c, w)
    return [(z,) for z in range(nwin)] + ([(0, 1)] if nwin > 2 else [])


def host_scalars(c, w, seed):
    """One lane at a time (the CPU twin has no wave): a scalar per zero set, both signs of the fold, and the special scalars."""
    rng = random.Random(seed)
    ks = [scalar_of(c, w, digit_string(c, w, rng)) for _ in range(4)]
    for zs in zero_sets(c, w):
        k = scalar_of(c, w, digit_string(c, w, rng, zs))
        ks += [k, c.n - k]
    return ks + special_scalars(c, w, brief=True)


def wave_batch(c, w, seed):
    """Whole waves, one after the other:
         for every zero set: a wave of non-zero digit strings with ONE lane (a different one each time) holding the zeros,
                             and a wave whose 64 lanes all hold them;
         one wave of folded scalars (n - k: the same digits, every sign flipped) with a zero lane in it;
         the special scalars, padded to whole waves with non-zero digit strings.
    Returns the list of scalars; its length is a multiple of 64."""
    rng = random.Random(seed)
    pool = [digit_string(c, w, rng) for _ in range(WAVE)]              # 64 strings without a zero digit
    fillers = [scalar_of(c, w, d) for d in pool]

    def with_zeros(d, zs):
        d = list(d)
        for z in zs:
            d[z] = 0
        return scalar_of(c, w, _settle(c, w, d))
    ks = []
    for i, zs in enumerate(zero_sets(c, w)):
        lane = (7 * i + 3) % WAVE
        wave = list(fillers)
        wave[lane] = with_zeros(pool[lane], zs)
        ks += wave
        ks += [with_zeros(d, zs) for d in pool]
    wave = [c.n - k for k in fillers]
    wave[17] = c.n - with_zeros(pool[17], (cv.window_count(c, w) // 2,))
    ks += wave
    sp = special_scalars(c, w)
    ks += sp + fillers[: -len(sp) % WAVE]
    assert len(ks) % WAVE == 0
    return ks
