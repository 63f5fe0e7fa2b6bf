"""Inputs for the tests of k_normalize's per-point work (tests/test_gpu_normalize_trim.py on gfx950, tests/test_normalize_trim_twin.py
on the g++ twin).  Plain module, seeded; every comparison made with it is exact.

  identity_records / wire_records   wire records X || Y || Z for the two entry points, with Z = 0 at chosen positions of the lanes' chains
  zero_test_limbs                   Z as LIMBS for raw point op 19 (csrc/ecgpu_selftest_point_raw.h): the identity test of the forward
                                    pass, Field::is_zero_short, beside Field::is_zero — what a wire record cannot carry: the limbs of
                                    tests/point_vectors.py (imported: limbs at the magnitude limits, the identity spelt 0 and p) and, for
                                    k256, every multiple of p that magnitude-1 limbs can hold in canonical and shifted limb splits, its
                                    neighbours, the limb extremes, a top limb at and above 2^24 (the fold) and random limbs"""
import random

import numpy as np

import comb_vectors as cv
import point_vectors as pv
from field_vectors import layout


def identity_records(n):
    """Where the degenerate records of a call on n records go: a sorted list of record indices.  n = 1: the one record."""
    T = cv.normalize_lanes(n)[1]
    chain = lambda t: list(range(t, n, T))
    pick = set()
    if n == 1:
        return [0]
    pick.add(chain(3)[0])                      # first of its chain
    pick.add(chain(4)[-1])                     # last
    if len(chain(5)) >= 3:
        pick.add(chain(5)[1])                  # in the middle
    pick.update(chain(6))                      # the whole chain
    pick.add(chain(T - 1)[0])                  # the last lane: at 65,537 and 131,073 it owns fewer records than lane 0
    pick.update(chain(t)[0] for t in range(64, 128))      # all 64 lanes of a wave, first records
    pick.update(chain(t)[-1] for t in range(128, 192))    # ... and the last records of another wave
    return sorted(pick)


def wire_records(c, n, seed, identities=True):
    """(n, 3 L) records X || Y || Z: the small-value combinations, the point vectors' values, random; Z = 0 at identity_records(n)
    unless identities is False (then the small-value combinations with Z = 0 are left out too)"""
    assert c.p >> (8 * c.L - 1) == 1 and not c.le
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, 256, (n, 3, c.L), dtype=np.uint8)
    rec[:, :, 0] &= 0x7F                                         # below p: the top bit clear (p has it set)
    enc = lambda v: np.frombuffer(int(v).to_bytes(c.L, c.order), np.uint8)
    special = [(x, y, z) for z in (1, c.p - 1, 0) for x in (0, 1, c.p - 1) for y in (0, 1, c.p - 1) if identities or z]
    lay = layout(c.name)
    S = pv.get_set(c.name)
    P, _ = pv.arrays(S, pv.vectors(c.name)[0][11])               # the XYZZ accumulators of op 11: slots x, y, zz, zzz of NL limbs
    for row in P[:: max(1, len(P) // 96)]:
        vals = [sum(int(row[s * lay.nl + i]) << (lay.b * i) for i in range(lay.nl)) % c.p for s in range(3)]
        if identities or vals[2]:
            special.append(tuple(vals))
    at = np.linspace(200, n - 1, len(special)).astype(int) if n > 400 + len(special) else np.arange(min(n, len(special)))
    for j, (x, y, z) in zip(at, special):
        rec[j, 0], rec[j, 1], rec[j, 2] = enc(x), enc(y), enc(z)
    if identities:
        rec[identity_records(n), 2] = 0
    return rec.reshape(n, 3 * c.L)


def zero_test_limbs(name, seed=0x4E0D):
    """(records, expected): uint32 records of four slots of NL limbs for raw point op 19 — only slot 2, Z, is read — and whether the
    value those limbs stand for is 0 modulo p.  Every limb set is one the magnitude-1 type allows (limbs up to LB; on the Montgomery
    sets the imported vectors only, which respect their top-limb bound)."""
    S = pv.get_set(name)
    c, lay = S.c, layout(name)
    nl, b = lay.nl, lay.b
    zs = []
    vecs = pv.vectors(name)[0]
    for op in (0, 4, 17):                                         # homogeneous P: slot 2 is Z, with the identity spellings 0Y0 .. pYp
        P, _ = pv.arrays(S, vecs[op])
        zs += [[int(x) for x in row[2 * nl: 3 * nl]] for row in P]
    for op in (11, 14):                                           # XYZZ: ZZ and ZZZ at value magnitude JV are NOT magnitude 1: X, Y only
        P, _ = pv.arrays(S, vecs[op])
        zs += [[int(x) for x in row[s * nl: (s + 1) * nl]] for row in P[::4] for s in (0, 1)]
    zs = [z for z in zs if S.mag_ok(z, 1, 1)]                     # check_mag<1, 1>: what m(Z) may hold
    imported = len(zs)
    assert imported >= 200, (name, imported)
    if name == "k256":
        rng = random.Random(seed)
        mask, lb = (1 << b) - 1, S.LB
        zs += [[lb] * 9, [0] * 9, [mask] * 9, [lb] * 8 + [0], [0] * 8 + [lb], [0] * 8 + [1 << 24], [mask] * 8 + [(1 << 24) - 1],
               [mask] * 8 + [1 << 24]]
        for mult in range(34):
            for d in (-2, -1, 0, 1, 2):
                v = mult * c.p + d
                if v < 0:
                    continue
                a = [(v >> (b * i)) & mask for i in range(8)] + [v >> (b * 8)]
                if a[8] <= lb:
                    zs.append(a)
                for i in range(8):                               # the same value with one unit of limb i + 1 moved down into limb i
                    if a[i + 1] > 0 and a[i] + (1 << b) <= lb and a[8] <= lb:
                        s = list(a)
                        s[i + 1] -= 1
                        s[i] += 1 << b
                        zs.append(s)
        for _ in range(3000):
            zs.append([rng.randrange(lb + 1) for _ in range(9)])
            zs.append([rng.choice([0, 1, mask, mask + 1, lb, rng.randrange(lb + 1)]) for _ in range(9)])
    rec = np.zeros((len(zs), 4 * nl), np.uint32)
    rec[:, 2 * nl: 3 * nl] = np.array(zs, dtype=np.uint64).astype(np.uint32)
    want = np.array([sum(x << (b * i) for i, x in enumerate(z)) % c.p == 0 for z in zs])
    assert want[:imported].sum() >= 8 and (~want[:imported]).sum() >= 100, (name, int(want[:imported].sum()))
    if name == "k256":
        plimbs = [0x1FFFFC2F, 0x1FFFFFF7] + [mask] * 6 + [0xFFFFFF]
        assert plimbs in zs and [0] * 9 in zs and want.sum() >= 60 and any(w and z[8] >> 24 for w, z in zip(want, zs))
    return rec, want
