#!/usr/bin/env python3
"""Writes tests/modinv_search_constants.py: family S of tests/modinv_vectors.py, the inputs that push the traces of
tools/modinv_model.py to their extremes, for both moduli of all twelve parameter sets.

Seeded and step-bounded, so a second run writes the same file (`--check` compares instead of writing).  Per modulus:
  * the population is the RANDOM_COUNT seeded random inputs of modinv_vectors.random_inputs — the very inputs check_coverage takes
    its random baseline from, so no threshold can fall below the baseline — and families L and T;
  * for every extreme of modinv_vectors.S_EXTREMES: the PARENTS best of the population, then ROUNDS rounds of CHILDREN mutants per
    parent (one to three bits flipped, or +- 2^k, mod m), the best PARENTS of parents and children kept; the best input and the figure
    it reaches (the threshold) are recorded;
  * for every state of modinv_vectors.S_STATES: the first input of the population that shows it, else the first among ROUNDS rounds of
    mutants of the inputs nearest to it; a state nobody shows is an error.

    python tools/modinv_search.py [--check] [--jobs N]            (no GPU; a few minutes on one core)
"""
import argparse
import os
import random
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import modinv_vectors as mv                                                   # noqa: E402
mm = mv.mm

PARENTS, CHILDREN, ROUNDS = 48, 16, 5
OUT = os.path.join(ROOT, "tests", "modinv_search_constants.py")


def mutate(rng, x, m):
    bits = m.bit_length()
    kind = rng.randrange(3)
    if kind == 0:
        for _ in range(rng.randrange(1, 4)):
            x ^= 1 << rng.randrange(bits)
    elif kind == 1:
        x += rng.choice((-1, 1)) << rng.randrange(bits)
    else:
        k = 30 * rng.randrange((bits + 29) // 30)                             # one limb of the inversion re-drawn
        x = (x & ~(mm.M30 << k)) | (rng.randrange(1 << 30) << k)
    return x % m


def run_form(name, which, form, xs):
    m = mv.modulus(name, which)
    if form == "ct":
        return mm.invert(xs, m, mv.nw(name), check_result=False)[1]
    return mm.invert_var(xs, m, mv.nw(name), wave=1, check_result=False)[1]


def search(job):
    name, which = job
    m = mv.modulus(name, which)
    rng = random.Random(mv.seed(name, which, 0x5EA7C4))
    pop = list(dict.fromkeys(mv.random_inputs(name, which) + mv.family_l(name, which) + mv.family_t(name, which)))
    tr = mv.traces(name, which, pop)
    out = {}
    for goal, (form, fig) in sorted(mv.S_EXTREMES.items()):
        figs = fig(tr[form])
        order = np.argsort(-figs, kind="stable")[:PARENTS]
        best = [(float(figs[j]), pop[j]) for j in order]
        for _ in range(ROUNDS):
            kids = list(dict.fromkeys(mutate(rng, x, m) for _, x in best for _ in range(CHILDREN)))
            kf = fig(run_form(name, which, form, kids))
            best = sorted(set(best + [(float(v), x) for v, x in zip(kf, kids)]), key=lambda t: (-t[0], t[1]))[:PARENTS]
        out[goal] = (best[0][1], best[0][0])
    for goal, (form, pred) in sorted(mv.S_STATES.items()):
        hit = np.nonzero(pred(tr[form]))[0]
        if len(hit):
            out[goal] = (pop[int(hit[0])], None)
            continue
        seeds = pop[-256:]
        for _ in range(ROUNDS * 4):
            kids = list(dict.fromkeys(mutate(rng, x, m) for x in seeds for _ in range(CHILDREN)))
            hit = np.nonzero(pred(run_form(name, which, form, kids)))[0]
            if len(hit):
                out[goal] = (kids[int(hit[0])], None)
                break
            seeds = kids[:256]
        else:
            raise SystemExit("%s %s: no input shows the state '%s'" % (name, which, goal))
    return name, which, out


def render(results):
    lines = ['"""Family S of tests/modinv_vectors.py: written by tools/modinv_search.py, which reproduces it.  Do not edit.',
             "FAMILY_S[set][modulus][goal] = (input, the figure the search reached with it — None for a state)\"\"\"",
             "FAMILY_S = {"]
    for name in mv.CURVES:
        lines.append('    "%s": {' % name)
        for which in mv.WHICH:
            lines.append('        "%s": {' % which)
            for goal, (x, thr) in sorted(results[(name, which)].items()):
                lines.append('            "%s": (%#x, %r),' % (goal, x, thr))
            lines.append("        },")
        lines.append("    },")
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    ap.add_argument("--jobs", type=int, default=1)
    a = ap.parse_args()
    mm.check_header_constants()
    if a.jobs > 1:
        with ProcessPoolExecutor(a.jobs) as ex:
            done = list(ex.map(search, mv.MODULI))
    else:
        done = [search(j) for j in mv.MODULI]
    text = render({(n, w): o for n, w, o in done})
    if a.check:
        same = open(OUT).read() == text
        print("modinv search reproduces tests/modinv_search_constants.py: %s" % same)
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote %s: %d moduli, %d goals each" % (os.path.relpath(OUT, ROOT), len(done), len(done[0][2])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
