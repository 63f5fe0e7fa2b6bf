"""-m gpu: the two forms of the comb walk in fixed_base_mul (csrc/ecgpu_fixedmul.h) through ecgpu_batch_mul_base_dev, byte for byte
against the oracle.

A wave runs load / affine + affine / a loop of xyzz_madd while every active lane has a non-zero digit, and falls into the state
machine at the first window where some lane has a zero digit.  tests/fixed_trim_vectors.py builds, per curve and width, whole
waves that leave the fast path at every window — through one lane among 63 that would have stayed, and through all 64 — at
window 0, window 1 and both, folded scalars, one-window scalars, 0, 1, n - 1, the comb's corner scalars and the carry patterns.
(k256 and p256 run the fast path; p384 and bp256 keep the single loop — COMB_FAST_WALK — and pass the same scalars.)
Every table is pinned on an engine of its own (tests/test_gpu_comb_table.py does the same) and its width asserted.

The batch sizes 1, 63, 64, 65 and 257 (a partly filled wave, a partly filled block) are cut out of the same batch, at waves that
hold zero digits, and compared with the same oracle result."""
import numpy as np
import pytest

import comb_vectors as cv
import fixed_trim_vectors as ftv
import oracle_lib
import pyec
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu

CASES = [(name, w) for name in ftv.CURVES for w in ftv.widths(name)]
SIZES = (1, 63, 64, 65, 257)
STARTS = (0, 2 * ftv.WAVE, 3 * ftv.WAVE + 1)            # the wave with a lone zero at window 0; at window 1; inside the all-zero wave


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    oracle_lib.build()


def run_dev(eng, c, scal):
    n = scal.size // c.L
    d_k = eng.to_device(scal)
    d_p, d_f = eng.dev_alloc(n * 2 * c.L), eng.dev_alloc(max(n, 16))
    try:
        eng.mul_by_generator_dev(c.cid, d_k, n, d_p, d_f)
        return eng.to_host(d_p, n * 2 * c.L).reshape(n, 2 * c.L), eng.to_host(d_f, n)
    finally:
        for b in (d_k, d_p, d_f):
            b.free()


@pytest.mark.parametrize("curve,w", CASES)
def test_fast_path_and_every_fall_back(curve, w):
    c = pyec.CURVES[curve]
    ks = ftv.wave_batch(c, w, 0xF17ED000 + 64 * c.cid + w)
    scal = np.frombuffer(cv.enc(c, ks), np.uint8)
    want, winf = oracle_lib.batch_mul_base_mt(c.cid, scal)
    want = np.asarray(want, np.uint8).reshape(len(ks), 2 * c.L)
    winf = np.asarray(winf, np.uint8)
    assert winf.sum() == ks.count(0) >= 1
    eng = ecgpu_module().Engine(0)          # raises without the HIP extension / a gfx950 device: no fallback
    try:
        eng.set_base_window(c.cid, w)
        got, ginf = run_dev(eng, c, scal)
        info = eng.base_table_info(c.cid)
        assert info["window_bits"] == w, (curve, w, info)
        bad = np.flatnonzero((got != want).any(axis=1) | (ginf != winf))
        assert bad.size == 0, "%s w = %d: %d of %d differ, first: scalar %d (wave %d, lane %d) k = %#x, digits %s" % (
            curve, w, bad.size, len(ks), bad[0], bad[0] // 64, bad[0] % 64, ks[bad[0]], cv.recode(c, w, ks[bad[0]]))
        for start in STARTS:
            for n in SIZES:
                sub = scal.reshape(len(ks), c.L)[start:start + n].reshape(-1)
                got, ginf = run_dev(eng, c, sub)
                assert bytes(got) == bytes(want[start:start + n]) and bytes(ginf) == bytes(winf[start:start + n]), (curve, w, start, n)
        assert eng.base_table_info(c.cid)["window_bits"] == w
    finally:
        eng.close()
