"""-m gpu: the adversarial limb-level vectors of tests/field_vectors.py on gfx950, through ecgpu_selftest_field — families C
(canonical domain, k_selftest_field), R (raw domain at the magnitude limits, ops 30 - 39) and N (ScalarN, ops 40 - 44; both
k_selftest_field_raw), all twelve parameter sets, one call per (set, op) with every case batched.  Expected values are Python
integers, equality is exact; a mismatch reports the first differing index with its operands and both values.
tests/test_field_adversarial.py runs the same vectors through the g++ twin, so a failure here alone is the gfx950 compiler's
rendering (or the k256 assembly blocks), and a failure in both is the source.

As on the CPU these vectors do not reach the slack between 2^B - 1 and LB - 1 of a limb (operands enter with strict limbs);
tools/field_model.py covers it on the restatement and k256's op 15 below feeds reduced products back in."""
import numpy as np
import pytest

import field_vectors as fv
import pyec
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu

CURVES = fv.CURVES            # gpu_common.ALL_CURVES and bign256


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


def _arr(c, vals):
    return np.frombuffer(fv.enc(c, vals), np.uint8)


def _run(eng, c, fam):
    for op in sorted(fam):
        a, b, want = fam[op]
        got = fv.dec(c, eng.selftest_field(c.cid, op, _arr(c, a), _arr(c, b) if b is not None else None))
        msg = fv.first_mismatch(c, op, fam[op], got)
        assert msg is None, msg


@pytest.mark.parametrize("curve", CURVES)
def test_device_canonical_domain_structured_and_steered(eng, curve):
    c = pyec.CURVES[curve]
    fam = fv.family_c(curve)
    fv.check_coverage(curve, fam_c=fam)
    _run(eng, c, fam)


@pytest.mark.parametrize("curve", CURVES)
def test_device_raw_domain_at_the_magnitude_limits(eng, curve):
    c = pyec.CURVES[curve]
    fam = fv.family_r(curve)
    fv.check_coverage(curve, fam_r=fam)
    _run(eng, c, fam)


@pytest.mark.parametrize("curve", CURVES)
def test_device_scalars_mod_n(eng, curve):
    c = pyec.CURVES[curve]
    fam = fv.family_n(curve)
    fv.check_coverage(curve, fam_n=fam)
    _run(eng, c, fam)


def test_device_k256_assembly_blocks_and_row_parallel_field_on_raw_extremes(eng):
    """Family R's pairs through op 15 (7 a b + 7 a b by the assembly blocks AND the compiler's k_reduce from the same columns, the
    nine limbs compared on the device: a difference comes back as all-ones bytes) and op 16 (13 a b by the row-parallel field of
    ecgpu_rows.h: the operands in the first four lanes of each wave, the product of lane (i mod 4) in every lane i).  Both ops take
    canonical operands — for k256 the canonical words ARE the limbs — so of the raw pairs those with a member in [p, 2^256) stay
    with ops 30 - 39; the count that remains is asserted."""
    c = pyec.CURVES["k256"]
    p = c.p
    pairs = [(a, b) for a, b in fv.r_pairs("k256") if a < p and b < p]
    assert len(pairs) >= 650
    a = [x for x, _ in pairs]
    b = [y for _, y in pairs]
    entry = (a, b, [14 * x * y % p for x, y in pairs])
    msg = fv.first_mismatch(c, 15, entry, fv.dec(c, eng.selftest_field(c.cid, 15, _arr(c, a), _arr(c, b))))
    assert msg is None, msg
    while len(pairs) % 4:
        pairs.append(pairs[-1])
    la, lb, want = [], [], []
    for w in range(len(pairs) // 4):
        four = pairs[4 * w: 4 * w + 4]
        la += [x for x, _ in four] + [1] * 60                    # the other lanes' operands must not matter
        lb += [y for _, y in four] + [2] * 60
        want += [13 * x * y % p for x, y in four] * 16
    assert len(la) % 64 == 0
    msg = fv.first_mismatch(c, 16, (la, lb, want), fv.dec(c, eng.selftest_field(c.cid, 16, _arr(c, la), _arr(c, lb))))
    assert msg is None, msg


@pytest.mark.parametrize("curve", ["p256", "bign256"])
def test_device_selftest_op_ranges(eng, curve):
    """Ops 0 - 21 keep rejecting operands >= p, ops 30 - 44 take them, and an unknown op is a range error."""
    ecgpu = ecgpu_module()
    c = pyec.CURVES[curve]
    one, pp = _arr(c, [1]), _arr(c, [c.p])
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.selftest_field(c.cid, 0, one, pp)
    assert e.value.code == ecgpu.ERR_POINT
    assert fv.dec(c, eng.selftest_field(c.cid, 39, pp, one)) == [1]
    for op in (22, 29, 45, 99):
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.selftest_field(c.cid, op, one, one)
        assert e.value.code == ecgpu.ERR_SCALAR_RANGE
