"""-m gpu: the adversarial coordinates of tests/point_vectors.py on gfx950, through ecgpu_selftest_point_raw
(k_selftest_point_raw: Group<C>'s formulas and ct_dbl4 on raw limbs), all twelve parameter sets, one call per (set, op) with every
vector batched — the counts are what the generator gives, no multiples of the block size, so the tail guard runs.  Three checks
per vector: the class of the result against the model; the returned limbs against what the return type promises; and the limbs
bit for bit against the g++ twin's (both run the same integer algorithm — on k256 that sets the assembly reduction against the
C++ one at formula level): by the digests tests/test_point_vectors.py pins in tests/golden/point_vectors_twin.json, and by the
twin itself where a digest differs, to name the vector.  tests/test_point_vectors.py runs the same vectors through the twins alone, so a failure here alone is
the gfx950 rendering, and a failure in both is the source."""
import numpy as np
import pytest

import point_vectors as pv
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


def _run(eng, S, op, vs):
    P, Q = pv.arrays(S, vs)
    got = eng.selftest_point_raw(S.c.cid, op, P, Q)
    msg = pv.first_failure(S, op, vs, got)
    assert msg is None, msg
    if pv.digest(got) == pv.golden()[S.name][str(op)]:
        return                                                   # the twin's limbs, as tests/test_point_vectors.py pinned them
    import hostcheck_lib as hc                                   # a difference: the twin itself, to name the vector
    twin = hc.point_raw(S.c.cid, op, P, Q)
    assert not np.array_equal(got, twin), "%s op %d: tests/golden/point_vectors_twin.json is not the twin's output" % (S.name, op)
    i = int(np.nonzero((got != twin).any(axis=1))[0][0])
    raise AssertionError("%s op %d: device and g++ twin differ at %d (%s): %s / %s" % (
        S.name, op, i, vs[i].tag, [hex(int(w)) for w in got[i]], [hex(int(w)) for w in twin[i]]))


@pytest.mark.parametrize("curve", pv.CURVES)
def test_device_point_formulas_on_adversarial_limbs(eng, curve):
    """ops 0 - 14 and 17 on families A - E, every vector of the set"""
    S = pv.get_set(curve)
    vecs, _ = pv.vectors(curve)
    assert sum(1 for o in vecs if len(vecs[o]) % 256) >= 15                  # the last workgroup is a partial one
    for op in sorted(o for o in vecs if o & 0xFF not in (15, 16)):
        _run(eng, S, op, vecs[op])


@pytest.mark.parametrize("curve", pv.CURVES)
def test_device_chains_and_single_record(eng, curve):
    """dbl(add(acc, Q)) and the ladder step (four jac_dbl, one jac_madd) at 1, 4 and 16 steps; n = 1 once per set"""
    S = pv.get_set(curve)
    vecs, _ = pv.vectors(curve)
    assert sorted(o >> 8 for o in vecs if o >> 8) == sorted(2 * pv.CHAIN_STEPS)
    for op in sorted(o for o in vecs if o & 0xFF in (15, 16)):
        _run(eng, S, op, vecs[op])
    P, Q = pv.arrays(S, vecs[0])                                              # one record, one lane: the first row of the batch
    assert np.array_equal(eng.selftest_point_raw(S.c.cid, 0, P[:1], Q[:1]), eng.selftest_point_raw(S.c.cid, 0, P, Q)[:1])


def test_device_raw_point_op_range(eng):
    ecgpu = ecgpu_module()
    S = pv.get_set("p256")
    P, Q = pv.arrays(S, pv.vectors("p256")[0][0][:3])
    for op in (18, 99, 255, 4 | 1 << 8, 15 | 65 << 8):
        with pytest.raises(ecgpu.EcgpuError) as e:
            eng.selftest_point_raw(S.c.cid, op, P, Q)
        assert e.value.code == ecgpu.ERR_SCALAR_RANGE
    with pytest.raises(ecgpu.EcgpuError) as e:
        eng.selftest_point_raw(S.c.cid, 0, P[:, :-1], None)
    assert e.value.code == ecgpu.ERR_ARG
