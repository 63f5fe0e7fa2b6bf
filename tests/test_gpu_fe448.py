"""csrc/ecgpu_fe448.h on gfx950: the vectors of tests/fe448_vectors.py through ecgpu_selftest_fe448, every op, limb for limb against
the g++ twin's output for the same rows (tests/hostcheck_x448; tests/test_hostcheck_x448.py holds the twin against Python integers)."""
import ctypes

import numpy as np
import pytest

import fe448_vectors as fv
from gpu_common import ecgpu_module
from test_hostcheck_x448 import twin_fe448

pytestmark = pytest.mark.gpu
ERR_ARG = -7


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    yield e
    e.close()


def device(eng, op, rows):
    a = np.array(fv.flat(rows, 1), np.uint32)
    fb = fv.flat(rows, 2)
    return eng.selftest_fe448(op, a, None if fb is None else np.array(fb, np.uint32))


@pytest.mark.parametrize("op", range(9), ids=fv.OP_NAMES)
def test_every_op_limb_for_limb_against_the_twin(eng, op):
    rows = fv.rows(op)
    got, want = device(eng, op, rows), twin_fe448(op, rows)
    bad = [rows[i][0] for i in range(len(rows)) if not np.array_equal(got[i], want[i])]
    assert not bad, (fv.OP_NAMES[op], bad[:8])


def test_more_rows_than_a_block_and_one_row(eng):
    rows = (fv.rows(fv.MUL) * 3)[:257]                                   # 64 lanes per block: five blocks, the last with one lane
    assert np.array_equal(device(eng, fv.MUL, rows), twin_fe448(fv.MUL, rows))
    assert np.array_equal(device(eng, fv.SQR, fv.rows(fv.SQR)[:1]), twin_fe448(fv.SQR, fv.rows(fv.SQR)[:1]))


def test_argument_errors(eng):
    lib = eng._lib
    b = np.zeros(64, np.uint8)
    p = b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.ecgpu_selftest_fe448(eng._ctx, 9, p, p, ctypes.c_size_t(1), p) == ERR_ARG       # unknown op
    assert lib.ecgpu_selftest_fe448(eng._ctx, -1, p, p, ctypes.c_size_t(1), p) == ERR_ARG
    assert lib.ecgpu_selftest_fe448(eng._ctx, 0, None, p, ctypes.c_size_t(1), p) == ERR_ARG
    assert lib.ecgpu_selftest_fe448(eng._ctx, 0, p, p, ctypes.c_size_t(1), None) == ERR_ARG
    assert lib.ecgpu_selftest_fe448(eng._ctx, 0, None, None, ctypes.c_size_t(0), None) == 0      # n = 0
    assert eng.selftest_fe448(fv.SQR, np.zeros(0, np.uint32)).shape == (0, 16)
