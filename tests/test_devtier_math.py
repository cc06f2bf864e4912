"""The device tier's host leg: every field op of tests/devtier/devtier.hip, applied on the host to raw limbs at the bounds the headers
promise, against plain bigint references (tests/devtier_cases.py).  No GPU; tests/test_gpu_devtier_math.py runs the same cases in one
launch per op."""
import pytest

import devtier_cases as DC


@pytest.fixture(scope="module")
def lib():
    return DC.load()


@pytest.mark.parametrize("op", DC.ALL_OPS, ids=lambda op: op.id)
def test_host_leg(lib, op):
    cases = DC.cases_of(op)
    DC.CHECK[op.fam](op, cases, DC.run(lib, op, cases, 0))


def test_every_case_list_holds_the_fixed_patterns_and_the_random_draws():
    for op in DC.ALL_OPS:
        assert len(DC.cases_of(op)) >= DC.N_RANDOM + 20, op.id


def test_unknown_op_is_refused(lib):
    import ctypes
    import numpy as np
    out = np.zeros(64, dtype=np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    for fam in ("fe", "fq", "fq9", "fr9", "f128", "point", "sc", "fp", "ge"):
        assert getattr(lib, "devtier_" + fam)(99, 1, p, p, p, p, 0) == -1
