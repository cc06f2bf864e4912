"""The device tier's device leg: the cases of tests/test_devtier_math.py with one lane per case, one launch per op, on code compiled for
gfx950 with the product's flags.  The device result must equal the host leg's limb for limb (so a divergence between the two compilers is
reported as such) and then meet the bigint reference.  Needs no zkp_hip_init, no generator tables and no keys."""
import numpy as np
import pytest

import devtier_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return DC.load()


@pytest.mark.parametrize("op", DC.ALL_OPS, ids=lambda op: op.id)
def test_device_leg(lib, op):
    cases = DC.cases_of(op)
    host = DC.run(lib, op, cases, 0)
    dev = DC.run(lib, op, cases, 1)
    diff = np.nonzero((host != dev).any(axis=1))[0]
    assert diff.size == 0, "%s: device and host builds differ in %d cases, first: %r -> host %r device %r" % (
        op.id, diff.size, cases[diff[0]], host[diff[0]].tolist(), dev[diff[0]].tolist())
    DC.CHECK[op.fam](op, cases, dev)
