"""The device leg of the device tier of the Groth16 verifier's arithmetic: the cases of tests/test_devtier_pairing.py with one lane per case on
code compiled for gfx950 with the product's flags, and every chain of the Fq2 machine in ONE launch of the product's own kernel (libzkp_hip.so's
k_fq2vm through g16_vm_launch_chain) against the host interpreter, word for word over the whole slot buffer.  A device result must first equal
the host build's (a divergence is a code-generation or interpreter finding and is reported as chain, envelope, slot, word) and then meet the
bigint reference.  Needs no zkp_hip_init and no keys."""
import os
import subprocess
import sys

import numpy as np
import pytest

import devtier_pairing_cases as PC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return PC.load()


@pytest.fixture(scope="module")
def scn():
    return PC.Scenario()


@pytest.mark.parametrize("op", PC.PAIRING_OPS, ids=lambda op: op.id)
def test_device_leg(lib, op):
    cases = PC.cases_of(op)
    host = PC.run(lib, op, cases, 0)
    dev = PC.run(lib, op, cases, 1)
    diff = np.nonzero((host != dev).any(axis=1))[0]
    assert diff.size == 0, "%s: device and host builds differ in %d cases, first: case %d, words %r -> host %r device %r" % (
        op.id, diff.size, diff[0], np.nonzero(host[diff[0]] != dev[diff[0]])[0].tolist(), host[diff[0]].tolist(), dev[diff[0]].tolist())
    PC.DC.CHECK[op.fam](op, cases, dev)


def _same(chain, host, dev):
    msg = PC.vm_diff(chain, host, dev)
    assert msg is None, msg


@pytest.mark.parametrize("n", PC.VM_SIZES)
def test_miller_a(lib, scn, n):
    host, dev = PC.run_miller_a(lib, scn, n, 0), PC.run_miller_a(lib, scn, n, 1)
    _same("miller_a", host, dev)
    PC.check_miller_a(scn, dev)


@pytest.mark.parametrize("n", PC.VM_SIZES)
def test_subgroup(lib, n):
    host, pts, outside = PC.run_subgroup(lib, n, 0)
    dev = PC.run_subgroup(lib, n, 1)[0]
    _same("subgroup", host, dev)
    PC.check_subgroup(dev, pts, outside)


@pytest.mark.parametrize("n", PC.VM_SIZES)
def test_lines(lib, scn, n):
    """chain L (the product runs it on the host, once per key) on the device: the line tables of n points; their meaning is chain B's test"""
    pts = ([scn.gamma, scn.delta] + scn.B)[:n]
    _same("lines", PC.run_lines(lib, pts, 0), PC.run_lines(lib, pts, 1))


@pytest.mark.parametrize("n", PC.VM_SIZES)
def test_miller_b(lib, scn, n):
    tab_dev, _ = PC.lines_table(lib, scn.gamma, scn.delta, 1)                 # the table itself from the device's chain L
    tab, _ = PC.lines_table(lib, scn.gamma, scn.delta, 0)
    assert (tab == tab_dev).all()
    host, dev = PC.run_miller_b(lib, scn, tab, n, 0), PC.run_miller_b(lib, scn, tab_dev, n, 1)
    _same("miller_b", host, dev)
    PC.check_miller_b(scn, dev)


@pytest.mark.parametrize("n", PC.VM_SIZES)
def test_finish(lib, scn, n):
    host, inp, k = PC.run_finish(lib, scn, n, 0)
    dev = PC.run_finish(lib, scn, n, 1)[0]
    _same("finish", host, dev)
    PC.check_finish(scn, dev, inp, k)


CHILD = """
import sys
import numpy as np
import devtier_pairing_cases as PC
np.save(sys.argv[1], PC.run_miller_a(PC.load(), PC.Scenario(n=33, seed=10), 33, 1))
"""


def test_register_file_holds_nothing_between_launches(lib, tmp_path):
    """Chain A twice in this process on different inputs: the second result equals that of a process that ran it alone, so nothing depends on what
    an earlier launch left in LDS.  The other process is a fresh child, started normally."""
    first = PC.run_miller_a(lib, PC.Scenario(n=33, seed=9), 33, 1)
    second = PC.run_miller_a(lib, PC.Scenario(n=33, seed=10), 33, 1)
    assert (first != second).any()
    out = str(tmp_path / "alone.npy")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    subprocess.run([sys.executable, "-c", CHILD, out], check=True, cwd=ROOT, env=env, timeout=300)
    _same("miller_a", np.load(out), second)
