"""The host leg of the device tier of the Groth16 verifier's arithmetic: the Fq2 operations through the Fq2 machine's ALU, the Fq12 tower and
the machine's chains (fq2vm::run_host), applied on the host to raw limbs at the bounds tests/test_fq_bounds.py proves, against oracle/py
bigints (tests/devtier_pairing_cases.py).  No GPU; tests/test_gpu_devtier_pairing.py runs the same cases on the device."""
import ctypes

import numpy as np
import pytest

import devtier_pairing_cases as PC
from devtier_pairing_cases import BN, GEN, PQ

# ---- the bigint meaning of what a chain leaves: shared with the device leg, which applies the same functions to the device's buffers


@pytest.fixture(scope="module")
def lib():
    return PC.load()


@pytest.fixture(scope="module")
def scn():
    return PC.Scenario()


@pytest.mark.parametrize("op", PC.PAIRING_OPS, ids=lambda op: op.id)
def test_host_leg(lib, op):
    cases = PC.cases_of(op)
    PC.DC.CHECK[op.fam](op, cases, PC.run(lib, op, cases, 0))


def test_case_lists():
    for op in PC.FQ2_OPS:
        assert len(PC.cases_of(op)) >= PC.DC.N_RANDOM + 20, op.id
    long_ops = ("fq12_pow_x", "miller_loop", "final_exponentiation", "final_exponentiation_chain")
    for op in PC.F12_OPS:
        assert len(PC.cases_of(op)) == (PC.N_LONG if op.name in long_ops else PC.N_ARITH), op.id


def test_unknown_ops_and_chains_are_refused(lib):
    out = np.zeros(256, dtype=np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    for op in (0, PC.OPC["LDG"], PC.OPC["STG"], PC.OPC["LDC"], PC.OPC["LDK"], PC.OPC["STC"], PC.OPC["END"], 31, 35):
        assert lib.devtier_fq2(op, 1, p, p, p, p, 0) == -1
    assert lib.devtier_fq12(len(PC.F12_NAMES), 1, p, p, p, p, 0) == -1
    assert lib.devtier_fq2vm(5, 1, p, p, 0) == -1 and lib.devtier_fq2vm(0, 0, p, p, 0) == -1 and lib.devtier_fq2vm(2, 1, p, None, 0) == -1


def test_machine_geometry_is_the_generators(lib):
    """the slot numbers, the line table's size and the scripts' lengths of fq2vm_programs.h are those tools/gen_fq2vm.py computes"""
    sc = GEN.scripts()
    for chain, name in (("miller_a", "miller"), ("subgroup", "subgroup"), ("finish", "finish"), ("miller_b", "miller_b"), ("lines", "lines")):
        assert PC.vm_geom(lib, chain)["len"] == len(sc[name]), chain
    assert PC.vm_geom(lib, "miller_a")["slots"] == GEN.N_SLOTS and PC.vm_geom(lib, "miller_b")["kwords"] == GEN.N_LINE_SLOTS * 20


def test_miller_a_host(lib, scn):
    PC.check_miller_a(scn, PC.run_miller_a(lib, scn, 33, 0))


def test_subgroup_host(lib):
    PC.check_subgroup(*PC.run_subgroup(lib, 33, 0))


def test_lines_and_miller_b_host(lib, scn):
    tab, _ = PC.lines_table(lib, scn.gamma, scn.delta)
    io = PC.run_miller_b(lib, scn, tab, 33, 0)
    PC.check_miller_b(scn, io)
    # an operand that ignored the cursor, or a table read in another order, gives another value: gamma's and delta's rows swapped
    swapped = PC.run_miller_b(lib, scn, tab[:, ::-1], 1, 0)
    assert PC.final_exp(PC.slot_f12(swapped, GEN.SLOT_F0, 0)) != PC.final_exp(PC.slot_f12(io, GEN.SLOT_F0, 0))


def test_finish_host(lib, scn):
    PC.check_finish(scn, *PC.run_finish(lib, scn, 33, 0))
