"""The Groth16 key tables, digit recodings and their join on the device (tests/devtier/devtier_g16.h, tests/devtier_g16_cases.py).

A. k_g16_build_table, the product's code object through g16_launch_build_table: every stored entry of a table read back and compared, as
   canonical affine words, with (i + 1) * 2^bit(w) * P_s in bigint curve arithmetic -- exact equality; the stored words held to the class
   the reader assumes; a guard behind the table untouched and no entry left unwritten.  Up to radix 2^11 three slots are checked at every
   entry.  From radix 2^13 up there are two slots: slot 0 (the generator) at every entry, slot 1 (a full-width multiple) SAMPLED at the
   first, second, eighth, ninth and last entry of every 512-entry segment of every window and at 256 seeded entries.
B. g16_recode at its nine forms and sc_recode_signed_rt at the ed25519 radices, one lane per scalar: word for word the host leg, and the
   bigint conditions of tests/test_devtier_g16.py.
C. builder, recoder (device), planner (g16_plan_chunks + make_gather_steps), k_msm_gather and k_sum_t in one chain against
   acc_init + s_0 P_0 + s_1 P_1.
Needs no zkp_hip_init, no keys and no generator tables.  Each test prints its reference and total wall time."""
import time

import numpy as np
import pytest

import devtier_g16_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return GC.DC.load()


# (g2, packed, wbits, uneven); the plain form is the verifier's gamma_abc_g1 tables, G1 at radix 2^10 -- the product builds no plain G2 table
TABLES = [(g2, 1, w, u) for g2 in (0, 1) for w, u in ((8, 0), (9, 0), (10, 0), (11, 0), (13, 0), (14, 0), (14, 1), (15, 0))] + [(0, 0, 10, 0)]


@pytest.mark.parametrize("g2,msm_form,wbits,uneven", TABLES, ids=["%s-%s-w%d%s" % ("G2" if t[0] else "G1", "packed" if t[1] else "plain", t[2], "u" if t[3] else "") for t in TABLES])
def test_every_entry_of_a_built_table(lib, g2, msm_form, wbits, uneven):
    nslots = 3 if wbits <= 11 else 2
    full = range(nslots) if wbits <= 11 else (0,)
    t0 = time.time()
    for s in full:
        GC.slot_reference(g2, s, wbits, bool(uneven))
    t1 = time.time()
    raw, aff, guard = GC.run_table(lib, g2, msm_form, wbits, uneven, nslots)
    GC.check_table(g2, msm_form, wbits, bool(uneven), nslots, raw, aff, guard, set(full))
    print("\ng16 table %s %s w%d%s: reference %.2f s, whole test %.2f s" % ("G2" if g2 else "G1", "packed" if msm_form else "plain", wbits, "u" if uneven else "", t1 - t0, time.time() - t0))


@pytest.mark.parametrize("fm", GC.FORMS, ids=lambda f: f.id)
def test_recoding_device_leg(lib, fm):
    xs = GC.scalars_of(fm.id)
    host, dev = GC.run_digits(lib, fm, xs, 0), GC.run_digits(lib, fm, xs, 1)
    diff = np.nonzero((host != dev).any(axis=1))[0]
    assert diff.size == 0, "%s: device and host builds differ in %d cases, first: %x -> host %r device %r" % (
        fm.id, diff.size, xs[diff[0]] if diff.size else 0, host[diff[0]].tolist() if diff.size else None, dev[diff[0]].tolist() if diff.size else None)
    GC.check_digits(fm, xs, dev)


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("fm", [GC.FORMS[i] for i in (0, 3, 6, 8, 7)], ids=lambda f: f.id)
@pytest.mark.parametrize("g2", [0, 1], ids=["G1", "G2"])
def test_builder_recoder_and_planner_meet(lib, g2, fm, chunks):
    t0 = time.time()
    pairs = GC.row_pairs(fm)
    GC.run_fixed_mul(lib, g2, fm, chunks, pairs)
    print("\ng16 fixed mul %s %s chunks %d: %d rows in launches of %d, %.2f s" % ("G2" if g2 else "G1", fm.id, chunks, len(pairs), GC.ROWS, time.time() - t0))
