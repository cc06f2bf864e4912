"""The Groth16 entry points of the device tier without a GPU: the Python geometry and references checked against DESIGN.md and against
themselves, the digit recodings' host leg (g16_recode at its nine forms, sc_recode_signed_rt at the ed25519 radices) at their bounds, the
planner's step list against the geometry, and the arguments the harness refuses before it launches anything.
tests/test_gpu_devtier_g16.py runs the device legs."""
import ctypes

import numpy as np
import pytest

import devtier_g16_cases as GC
from oracle.py import bn254 as BN


@pytest.fixture(scope="module")
def lib():
    return GC.DC.load()


def test_geometry_is_the_one_design_md_states():
    even, uneven = GC.geom(14), GC.geom(14, True)
    assert (even.nwin, even.slot_ent, even.digw, even.nwin_u64) == (19, 155648, 10, 5)
    assert (uneven.nwin, uneven.slot_ent, uneven.digw, uneven.nwin_u64) == (18, 172544, 9, 5)
    assert uneven.bit[16:] == [224, 239] and uneven.off[16:] == [16 * 8192, 18 * 8192] and uneven.ent[16:] == [16384, 25088]
    assert [GC.geom(w).nwin for w in range(8, 16)] == [32, 29, 26, 24, 22, 20, 19, 17]
    assert GC.geom(8).slot_ent == 32 * 128 and GC.geom(15).slot_ent == 278528 and GC.geom(10).nwin_u64 == 7
    assert [f.g.nwin for f in GC.FORMS[9:]] == [24, 22, 20, 19, 17]        # ed25519, radix 2^11 .. 2^15: scalars below l < 2^253
    for f in GC.FORMS:
        g = f.g
        assert g.bit[-1] + g.width[-1] >= (g.q - 1).bit_length() + (0 if g.uneven else 1) and g.digw <= GC.DIGW_MAX


@pytest.mark.parametrize("fm", GC.FORMS, ids=lambda f: f.id)
def test_the_reference_recoding_stays_inside_its_caps(fm):
    """conditions on the reference alone, before the product is asked: no carry leaves the top window, no digit passes its window's entries"""
    xs = GC.scalars_of(fm.id)
    assert len(xs) >= GC.N_RANDOM + 40 and all(0 <= x < fm.g.q for x in xs)
    top = GC.check_reference_caps(fm, xs)
    if fm.g.uneven:
        assert GC.recode(BN.R - 1, fm.g)[0][-1] == top == 24777 and top <= 24784 <= fm.g.ent[-1] == 25088
        assert all(GC.recode(x, fm.g)[0][-1] >= 0 for x in xs)
    if fm.id == "g16_recode_w15":
        assert top == 12388 <= 16384


@pytest.mark.parametrize("fm", GC.FORMS, ids=lambda f: f.id)
def test_recoding_host_leg(lib, fm):
    xs = GC.scalars_of(fm.id)
    GC.check_digits(fm, xs, GC.run_digits(lib, fm, xs, 0))


def test_table_references_agree_with_scalar_multiplication():
    """the chain and the sampled route against (i + 1) 2^bit(w) m G as one integer multiple of the generator, and against each other"""
    for g2, wbits, uneven, slot in ((0, 8, False, 1), (1, 8, False, 2)):
        g, (c, gen) = GC.geom(wbits, uneven), GC.curve(g2)
        ref = GC.slot_reference(g2, slot, wbits, uneven)
        for w, i in ((0, 0), (0, 1), (3, 127), (g.nwin - 1, 5), (g.nwin - 1, 127), (17, 64)):
            want = c.mul_pt(gen, (i + 1) * (1 << g.bit[w]) * GC.base_mult(slot))
            assert ref[g.off[w] + i].tolist() == GC.pt_words(g2, want).tolist(), (g2, w, i)
    g = GC.geom(11)                                                          # two builder segments per window
    idx = GC.sample_indices(g, 5)
    assert {(0, 0), (0, 1), (0, 7), (0, 8), (0, 511), (0, 512), (0, 1023), (23, 512), (23, 1023)} <= set(idx) and len(idx) == 24 * 2 * 5 + 256
    full = GC.slot_reference(0, 1, 11, False)
    assert (GC.sample_reference(0, 1, g, idx) == full[[g.off[w] + i for w, i in idx]]).all()
    gu = GC.geom(14, True)
    idx = [(16, 0), (16, 16383), (17, 0), (17, 24776), (17, 25087)]
    got = GC.sample_reference(0, 1, gu, idx)
    for row, (w, i) in zip(got, idx):
        assert row.tolist() == GC.pt_words(0, BN.G1C.mul_pt(BN.G1, (i + 1) * (1 << gu.bit[w]) * GC.base_mult(1))).tolist()


def test_stored_form_checks_hold_the_classes():
    """the packed bound is the interval proof's, and the check refuses a coordinate at it"""
    for g2 in (0, 1):
        b = GC.packed_bound(g2)
        assert 2 * GC.DC.PQ < b <= 3 * GC.DC.PQ < 1 << 256
        ok = GC.to_words([b - 1] * (4 if g2 else 2)).reshape(1, -1)
        GC.check_stored_form(g2, 1, ok)
        with pytest.raises(AssertionError):
            GC.check_stored_form(g2, 1, GC.to_words([b] * (4 if g2 else 2)).reshape(1, -1))
    assert GC.packed_bound(0) * 10 < 24 * GC.DC.PQ                          # the kernel comment's "< 2.4 p"


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("fm", [GC.FORMS[i] for i in (0, 3, 6, 8, 7)], ids=lambda f: f.id)
def test_the_planner_s_steps_meet_the_geometry(lib, fm, chunks):
    """g16_plan_chunks + make_gather_steps for the two-slot launch: every step starts at the first entry of a window of the Python geometry
    and reads that window's digit half; no prefix sum of any row meets an exceptional case of the lazy additions"""
    steps, step0 = GC.plan(lib, fm.g, chunks)
    walk = GC.walk_of(fm.g, steps, step0)
    pairs = GC.row_pairs(fm)
    assert len(pairs) % GC.ROWS == 0 and {x for pr in pairs for x in pr} >= set(GC.pinned(fm.g))
    GC.assert_no_exceptional_case(fm.g, walk, step0.tolist(), pairs, (GC.base_mult(0), GC.base_mult(1)))


def test_the_harness_refuses_before_it_launches(lib):
    for wbits, uneven, nslots, rc in ((7, 0, 1, -1), (16, 0, 1, -1), (13, 1, 1, -1), (15, 1, 1, -1), (14, 2, 1, -1), (14, 1, 0, -2), (10, 0, 5, -2)):
        for g2 in (0, 1):
            for msm_form in (0, 1):
                GC.run_table(lib, g2, msm_form, wbits, uneven, nslots, expect_rc=rc)
    out = np.zeros(64, dtype=np.uint32)
    p = GC.ptr(out)
    assert lib.devtier_g16_table(0, 1, 8, 0, None, 1, p, p, p) == -3
    assert lib.devtier_g16_digits(14, 1, p, p, 0) == -1 and lib.devtier_g16_digits(-1, 1, p, p, 0) == -1 and lib.devtier_g16_digits(0, 0, p, p, 0) == -1
    assert lib.devtier_g16_plan(7, 0, 1, p, p) == -1 and lib.devtier_g16_plan(14, 0, 0, p, p) == -2 and lib.devtier_g16_plan(14, 1, 37, p, p) == -2
    u32 = ctypes.c_uint32
    assert lib.devtier_g16_fixed_mul(0, u32(16), u32(0), p, p, u32(1), u32(1), p, None, p) == -1
    assert lib.devtier_g16_fixed_mul(0, u32(13), u32(1), p, p, u32(1), u32(1), p, None, p) == -1
    assert lib.devtier_g16_fixed_mul(0, u32(14), u32(0), p, p, u32(0), u32(1), p, None, p) == -2
    assert lib.devtier_g16_fixed_mul(1, u32(14), u32(0), p, p, u32(1), u32(0), p, None, p) == -2
    assert lib.devtier_g16_fixed_mul(1, u32(14), u32(0), p, p, u32(1), u32(1), None, None, p) == -2
