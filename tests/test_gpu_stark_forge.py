"""The forged and mutated improvement envelopes of tests/stark_forge.py through the product on the MI355X: k_stark_verify behind
zkp_hip_verify_improvement_batch, and the mixed verifier.  Every verdict is compared with the oracle's (tests/test_stark_forge.py shows,
without a GPU, what each forgery proves about a verifier that accepts it)."""
import numpy as np
import pytest

import stark_forge as F
from util import P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from libzkp_amd import _native
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    return L


@pytest.fixture(scope="module")
def cases():
    return F.corpus()


def verdicts(L, cases, stride=None, beyond=64):
    """one call; rows padded with 0xFF up to a stride that is longer than every envelope, so that a read past an envelope's length shows;
    returns the verdicts and what lies behind them in the verdict array"""
    n = len(cases)
    stride = stride or max(len(c.env) for c in cases) + 37
    buf = np.full((n, stride), 0xFF, dtype=np.uint8)
    for i, c in enumerate(cases):
        assert len(c.env) < stride
        buf[i, :len(c.env)] = np.frombuffer(c.env, dtype=np.uint8)
    lens = np.array([len(c.env) for c in cases], dtype=np.uint32)
    olds = np.array([c.old for c in cases], dtype=np.uint64)
    ok = np.full(n + beyond, 7, dtype=np.uint8)
    assert L.zkp_hip_verify_improvement_batch(n, P(buf), stride, P(lens), P(olds), P(ok)) == 0
    return ok[:n].tolist(), ok[n:].tolist()


def test_whole_list_in_one_call(hip, cases):
    got, rest = verdicts(hip, cases)
    assert set(got) <= {0, 1} and rest == [7] * 64
    differ = [(c.name, g, c.want) for c, g in zip(cases, got) if bool(g) != c.want]
    print("%d envelopes, %d accepted, %d verdicts differ from the oracle's" % (len(cases), sum(got), len(differ)))
    assert not differ, differ
    assert not [c.name for c, g in zip(cases, got) if c.kind == "forgery" and g]
    assert all(g for c, g in zip(cases, got) if c.kind in ("honest", "vint_form"))
    assert sum(c.kind == "honest" for c in cases) > 100 and sum(c.kind == "forgery" for c in cases) == 14 * len(F.PAIRS)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_lane_and_block_edges(hip, cases, n):
    """the last envelope of the call (the last lane that works, in a workgroup that is full, one short of full, or holds one lane) is a
    forgery that only the DEEP identity at the last opened position refuses; the one before it is honest"""
    forged = next(c for c in cases if c.name.startswith("t_leaf_last"))
    honest = next(c for c in cases if c.kind == "honest")
    lst = ([c for c in cases if c is not forged][:n - 2] + [honest, forged])[-n:]
    assert len(lst) == n and lst[-1] is forged and (n == 1 or lst[-2] is honest)
    got, rest = verdicts(hip, lst)
    assert [bool(g) for g in got] == [c.want for c in lst] and set(got) <= {0, 1}
    assert got[-1] == 0 and (n == 1 or got[-2] == 1)
    assert rest == [7] * 64                                          # nothing written behind the n-th verdict


def test_mixed_verifier_gives_the_same_verdicts(hip, cases):
    import libzkp_amd as z
    assert all(c.old == int.from_bytes(c.env[10:18], "little") for c in cases)         # the mixed call takes `old` from the envelope
    got = z.verify_envelopes([c.env for c in cases], [5] * len(cases))
    differ = [(c.name, g, c.want) for c, g in zip(cases, got) if g != c.want]
    assert not differ, differ
