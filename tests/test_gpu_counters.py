"""The library's host-side counters, all nine families side by side (libzkp_amd/csrc/shard_counters.h; every reader of libzkp_amd.api): four
small calls in one process, every family read after each -- only the families a call feeds move -- then one family read with reset, and in a
process of its own the same calls, a shutdown and a fresh initialisation, after which every family reads zero.  The literal counts are what
the library gave for these calls before the counters shared one table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVELOPE_BYTES = 1094                                                     # an 8-bit range envelope
CONTAINER_BYTES = 12 + 2 * (4 + ENVELOPE_BYTES) + 32                      # "COMP", two counts, two prefixed envelopes, no metadata, the digest


def readers():
    import libzkp_amd as z
    from libzkp_amd import api
    return {"g16_verify": api.groth16_verify_counters, "batch_self_check": api.batch_self_check_counters, "verify_fanout": api.verify_fanout_counters,
            "verify_mixed": api.verify_mixed_counters, "bp_localise": api.bp_verify_counters, "composites": z.verify_composites_counters, "seal": api.seal_counters,
            "statements": api.verify_statements_counters, "key_check": api.key_check_counters}


def read_all(reset=False):
    return {name: fn(reset=reset) for name, fn in readers().items()}


def zeros():
    return {name: {k: (0.0 if k == "ms" else 0) for k in c} for name, c in read_all().items()}


def counts(snapshot):
    return {name: {k: v for k, v in c.items() if k != "ms"} for name, c in snapshot.items()}


def run_calls():
    """verify_envelopes, verify_ops, create_composite_proofs, verify_composite_proofs on two 8-bit range envelopes; every family read after
    each call, without reset: [("name of the call", snapshot), ...], the first one taken right after resetting every family"""
    import libzkp_amd as z
    rng = np.random.default_rng(2201)
    envs = z.prove_range_batch([5, 200], [0, 100], [255, 250], seeds=rng.bytes(64), n_bits=8)
    assert [len(e) for e in envs] == [ENVELOPE_BYTES] * 2
    read_all(reset=True)
    steps = [("reset", read_all())]
    assert z.verify_envelopes(envs + [b"\x02\x07"]) == [True, True, False]
    steps.append(("verify_envelopes", read_all()))
    assert z.verify_ops([("range", 5, 0, 255), ("range", 200, 100, 250)], envs) == [True, True]
    steps.append(("verify_ops", read_all()))
    containers = z.create_composite_proofs([envs])
    assert [len(c) for c in containers] == [CONTAINER_BYTES]
    steps.append(("create_composite_proofs", read_all()))
    assert z.verify_composite_proofs(containers) == [True]
    steps.append(("verify_composite_proofs", read_all()))
    return steps


# what each call adds, family by family (a family that is not named stays where it was, its milliseconds included)
FEEDS = {
    "verify_envelopes": {"verify_mixed": {"launches": 1, "point_adds": 2}},                              # one scheme pass, two envelopes with a row; the garbage gets none
    "verify_ops": {"statements": {"envelopes": 2, "refused_envelope": 0, "refused_statement": 0, "refused_proof": 0}},
    "create_composite_proofs": {"seal": {"containers": 1, "sealed": 1, "envelopes": 2, "bytes": CONTAINER_BYTES}},
    "verify_composite_proofs": {"composites": {"composites": 1, "malformed": 0, "envelopes": 2},
                                "verify_mixed": {"launches": 1, "point_adds": 2}},                       # the inner envelopes go through the mixed verifier's core
}
assert CONTAINER_BYTES == 2240


def check_steps(steps):
    assert [name for name, _ in steps] == ["reset"] + list(FEEDS)
    assert steps[0][1] == zeros()
    for (_, before), (name, after) in zip(steps, steps[1:]):
        print(name, json.dumps(after))
        for family, c in after.items():
            add = FEEDS[name].get(family)
            if add is None:
                assert c == before[family], (name, family)                                               # untouched, to the last bit of its milliseconds
            else:
                assert {k: c[k] - before[family][k] for k in add} == add, (name, family)
                assert c["ms"] > before[family]["ms"], (name, family)
    assert counts(steps[-1][1]) == {
        "g16_verify": {"launches": 0, "point_adds": 0}, "batch_self_check": {"launches": 0, "point_adds": 0}, "verify_fanout": {"launches": 0, "point_adds": 0},
        "verify_mixed": {"launches": 2, "point_adds": 4}, "bp_localise": {"failed_checks": 0, "segment_checks": 0, "jobs_again": 0},
        "composites": {"composites": 1, "malformed": 0, "envelopes": 2}, "seal": {"containers": 1, "sealed": 1, "envelopes": 2, "bytes": 2240},
        "statements": {"envelopes": 2, "refused_envelope": 0, "refused_statement": 0, "refused_proof": 0},
        "key_check": {"loads_checked": 0, "entries_checked": 0, "refused": 0}}


@pytest.fixture(scope="module")
def hip():
    from libzkp_amd import _native
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    return L


def test_each_call_moves_only_the_families_it_feeds_and_a_reset_zeroes_only_the_one_read(hip):
    steps = run_calls()
    check_steps(steps)
    last = steps[-1][1]
    assert readers()["verify_mixed"](reset=True) == last["verify_mixed"]                                 # the read that resets still returns the sums
    after = read_all()
    assert after["verify_mixed"] == {"launches": 0, "point_adds": 0, "ms": 0.0}
    assert {k: v for k, v in after.items() if k != "verify_mixed"} == {k: v for k, v in last.items() if k != "verify_mixed"}
    assert readers()["seal"](reset=True) == last["seal"] and read_all()["seal"] == zeros()["seal"]


_LIFECYCLE_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_counters as T
from libzkp_amd import _native, api
L = _native.lib()
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
steps = T.run_calls()
T.check_steps(steps)
api.shutdown()
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
print(json.dumps({"after_shutdown_and_init": T.read_all(), "zeros": T.zeros()}))
"""


def test_a_shutdown_carries_no_count_into_the_next_life():
    out = subprocess.run([sys.executable, "-c", _LIFECYCLE_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["after_shutdown_and_init"] == r["zeros"] and len(r["zeros"]) == 9
    assert all(v == 0 for c in r["after_shutdown_and_init"].values() for v in c.values())
