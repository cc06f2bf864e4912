"""The Groth16 batch verifier's localisation pass on the MI355X (g16_localise.h, kernels k_g16_seg_* of fq2vm_kernels.hip): when the batch
check of a call does not stand, one check per segment says where the bad envelopes can be and only those segments' envelopes get the
per-envelope check.  Every case compares the verdicts with the same call under ZKP_HIP_NO_BATCH_VERIFY=1 (per-envelope check only) and reads
what the call did from the counters (api.groth16_verify_counters: segment checks run, envelopes verified again)."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SWITCHES = ("ZKP_HIP_NO_BATCH_VERIFY", "ZKP_HIP_G16_LOCALISE", "ZKP_HIP_G16_LOCALISE_SEGMENT", "ZKP_HIP_G16_BATCH_VERIFY_ONLY")
INFINITY_G1 = bytes(63) + b"\x40"


@pytest.fixture(scope="module")
def proofs():
    """150 distinct equality proofs and 12 membership proofs (sets of 1 .. 64 elements: envelopes of different lengths) under the golden keys"""
    import libzkp_amd as z
    import libzkp_amd.api as api
    from libzkp_amd import _native
    _native.check(_native.lib().zkp_hip_init(0), "zkp_hip_init")
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        api.install_proving_key(kind, open(os.path.join(GOLD, name), "rb").read())
    rng = np.random.default_rng(2718)
    vals = [int(x) for x in rng.integers(0, 2**63, 150, dtype=np.uint64)]
    eq = z.prove_equality_batch(vals, vals)
    sets = [[int(x) for x in rng.integers(1, 2**64, int(rng.integers(1, 65)), dtype=np.uint64)] for _ in range(12)]
    mem = z.prove_membership_batch([s[i % len(s)] for i, s in enumerate(sets)], sets)
    assert len({p[266:] for p in eq}) == 150
    return eq, mem


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def cycled(src, n):
    return [src[i % len(src)] for i in range(n)]


def swap_commitment(blobs, i):
    """envelope i: a valid proof under its neighbour's commitment"""
    other = blobs[i + 1] if i + 1 < len(blobs) else blobs[i - 1]
    assert blobs[i][-32:] != other[-32:]
    blobs[i] = blobs[i][:-32] + other[-32:]


def verify(kind, blobs, monkeypatch, **env):
    """(verdicts, counters) of one call under the given switches; the counters are reset before it"""
    import libzkp_amd.api as api
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    api.groth16_verify_counters(reset=True)
    got = api._verify_snark_envelopes(kind, blobs)
    c = api.groth16_verify_counters(reset=True)
    for k in env:
        monkeypatch.delenv(k)
    assert api.groth16_verify_counters(reset=False) == {"launches": 0, "point_adds": 0, "ms": 0.0}          # reset means reset
    return got, c


def per_envelope(kind, blobs, monkeypatch):
    got, c = verify(kind, blobs, monkeypatch, ZKP_HIP_NO_BATCH_VERIFY="1")
    assert c["launches"] == 0 and c["point_adds"] == 0                                                       # no batch check, so none that failed
    return got


def suspects(n, size, bad):
    """(segments of n envelopes, summed sizes of the distinct segments that hold a bad envelope)"""
    nseg = -(-n // size)
    return nseg, sum(min(size, n - s * size) for s in {i // size for i in bad})


def test_one_bad_envelope_costs_its_segment(proofs, monkeypatch):
    n = 16384
    blobs = cycled(proofs[0], n)
    swap_commitment(blobs, 5000)
    want = [i != 5000 for i in range(n)]
    assert per_envelope(0, blobs, monkeypatch) == want
    got, c = verify(0, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE_SEGMENT="64")
    print("segment 64:", c)
    assert got == want and c["launches"] == 256 and c["point_adds"] == 64 and c["ms"] > 0
    got, c = verify(0, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE_SEGMENT="1024")
    print("segment 1024:", c)
    assert got == want and c["launches"] == 16 and c["point_adds"] == 1024
    got, c = verify(0, blobs, monkeypatch)
    print("default segment:", c)
    assert got == want and c["launches"] >= 2 and 0 < c["point_adds"] < n


def test_partial_last_segment_first_and_last_envelope_and_two_in_one_segment(proofs, monkeypatch):
    n, size = 8237, 64
    blobs = cycled(proofs[0], n)
    bad = (0, 4000, 4010, 8236)
    for i in bad:
        swap_commitment(blobs, i)
    want = [i not in bad for i in range(n)]
    assert per_envelope(0, blobs, monkeypatch) == want
    got, c = verify(0, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE_SEGMENT=str(size))
    nseg, m = suspects(n, size, bad)
    assert (nseg, m) == (129, 64 + 64 + 45)
    print(c)
    assert got == want and c["launches"] == nseg and c["point_adds"] == m


@pytest.mark.parametrize("k", (1, 200))
def test_several_rounds_of_chain_a(proofs, monkeypatch, k):
    """65 536 envelopes: the batch's chain A runs in several rounds of workgroups; one bad envelope, and 200 spread over the batch"""
    n = 65536
    blobs = cycled(proofs[0], n)
    bad = [31337] if k == 1 else [5 + 327 * i for i in range(200)]
    for i in bad:
        swap_commitment(blobs, i)
    want = np.ones(n, dtype=bool); want[bad] = False
    assert per_envelope(0, blobs, monkeypatch) == want.tolist()
    got, c = verify(0, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE_SEGMENT="128")
    nseg, m = suspects(n, 128, bad)
    print(c)
    assert got == want.tolist() and c["launches"] == nseg == 512 and c["point_adds"] == (n if 2 * m >= n else m)
    got, c = verify(0, blobs, monkeypatch)
    print("default segment:", c)
    assert got == want.tolist() and c["launches"] >= 2 and 0 < c["point_adds"] <= n and (k > 1 or c["point_adds"] < n)


def _f2_sqrt(bn, a):
    """square root in Fq2 (p = 3 mod 4), None for a non-residue"""
    def f2pow(b, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = bn.f2_mul(r, b)
            b = bn.f2_mul(b, b); e >>= 1
        return r
    if a == (0, 0):
        return (0, 0)
    a1 = f2pow(a, (bn.P - 3) // 4)
    alpha = bn.f2_mul(bn.f2_mul(a1, a1), a)
    a0 = bn.f2_mul(f2pow(alpha, bn.P), alpha)
    if a0 == (bn.P - 1, 0):
        return None
    x0 = bn.f2_mul(a1, a)
    if alpha == (bn.P - 1, 0):
        return bn.f2_mul((0, 1), x0)
    return bn.f2_mul(f2pow(bn.f2_add((1, 0), alpha), (bn.P - 1) // 2), x0)


def test_point_at_infinity_b_outside_g2_and_a_refused_encoding(proofs, monkeypatch):
    """Three envelopes in different segments: A at infinity (a valid encoding the batch check does not take), B moved out of G2 by a point of the
    twist's cofactor part (only the subgroup check refuses it; its segment is never cleared by a product), and both flag bits set in A's last
    byte (refused at the parse: it takes no part in any product).  Only the segments of the first two are verified again."""
    from oracle.py import bn254 as bn
    n = 16384
    blobs = cycled(proofs[0], n)
    b = bytearray(blobs[1000]); b[10:74] = INFINITY_G1; blobs[1000] = bytes(b)
    rr = random.Random(9)
    while True:
        x = (rr.randrange(bn.P), rr.randrange(bn.P))
        y = _f2_sqrt(bn, bn.f2_add(bn.f2_mul(bn.f2_sq(x), x), bn.B2))
        if y is not None:
            break
    cof = bn.G2C.mul_pt((x, y), bn.R, reduce=False)
    okb, bpt = bn.de_g2(blobs[7000][74:202])
    assert okb and cof is not None and bn.G2C.is_on_curve(cof)
    b = bytearray(blobs[7000]); b[74:202] = bn.ser_g2(bn.G2C.add_pts(bpt, cof)); blobs[7000] = bytes(b)
    b = bytearray(blobs[12000]); b[73] |= 0xC0; blobs[12000] = bytes(b)
    want = [i not in (1000, 7000, 12000) for i in range(n)]
    assert per_envelope(0, blobs, monkeypatch) == want
    got, c = verify(0, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE_SEGMENT="64")
    print(c)
    assert got == want and c["launches"] == 256 and c["point_adds"] == 128
    only_refused = cycled(proofs[0], n); only_refused[12000] = blobs[12000]          # a refused envelope alone leaves the batch check standing
    got, c = verify(0, only_refused, monkeypatch)
    assert got == [i != 12000 for i in range(n)] and c["launches"] == 0 and c["point_adds"] == 0


def test_every_third_envelope_bad_takes_the_whole_batch_pass(proofs, monkeypatch):
    n = 16384
    blobs = cycled(proofs[0], n)
    for i in range(0, n, 3):
        swap_commitment(blobs, i)
    want = [i % 3 != 0 for i in range(n)]
    assert per_envelope(0, blobs, monkeypatch) == want
    got, c = verify(0, blobs, monkeypatch)
    print(c)
    assert got == want and c["point_adds"] == n and c["launches"] >= 2


def test_all_valid_and_all_refused_run_no_second_pass(proofs, monkeypatch):
    n = 16384
    got, c = verify(0, cycled(proofs[0], n), monkeypatch)
    assert got == [True] * n and c["launches"] == 0 and c["point_adds"] == 0 and c["ms"] == 0
    refused = [bytes(298)] * n
    assert per_envelope(0, refused, monkeypatch) == [False] * n
    got, c = verify(0, refused, monkeypatch)
    assert got == [False] * n and c["launches"] == 0 and c["point_adds"] == 0


def test_localisation_switched_off_verifies_the_whole_batch_again(proofs, monkeypatch):
    n = 16384
    blobs = cycled(proofs[0], n)
    swap_commitment(blobs, 5000)
    got, c = verify(0, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE="0")
    assert got == [i != 5000 for i in range(n)] and c["launches"] == 0 and c["point_adds"] == n and c["ms"] > 0
    with pytest.raises(Exception, match="batch check did not stand"):                 # the diagnostic switch keeps its meaning: no localisation, the call fails
        verify(0, blobs, monkeypatch, ZKP_HIP_G16_BATCH_VERIFY_ONLY="1")


def test_membership_one_set_element_flipped(proofs, monkeypatch):
    n, size = 8237, 64
    blobs = cycled(proofs[1], n)
    assert len({len(e) for e in blobs}) > 1                                            # rows shorter than the stride
    b = bytearray(blobs[4000]); b[14] ^= 1; blobs[4000] = bytes(b)
    want = [i != 4000 for i in range(n)]
    assert per_envelope(1, blobs, monkeypatch) == want
    got, c = verify(1, blobs, monkeypatch, ZKP_HIP_G16_LOCALISE_SEGMENT=str(size))
    print(c)
    assert got == want and c["launches"] == 129 and c["point_adds"] == 64
    got, c = verify(1, blobs, monkeypatch)
    assert got == want and c["launches"] >= 2 and 0 < c["point_adds"] < n


_TWO_SHARDS_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native
L = _native.lib()
_native.init_devices([0, 0])                                  # two shards of the library on one GPU
gold = os.path.join(sys.argv[1], "tests", "golden")
api.install_proving_key(0, open(os.path.join(gold, "equality_mimc_pk.bin"), "rb").read())
rng = np.random.default_rng(99)
vals = [int(x) for x in rng.integers(0, 2**63, 150, dtype=np.uint64)]
eq = z.prove_equality_batch(vals, vals)
n = 16384
out = {}
api.groth16_verify_counters(reset=True)
for shard, bad in ((0, 5000), (1, 9000)):
    assert L.zkp_hip_use_device(shard) == 0
    blobs = [eq[i % 150] for i in range(n)]
    blobs[bad] = blobs[bad][:266] + blobs[bad + 1][266:]
    os.environ["ZKP_HIP_G16_LOCALISE_SEGMENT"] = "64"
    got = api._verify_snark_envelopes(0, blobs)
    del os.environ["ZKP_HIP_G16_LOCALISE_SEGMENT"]
    out["after_%d" % shard] = api.groth16_verify_counters(reset=False)
    os.environ["ZKP_HIP_NO_BATCH_VERIFY"] = "1"
    ref = api._verify_snark_envelopes(0, blobs)
    del os.environ["ZKP_HIP_NO_BATCH_VERIFY"]
    out["same_%d" % shard] = got == ref
    out["false_%d" % shard] = [i for i, v in enumerate(got) if not v]
out["read_and_reset"] = api.groth16_verify_counters(reset=True)
out["then"] = api.groth16_verify_counters(reset=False)
print(json.dumps(out))
"""


def test_two_shards_on_one_device_sum_their_counters():
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out = subprocess.run([sys.executable, "-c", _TWO_SHARDS_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(r)
    assert r["same_0"] and r["same_1"] and r["false_0"] == [5000] and r["false_1"] == [9000]
    assert (r["after_0"]["launches"], r["after_0"]["point_adds"]) == (256, 64)
    assert (r["after_1"]["launches"], r["after_1"]["point_adds"]) == (512, 128)          # shard 0's and shard 1's, summed
    assert (r["read_and_reset"]["launches"], r["read_and_reset"]["point_adds"]) == (512, 128)
    assert r["then"] == {"launches": 0, "point_adds": 0, "ms": 0.0}
