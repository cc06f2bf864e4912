"""One verify call for a list of composite proofs (include/libzkp_hip_composites.h; libzkp_amd/csrc/composite_steps.h, composite_impl.inc) on
the MI355X.

Reference verdicts never come from the call under test: per container they come from composite.parse_composite (malformed or not) and
z.verify_composite_proof (the per-container call that existed before).  Envelopes come from process_ops / prove_range_batch under fixed
seeds; the digest-only scenarios use format-valid fake envelopes of scheme 9.  Every scenario runs in a child process (its own shard
registration, keys and switches); the children run once per module and the tests read their results."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ZKP_HIP_VERIFY_SHARDS", "ZKP_HIP_VERIFY_SHARD_MIN", "ZKP_HIP_BATCH_VERIFY_MIN", "ZKP_HIP_G16_BATCH_VERIFY_MIN", "ZKP_HIP_NO_BATCH_VERIFY",
            "ZKP_HIP_BP_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_BATCH_VERIFY_ONLY", "ZKP_HIP_BP_LOCALISE", "ZKP_HIP_BP_LOCALISE_SEGMENT", "ZKP_HIP_COMPOSITES_DIGEST_LOG")

_COMMON = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native, composite
from comp_build import comp, digest_of, four_mib, proof, residue_family, straddle_family, u32
L = _native.lib()
GOLD = os.path.join(sys.argv[1], "tests", "golden")
VP = ctypes.c_void_p

def P(a):
    return a.ctypes.data_as(VP)

def seeds_for(n, salt):
    return bytes(np.random.default_rng(1000 + salt).integers(0, 256, 32 * n, dtype=np.uint8))

def raw_call(containers, flags=0):
    # zkp_hip_verify_composites itself: (rc, statuses, message)
    data = b"".join(containers)
    blob = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(c) for c in containers]))).astype(np.uint64)
    status = np.full(len(containers), 9, dtype=np.uint8)
    rc = L.zkp_hip_verify_composites(len(containers), P(blob), P(off), flags, P(status))
    return rc, status.tolist(), _native.last_error() if rc else ""

def reference_format(c):
    try:
        composite.parse_composite(c)
        return 1
    except composite.ProofFormatError:
        return 2

def reference_status(c):
    # the per-container path that existed before: parse_composite, then one verify_envelopes call
    try:
        return 1 if z.verify_composite_proof(c) else 0
    except composite.ProofFormatError:
        return 2

def flip(b, off, bit=0):
    b = bytearray(b); b[off] ^= 1 << bit
    return bytes(b)

out = {}
"""

_DIGEST = _COMMON + r"""
# no key is loaded in this process, and none is needed
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
rng = np.random.default_rng(5)
wave = []                                                        # one full wave plus six lanes, 0..5 proofs each
for i in range(70):
    proofs = [proof(10 + int(rng.integers(0, 300)), salt=i + k) for k in range(i % 6)]
    meta = [(b"key%d" % k, bytes(int(rng.integers(0, 40)))) for k in range(i % 3)]
    wave.append(comp(proofs, meta))
wave[13] = flip(wave[13], len(wave[13]) - 1); wave[64] = flip(wave[64], 30); wave[69] = wave[69][:-1]
z.verify_composites_counters(reset=True)
rc, st, msg = raw_call(wave, 1)
out["wave"] = {"rc": rc, "status": st, "ref": [reference_format(c) for c in wave], "counters": z.verify_composites_counters(reset=True)}

families = [c for c, _, _ in residue_family()] + [c for c, _, _ in straddle_family()]
families.append(comp([proof(10, salt=k) for k in range(1000)]))
families.append(comp([proof(10, salt=k) for k in range(1001)]))
families.append(comp([proof(77)], [(b"big", bytes(range(256)) * 256), (b"a", b"1")]))
families.append(comp([proof(77)], [(b"big", bytes(65537))]))
families.append(comp([proof(40)], [(b"k", b"first"), (b"\xc3\xa9", b"x"), (b"k", b"last"), (b"a", b"")]))
families.append(comp([proof(40)], [(b"\xed\xa0\x80", b"surrogate")]))
(at, _, _), (over, _, _) = four_mib()
families += [at, over, flip(at, 3000000)]
rc, st, msg = raw_call(families, 1)
out["families"] = {"rc": rc, "n": len(families), "status": st, "ref": [reference_format(c) for c in families], "lengths": [len(at), len(over)]}
# without the flag the fake envelopes (scheme 9) are rejected by the mixed verifier: 0 where there is one, 1 for a container without proofs
rc, st, msg = raw_call(wave, 0)
out["wave_full"] = {"rc": rc, "status": st, "want": [2 if reference_format(c) == 2 else 1 if i % 6 == 0 else 0 for i, c in enumerate(wave)]}
out["n0"] = [L.zkp_hip_verify_composites(0, None, None, 0, None), L.zkp_hip_verify_composites(0, None, None, 1, None)]

# the Python front end
out["py_false"] = z.verify_composite_proofs(wave, integrity_only=True)
out["py_empty"] = z.verify_composite_proofs([], integrity_only=True)
out["py_raise_clean"] = z.verify_composite_proofs([w for i, w in enumerate(wave) if i not in (13, 64, 69)], integrity_only=True, errors="raise")
msgs = {}
for name, lst, bad in (("digest", wave[:20], 13), ("truncated", wave[65:], 4), ("key", [wave[0], families[-4], wave[1]], 1)):
    try:
        z.verify_composite_proofs(lst, integrity_only=True, errors="raise")
        got = None
    except composite.ProofFormatError as e:
        got = str(e)
    try:
        composite.parse_composite(lst[bad]); want = None
    except composite.ProofFormatError as e:
        want = str(e)
    msgs[name] = [got, want]
out["py_raise"] = msgs
print(json.dumps(out))
"""

_FULL = _COMMON + r"""
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
    api.install_proving_key(kind, open(os.path.join(GOLD, name), "rb").read())
rng = np.random.default_rng(11)
ops = []
for i in range(6):
    v = int(rng.integers(1000, 1000 + 2**20)); vals = [int(x) for x in rng.integers(0, 2**30, 1 + i % 4)]
    s = [int(x) for x in rng.choice(2**32, (1, 5, 64)[i % 3], replace=False)]; o = int(rng.integers(0, 2**62))
    ops += [("range", v, 1000, 1000 + 2**20), ("threshold", vals, max(sum(vals) - i, 0)), ("equality", v, v), ("membership", s[i % len(s)], s),
            ("improvement", o, o + 1 + i), ("consistency", sorted(int(x) for x in rng.integers(0, 2**50, (2, 5)[i % 2])))]
envs = api.process_ops(ops, seeds_for(len(ops), 1))
assert len(envs) == 36 and sorted(set(e[1] for e in envs)) == [1, 2, 3, 4, 5, 6]
sizes = [0, 1, 2, 3] * 6                                        # 24 containers, 36 envelopes: empty and single-proof ones among them
inner, at = [], 0
for k in sizes:
    inner.append(envs[at:at + k]); at += k
meta = lambda i: [(b"issuer", b"acme"), (b"n", u32(i)), (b"issuer", b"late")][:i % 4]
base = [comp(p, meta(i)) for i, p in enumerate(inner)]
out["schemes"] = [[e[1] for e in p] for p in inner]
z.verify_mixed_counters(reset=True); z.verify_composites_counters(reset=True)
rc, st, msg = raw_call(base)
out["base"] = {"rc": rc, "status": st, "mixed": z.verify_mixed_counters(reset=True), "counters": z.verify_composites_counters(reset=True)}
out["base_ref"] = [reference_status(c) for c in base]

damaged = list(base)
i_flip, i_ver, i_dig = 7, 10, 15                                # containers of 3, 2 and 3 envelopes
p = list(inner[i_flip]); p[1] = flip(p[1], 150 if p[1][1] == 6 else 100); damaged[i_flip] = comp(p, meta(i_flip))
p = list(inner[i_ver]); p[0] = bytes([3]) + p[0][1:]; damaged[i_ver] = comp(p, meta(i_ver))
damaged[i_dig] = flip(base[i_dig], len(base[i_dig]) - 7)
out["damaged_at"] = [i_flip, i_ver, i_dig]
out["damaged_ref"] = [reference_status(c) for c in damaged]
z.verify_mixed_counters(reset=True); z.verify_composites_counters(reset=True)
rc, st, msg = raw_call(damaged)
out["damaged"] = {"rc": rc, "status": st, "mixed": z.verify_mixed_counters(reset=True), "counters": z.verify_composites_counters(reset=True)}
out["py"] = z.verify_composite_proofs(damaged)
try:
    z.verify_composite_proofs(damaged, errors="raise"); got = None
except composite.ProofFormatError as e:
    got = str(e)
try:
    composite.parse_composite(damaged[i_dig]); want = None
except composite.ProofFormatError as e:
    want = str(e)
out["py_raise"] = [got, want]
out["py_integrity"] = z.verify_composite_proofs(damaged, integrity_only=True)
print(json.dumps(out))
"""

_NO_KEY = _COMMON + r"""
# no Groth16 key exists in this process
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
eq_like = bytes([2, 2]) + u32(256) + u32(32) + bytes(288)
good, holder = comp([proof(20)]), comp([eq_like], [(b"k", b"v")])
rc, st, msg = raw_call([good, flip(holder, len(holder) - 1), good])
out["malformed_holder"] = [rc, st, msg]
rc, st, msg = raw_call([good, holder, good])
out["well_formed_holder"] = [rc, msg]
rc, st, msg = raw_call([good, holder, good], 1)
out["well_formed_holder_integrity_only"] = [rc, st]
blob = np.frombuffer(eq_like, dtype=np.uint8); off = np.array([0, 298], dtype=np.uint64); ok1 = np.zeros(1, dtype=np.uint8)
out["envelopes_call"] = [L.zkp_hip_verify_envelopes(1, P(blob), P(off), None, P(ok1)), _native.last_error()]
print(json.dumps(out))
"""

_RANGE = _COMMON + r"""
# started with ZKP_HIP_BATCH_VERIFY_MIN=64; two shards of the library on one GPU
_native.init_devices([0, 0])
n = 160
rng = np.random.default_rng(3)
v = [int(x) for x in rng.integers(0, 2**32, n)]
envs = z.prove_range_batch(v, [0] * n, [2**32] * n, seeds=seeds_for(n, 9))
groups = [envs[4 * i:4 * i + 4] for i in range(40)]
bad_at = 23
groups[bad_at][2] = flip(groups[bad_at][2], 700, 2)                           # a scalar of the first inner proof: reaches the equations
lst = [comp(g, [(b"i", u32(i))]) for i, g in enumerate(groups)]
out["bad_at"] = bad_at
os.environ["ZKP_HIP_VERIFY_SHARDS"] = "0"
out["ref"] = [reference_status(c) for c in lst]                               # 8 jobs per call: below the threshold, job by job
z.bp_verify_counters(reset=True); z.verify_fanout_counters(reset=True)
rc, st, msg = raw_call(lst)
out["one_shard"] = {"rc": rc, "status": st, "bp": z.bp_verify_counters(reset=True), "fanout": z.verify_fanout_counters(reset=True)}
del os.environ["ZKP_HIP_VERIFY_SHARDS"]
os.environ["ZKP_HIP_VERIFY_SHARD_MIN"] = "32"
z.verify_composites_counters(reset=True)
rc, st, msg = raw_call(lst)
out["two_shards"] = {"rc": rc, "status": st, "fanout": z.verify_fanout_counters(reset=True), "counters": z.verify_composites_counters(reset=True)}
print(json.dumps(out))
"""


def _child(script, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra_env)
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def digest():
    return _child(_DIGEST)


@pytest.fixture(scope="module")
def full():
    return _child(_FULL)


def test_a_wave_and_six_lanes_of_containers_get_the_reference_statuses(digest):
    w = digest["wave"]
    assert w["rc"] == 0 and w["status"] == w["ref"] and len(w["ref"]) == 70
    assert [i for i, s in enumerate(w["ref"]) if s == 2] == [13, 64, 69]
    c = w["counters"]
    assert (c["composites"], c["malformed"], c["envelopes"]) == (70, 3, 0) and c["ms"] > 0
    assert digest["n0"] == [0, 0]


def test_residues_straddles_and_the_limits_get_the_reference_statuses(digest):
    f = digest["families"]
    assert f["rc"] == 0 and f["status"] == f["ref"] and f["n"] == 131 + 8 * 64 + 7 + 9
    assert f["lengths"] == [4 << 20, (4 << 20) + 1]
    # 1000 proofs | 1001 | a 65536-byte value | 65537 | a repeated key | a surrogate in a key | exactly 4 MiB | one byte more | 4 MiB with a flipped byte
    assert f["status"][-9:] == [1, 2, 1, 2, 1, 2, 1, 2, 2]
    assert f["status"][:131] == [1] * 131 and sum(s == 2 for s in f["status"][131:-9]) == 7          # the stray bytes between the alignments


def test_without_the_flag_the_fake_envelopes_are_rejected(digest):
    w = digest["wave_full"]
    assert w["rc"] == 0 and w["status"] == w["want"] and set(w["status"]) == {0, 1, 2}


def test_python_front_end_on_digests(digest):
    assert digest["py_false"] == [s == 1 for s in digest["wave"]["ref"]] and digest["py_empty"] == []
    assert digest["py_raise_clean"] == [True] * 67
    for name, (got, want) in digest["py_raise"].items():
        assert got is not None and got == want, name
    assert "composition hash mismatch" in digest["py_raise"]["digest"][0] and "non-utf8" in digest["py_raise"]["key"][0]


def test_containers_of_all_six_schemes(full):
    b = full["base"]
    assert len(full["schemes"]) == 24 and sorted({s for p in full["schemes"] for s in p}) == [1, 2, 3, 4, 5, 6]
    assert full["base_ref"] == [1] * 24 and b["rc"] == 0 and b["status"] == [1] * 24
    assert b["mixed"]["launches"] == 6 and b["mixed"]["point_adds"] == 36                           # ONE pass of the mixed verifier over all 36
    c = b["counters"]
    assert (c["composites"], c["malformed"], c["envelopes"]) == (24, 0, 36)


def test_damage_is_confined_to_its_container(full):
    d, (i_flip, i_ver, i_dig) = full["damaged"], full["damaged_at"]
    want = [0 if i in (i_flip, i_ver) else 2 if i == i_dig else 1 for i in range(24)]
    assert full["damaged_ref"] == want and d["rc"] == 0 and d["status"] == want
    # the container with the wrong digest contributed no envelope: 36 less its 3, and the version-3 envelope is refused by the classification
    assert d["counters"]["envelopes"] == 33 and d["counters"]["malformed"] == 1 and d["mixed"]["point_adds"] == 32
    assert full["py"] == [s == 1 for s in want]
    assert full["py_raise"][0] is not None and full["py_raise"][0] == full["py_raise"][1]
    assert full["py_integrity"] == [i != i_dig for i in range(24)]


def test_a_process_without_keys():
    r = _child(_NO_KEY)
    assert r["malformed_holder"] == [0, [0, 2, 0], ""]                                              # (the fake scheme-9 envelopes of its neighbours are rejected)
    rc, msg = r["well_formed_holder"]
    assert rc == -3 and "no (usable) key loaded" in msg and [rc, msg] == r["envelopes_call"]
    assert r["well_formed_holder_integrity_only"] == [0, [1, 1, 1]]


@pytest.fixture(scope="module")
def ranges():
    return _child(_RANGE, ZKP_HIP_BATCH_VERIFY_MIN="64")


def test_batch_check_across_containers(ranges):
    want = [0 if i == ranges["bad_at"] else 1 for i in range(40)]
    o = ranges["one_shard"]
    assert ranges["ref"] == want and o["rc"] == 0 and o["status"] == want
    # 40 containers x 4 envelopes = 320 jobs in ONE batch check, which does not stand; then the localisation pass
    assert o["bp"]["failed_checks"] == 1 and o["bp"]["segment_checks"] >= 2 and 0 < o["bp"]["jobs_again"] < 320
    assert o["fanout"] == {"launches": 0, "point_adds": 0, "ms": 0.0}


def test_two_shards_on_one_gpu(ranges):
    want = [0 if i == ranges["bad_at"] else 1 for i in range(40)]
    t = ranges["two_shards"]
    assert t["rc"] == 0 and t["status"] == want == ranges["one_shard"]["status"]
    assert (t["fanout"]["launches"], t["fanout"]["point_adds"]) == (2, 40)
    assert (t["counters"]["composites"], t["counters"]["malformed"], t["counters"]["envelopes"]) == (40, 0, 160)


def test_the_python_names_are_exported():
    import libzkp_amd as z
    from libzkp_amd import _native, composite
    assert z.verify_composite_proofs is composite.verify_composite_proofs and z.verify_composites_counters is composite.verify_composites_counters
    assert "verify_composite_proofs" in z.__all__ and "verify_composites_counters" in z.__all__
    assert _native.EXPORTS_COMPOSITES == ("zkp_hip_verify_composites", "zkp_hip_composites_counters")
