"""Sealing a list of composite proofs in one call (include/libzkp_hip_seal.h; libzkp_amd/csrc/composite_seal.h, composite_seal_impl.inc) on
the MI355X.

Reference bytes never come from the call under test: per container they come from comp_build.comp (hashlib, keys as raw bytes) and from
composite._serialize_composite / create_composite_proof / create_proof_with_metadata, the Python that existed before.  All comparisons
are byte equality.  The host-buffer scenarios use format-valid fake envelopes of scheme 9 and need no key; the batch scenarios prove one op
of each of the six schemes under fixed seeds and the committed golden keys.  Every scenario runs in a child process (its own shard
registration and keys); the children run once per module and the tests read their results."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = r"""
import ctypes, hashlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native, composite
from comp_build import comp, entry, four_mib, proof, residue_family, straddle_family, u32
L = _native.lib()
GOLD = os.path.join(sys.argv[1], "tests", "golden")
VP = ctypes.c_void_p

def P(a):
    return None if a is None else a.ctypes.data_as(VP)

def offsets(lengths):
    return np.concatenate(([0], np.cumsum(lengths, dtype=np.uint64))).astype(np.uint64)

def wire(meta):
    return b"".join(entry(k, v) for k, v in meta)

def raw_seal(lists, metas=None, lead=0, cap=None, stray=0):
    # libzkp_seal_composites itself: (rc, statuses, out_off, the whole output buffer: lead | cap | 8 guard bytes); `stray` bytes of
    # another envelope lie in front of the first one
    envs = [bytes(stray)] + [p for lst in lists for p in lst]
    env_blob, env_off = np.frombuffer(b"".join(envs) or b"\0", dtype=np.uint8), offsets([len(e) for e in envs])
    first = (offsets([len(lst) for lst in lists]) + np.uint64(1)).astype(np.uint64)
    n = len(lists)
    meta_blob = meta_off = None
    if metas is not None:
        meta_blob, meta_off = np.frombuffer(b"".join(metas) or b"\0", dtype=np.uint8), offsets([len(m) for m in metas])
    status, out_off = np.full(n, 9, dtype=np.uint8), np.full(n + 1, 9, dtype=np.uint64)
    if cap is None:
        rc = L.libzkp_seal_composites(n, P(env_blob), P(env_off), len(envs), P(first), P(meta_blob), P(meta_off), None, 0, P(out_off), P(status))
        cap = int(out_off[n])
        assert rc == (-3 if cap else rc), rc
    out = np.full(lead + cap + 8, 0xA5, dtype=np.uint8)
    rc = L.libzkp_seal_composites(n, P(env_blob), P(env_off), len(envs), P(first), P(meta_blob), P(meta_off), VP(out.ctypes.data + lead), cap, P(out_off), P(status))
    return rc, status.tolist(), [int(x) for x in out_off], out

def pieces(out, off, lead=0):
    return [out[lead + off[i]:lead + off[i + 1]].tobytes() for i in range(len(off) - 1)]

def guards(out, off, lead=0):
    return bool((out[:lead + off[0]] == 0xA5).all() and (out[lead + off[-1]:] == 0xA5).all())

def sha(bs):
    return [hashlib.sha256(b).hexdigest() for b in bs]

def verify_integrity(containers):
    blob = np.frombuffer(b"".join(containers), dtype=np.uint8)
    off = offsets([len(c) for c in containers])
    st = np.full(len(containers), 9, dtype=np.uint8)
    rc = L.zkp_hip_verify_composites(len(containers), P(blob), P(off), _native.COMPOSITES_INTEGRITY_ONLY, P(st))
    return rc, st.tolist()

out = {}
"""

_HOST = _COMMON + r"""
# no key is loaded in this process, and none is needed
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
rng = np.random.default_rng(5)
lists, metas = [], []                                            # one full wave plus six lanes
for i in range(70):
    lists.append([proof(10 + int(rng.integers(0, 300)), salt=i + k) for k in range(1 + i % 6)])
    metas.append([(b"key%d" % k, bytes(int(rng.integers(0, 40)))) for k in range(i % 3)])
lists[13] = []
lists[64] = lists[64][:2] + [bytes(9)] + lists[64][2:]
want = [comp(p, m) if i not in (13, 64) else b"" for i, (p, m) in enumerate(zip(lists, metas))]
z.seal_counters(reset=True)
rc, st, off, buf = raw_seal(lists, [wire(m) for m in metas], lead=3, stray=1)
got = pieces(buf, off, 3)
out["wave"] = {"rc": rc, "status": st, "same": [g == w for g, w in zip(got, want)], "guards": guards(buf, off, 3), "counters": z.seal_counters(reset=True),
               "expect": {"containers": 70, "sealed": 68, "envelopes": sum(len(p) for i, p in enumerate(lists) if i not in (13, 64)), "bytes": sum(len(w) for w in want)}}
sealed = [g for g in got if g]
rc, vst = verify_integrity(sealed)
back = [composite.parse_composite(g) for g in sealed]
keep = [i for i in range(70) if i not in (13, 64)]
out["round_trip"] = {"rc": rc, "status": vst, "parsed": [back[j] == (lists[i], {k.decode(): v for k, v in metas[i]}) for j, i in enumerate(keep)]}

fam = [(c, p, m) for c, p, m in residue_family()] + [(c, p, m) for c, p, m in straddle_family() if p is not None]
rc, st, off, buf = raw_seal([p for _, p, _ in fam], [wire(m) for _, _, m in fam], lead=2, stray=3)
got = pieces(buf, off, 2)
out["families"] = {"rc": rc, "n": len(fam), "status_all_1": st == [1] * len(fam), "same": sum(g == c for g, (c, _, _) in zip(got, fam)), "guards": guards(buf, off, 2)}
rc, vst = verify_integrity(got)
out["families_verify"] = [rc, vst == [1] * len(fam)]

G = proof(47, salt=3)
(at, p4, m_at), (over, _, m_over) = four_mib()
m1000 = [(b"key%04d" % (999 - k), bytes(k % 5)) for k in range(1000)]
limits = [
    ([G], [], 1), ([], [], 2), ([G, bytes(9)], [], 2), ([bytes([2, 9]) + u32(5) + u32(0) + bytes(6)], [], 2),
    ([bytes([2, 9]) + u32(900 * 1024 + 1) + u32(0) + bytes(900 * 1024 + 1)], [], 2), ([bytes([2, 9]) + u32(900 * 1024) + u32(0) + bytes(900 * 1024)], [], 1),
    ([bytes([2, 9]) + u32(5) + u32(257) + bytes(262)], [], 2), ([bytes([2, 9]) + u32(5) + u32(256) + bytes(261)], [], 1),
    ([proof(10 + k % 4, salt=k) for k in range(1000)], [], 1), ([proof(10, salt=k) for k in range(1001)], [], 3),
    ([G], m1000, 1), ([G], m1000 + [(b"one more", b"")], 3),
    ([G], [(b"k" * 1024, b"v")], 1), ([G], [(b"k" * 1025, b"v")], 3),
    ([G], [(b"k", bytes(range(256)) * 256)], 1), ([G], [(b"k", bytes(65537))], 3),
    ([G], [(b"\xed\xa0\x80", b"surrogate")], 3), ([G], [(b"caf\xc3\xa9", b"x"), (b"", b"")], 1),
    ([G], [(b"k", b"first"), (b"j", b"x"), (b"k", b"last")], 3), ([G], wire([(b"kk", bytes(50))])[:-1], 3), ([G], wire([(b"kk", b"v")]) + b"\0", 3),
    (p4, m_at, 1), (p4, m_over, 3),
]
rc, st, off, buf = raw_seal([c[0] for c in limits], [c[1] if isinstance(c[1], bytes) else wire(c[1]) for c in limits], lead=1, stray=2)
got = pieces(buf, off, 1)
out["limits"] = {"rc": rc, "status": st, "want": [c[2] for c in limits], "same": [g == (comp(c[0], c[1]) if c[2] == 1 else b"") for g, c in zip(got, limits)],
                 "guards": guards(buf, off, 1), "four_mib": [len(got[-2]), got[-2] == at]}
rc, vst = verify_integrity([g for g in got if g])
out["limits_verify"] = [rc, vst]

# a buffer one byte too small; n = 0; argument errors
small = [[G], [], [proof(13), proof(10)]]
rc, st, off, buf = raw_seal(small, None, lead=4)
need = off[-1]
rc2, st2, off2, buf2 = raw_seal(small, None, lead=4, cap=need - 1)
out["out_cap"] = {"rc": [rc, rc2], "need": [need, off2[-1], len(comp([G])) + len(comp(small[2]))], "untouched": bool((buf2 == 0xA5).all()), "msg": _native.last_error(), "status": [st, st2]}
out["n0"] = L.libzkp_seal_composites(0, None, None, 0, None, None, None, None, 0, None, None)
one = np.zeros(2, dtype=np.uint64); st1 = np.zeros(2, dtype=np.uint8); blob = np.frombuffer(G + G, dtype=np.uint8); eoff = offsets([47, 47])
args = []
for first in ([0, 2, 1], [1, 0, 2], [0, 1, 3]):
    f = np.array(first, dtype=np.uint64); o3 = np.zeros(3, dtype=np.uint64)
    args.append(L.libzkp_seal_composites(2, P(blob), P(eoff), 2, P(f), None, None, None, 0, P(o3), P(st1)))
f = np.array([0, 1, 2], dtype=np.uint64); o3 = np.zeros(3, dtype=np.uint64)
args.append(L.libzkp_seal_composites(2, P(blob), P(eoff), 2, None, None, None, None, 0, P(o3), P(st1)))           # first
args.append(L.libzkp_seal_composites(2, P(blob), None, 2, P(f), None, None, None, 0, P(o3), P(st1)))            # env_off
args.append(L.libzkp_seal_composites(2, None, P(eoff), 2, P(f), None, None, None, 0, P(o3), P(st1)))            # env_blob
args.append(L.libzkp_seal_composites(2, P(blob), P(eoff), 2, P(f), None, None, None, 0, None, P(st1)))          # out_off
args.append(L.libzkp_seal_composites(2, P(blob), P(eoff), 2, P(f), None, None, None, 0, P(o3), None))           # status
args.append(L.libzkp_seal_composites(2, P(blob), P(eoff), 2, P(f), None, None, None, 7, P(o3), P(st1)))         # out with room claimed
args.append(L.libzkp_seal_composites(2, P(blob), P(eoff), 2, P(f), None, P(np.array([0, 5, 3], dtype=np.uint64)), None, 0, P(o3), P(st1)))      # meta_off runs backwards
out["arguments"] = args

# the Python front end
py_lists = [[G], [proof(20), proof(31)], [proof(12)]]
py_meta = [{"issuer": b"acme", "n": u32(1)}, {}, {"é": b"", "a": b"1"}]
out["py"] = [z.create_composite_proofs(py_lists) == [composite.create_composite_proof(p) for p in py_lists],
             z.create_composite_proofs([p[:1] for p in py_lists], py_meta) == [composite.create_proof_with_metadata(p[0], m) for p, m in zip(py_lists, py_meta)],
             z.create_composite_proofs(py_lists, py_meta) == [composite._serialize_composite(p, m) for p, m in zip(py_lists, py_meta)],
             z.create_composite_proofs([]) == []]
bad = {"empty": [[G], [], [G]], "malformed": [[G], [G, bytes([2, 9]) + u32(5) + u32(0) + bytes(6)]], "short": [[bytes(3)]]}
raised = {}
for name, lst in bad.items():
    i = [k for k, p in enumerate(lst) if not p or any(len(e) != 47 for e in p)][0]
    pair = []
    for fn in (lambda: z.create_composite_proofs(lst), lambda: composite.create_composite_proof(lst[i])):
        try:
            fn(); pair.append(None)
        except Exception as e:
            pair.append([type(e).__name__, str(e)])
    raised[name] = pair
out["py_raise"] = raised
res = z.create_composite_proofs(bad["empty"] + [[G] * 1001], errors="none")
out["py_none"] = [res[0] == composite.create_composite_proof([G]), res[1] is None, res[2] == res[0], res[3] is None]
try:
    z.create_composite_proofs([[G] * 1001]); out["py_unreadable"] = None
except ValueError as e:
    out["py_unreadable"] = str(e)
print(json.dumps(out))
"""

_BATCH = _COMMON + r"""
# argv[2]: "one" (one shard) or "two" (two shards of the library on one GPU: the several-shards path)
if sys.argv[2] == "two":
    _native.init_devices([0, 0])
else:
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
    api.install_proving_key(kind, open(os.path.join(GOLD, name), "rb").read())
out["shards"] = int(L.zkp_hip_device_count())
ops = [("range", 5000, 1000, 1000 + 2**20), ("threshold", [10, 20, 30], 55), ("equality", 777, 777), ("membership", 9, [7, 8, 9, 11]),
       ("improvement", 5, 500), ("consistency", [1, 5, 5, 9])]
seeds = bytes(np.random.default_rng(1007).integers(0, 256, 32 * len(ops), dtype=np.uint8))
counts = [1, 2, 3]
meta = [{"issuer": b"acme", "n": u32(0)}, {}, {"z": b"last", "a": bytes(40)}]
envs = api.process_ops(ops, seeds)
out["schemes"] = [e[1] for e in envs]
want = [composite.create_proof_with_metadata(envs[0], meta[0]), composite.create_composite_proof(envs[1:3]), composite._serialize_composite(envs[3:6], meta[2])]
z.seal_counters(reset=True)
got = z.process_ops_sealed(ops, counts, meta, seeds=seeds)
out["sealed"] = {"same": got == want, "counters": z.seal_counters(reset=True), "bytes": sum(len(w) for w in want), "verified": z.verify_composite_proofs(got)}
got_plain = z.process_ops_sealed(ops, counts, None, seeds=seeds)
out["sealed_without_metadata"] = got_plain == [composite.create_composite_proof(envs[0:1]), composite.create_composite_proof(envs[1:3]), composite.create_composite_proof(envs[3:6])]
got_sc = z.process_ops_sealed(ops, counts, meta, seeds=seeds, self_check=True)
out["self_check"] = {"same": got_sc == want, "verified": z.verify_composite_proofs(got_sc), "checked": z.batch_self_check_counters(reset=True)}

# one op that fails validation (a range value outside its bounds): its container alone is not sealed, and the batch stays whole
bad_ops = list(ops); bad_ops[1] = ("range", 5, 1000, 2000)
arr, la, cap, sp = api._marshal_ops(bad_ops, seeds, False)
n = len(bad_ops)
def fetch(batch):
    o, off, st = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_batch_fetch(batch, P(o), cap, P(off), P(st))
    return [rc, hashlib.sha256(o[:int(off[n])].tobytes()).hexdigest(), [int(x) for x in off], st.tolist()], o, off
batch = VP()
assert L.zkp_hip_batch_stage(n, ctypes.byref(arr), P(la), sp, ctypes.byref(batch)) == 0, _native.last_error()
assert L.zkp_hip_batch_prove_async(batch) == 0, _native.last_error()
first = offsets(counts)
wires = [composite._metadata_wire(m) for m in meta]
mblob, moff = np.frombuffer(b"".join(wires), dtype=np.uint8), offsets([len(w) for w in wires])
room = cap + 4 * n + 44 * 3 + int(moff[-1])
sb, soff, sst = np.full(room + 8, 0xA5, dtype=np.uint8), np.zeros(4, dtype=np.uint64), np.full(3, 9, dtype=np.uint8)
rc = L.libzkp_seal_batch(batch, 3, P(first), P(mblob), P(moff), P(sb), room, P(soff), P(sst))
after, o, off = fetch(batch)
L.zkp_hip_batch_free(batch)
batch = VP()
assert L.zkp_hip_batch_stage(n, ctypes.byref(arr), P(la), sp, ctypes.byref(batch)) == 0, _native.last_error()
assert L.zkp_hip_batch_prove_async(batch) == 0, _native.last_error()
alone, _, _ = fetch(batch)
L.zkp_hip_batch_free(batch)
raw = o.tobytes()
e = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
soff = [int(x) for x in soff]
out["failed_op"] = {"rc": rc, "status": sst.tolist(), "off": soff, "op_status_nonzero": [i for i, s in enumerate(after[3]) if s != 0],
                    "same": [sb[soff[0]:soff[1]].tobytes() == composite.create_proof_with_metadata(e[0], meta[0]), soff[1] == soff[2],
                             sb[soff[2]:soff[3]].tobytes() == composite._serialize_composite(e[3:6], meta[2])],
                    "guards": bool((sb[soff[3]:] == 0xA5).all()), "fetch_after_seal": after, "fetch_alone": alone}
try:
    z.process_ops_sealed(bad_ops, counts, meta, seeds=seeds); out["py_failed_op"] = None
except api.ZkpBackendError as ex:
    out["py_failed_op"] = str(ex)
print(json.dumps(out))
"""


def _child(script, *args):
    r = subprocess.run([sys.executable, "-c", script, ROOT] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def host():
    return _child(_HOST)


@pytest.fixture(scope="module", params=["one", "two"])
def batch(request):
    return request.param, _child(_BATCH, request.param)


def test_a_wave_and_six_lanes_of_containers_get_the_reference_bytes(host):
    w = host["wave"]
    want = [2 if i in (13, 64) else 1 for i in range(70)]
    assert w["rc"] == 1 and w["status"] == want and w["same"] == [True] * 70 and w["guards"]
    c = w["counters"]
    assert {k: c[k] for k in w["expect"]} == w["expect"] and c["ms"] > 0


def test_everything_sealed_is_read_back_by_the_verifier_and_by_parse_composite(host):
    r = host["round_trip"]
    assert r["rc"] == 0 and r["status"] == [1] * 68 and r["parsed"] == [True] * 68
    assert host["families_verify"] == [0, True]
    assert host["limits_verify"] == [0, [1] * sum(s == 1 for s in host["limits"]["want"])]


def test_residues_and_straddles_get_the_reference_bytes(host):
    f = host["families"]
    assert f["rc"] == 0 and f["n"] == 131 + 8 * 64 and f["status_all_1"] and f["same"] == f["n"] and f["guards"]


def test_the_limits_on_both_sides(host):
    m = host["limits"]
    assert m["rc"] == 1 and m["status"] == m["want"] and m["same"] == [True] * len(m["want"]) and m["guards"]
    assert m["four_mib"] == [4 << 20, True] and {1, 2, 3} == set(m["want"])


def test_out_cap_n_0_and_argument_errors(host):
    c = host["out_cap"]
    assert c["rc"] == [1, -3] and c["need"][0] == c["need"][1] == c["need"][2] and c["untouched"] and "out_off[n] holds the required size" in c["msg"]
    assert c["status"] == [[1, 2, 1], [1, 2, 1]]
    assert host["n0"] == 0 and host["arguments"] == [-3] * 10


def test_python_front_end(host):
    assert host["py"] == [True] * 4 and host["py_none"] == [True] * 4
    r = host["py_raise"]
    for name in ("empty", "malformed", "short"):
        assert r[name][0] is not None and r[name][0] == r[name][1], name
    assert r["empty"][0] == ["ValueError", "proof list cannot be empty"] and r["malformed"][0][0] == "ProofFormatError" and "mismatch" in r["malformed"][0][1]
    assert host["py_unreadable"] is not None and "too many items: proofs=1001" in host["py_unreadable"]


def test_a_proved_batch_is_sealed_into_the_bytes_of_the_host_functions(batch):
    which, b = batch
    assert b["shards"] == (1 if which == "one" else 2) and sorted(b["schemes"]) == [1, 2, 3, 4, 5, 6]
    s = b["sealed"]
    assert s["same"] and s["verified"] == [True] * 3 and b["sealed_without_metadata"]
    c = s["counters"]
    assert (c["containers"], c["sealed"], c["envelopes"], c["bytes"]) == (3, 3, 6, s["bytes"]) and c["ms"] > 0


def test_a_self_checked_batch_is_sealed_the_same(batch):
    _, b = batch
    s = b["self_check"]
    assert s["same"] and s["verified"] == [True] * 3 and (s["checked"]["launches"], s["checked"]["point_adds"]) == (6, 0)


def test_a_failed_op_fails_its_container_alone_and_the_batch_stays_whole(batch):
    _, b = batch
    f = b["failed_op"]
    assert f["rc"] == 1 and f["status"] == [1, 0, 1] and f["op_status_nonzero"] == [1] and f["same"] == [True] * 3 and f["guards"]
    assert f["fetch_after_seal"] == f["fetch_alone"] and f["fetch_alone"][0] == 1
    assert b["py_failed_op"] is not None and "container 1" in b["py_failed_op"]


def test_cpp_program_seals_through_the_header_alone():
    import __graft_entry__ as ge
    exe = ge.build_abi_seal_caller()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "abi_call_seal ok: 3 symbols" in r.stdout
