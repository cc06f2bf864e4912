"""bench.py --dump-outputs (no GPU): the packed results of a batch as float .npy files, whole when they fit the 64 MB budget,
else a seeded sample of ops that does not depend on what the build computed."""
import os

import numpy as np

import bench
from libzkp_amd import workloads as wl


def _packed(n):
    ops, _, _ = wl.mixed_ops(n, 5)
    rng = np.random.default_rng(1)
    k = ops["kind"]
    lens = np.where(k == wl.OP_RANGE, wl.RANGE_BYTES, np.where(k == wl.OP_EQUALITY, wl.EQUALITY_BYTES,
                    np.where(k == wl.OP_MEMBERSHIP, wl.membership_bytes(16), rng.integers(2000, wl.IMPROVEMENT_MAX_BYTES, n))))
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return ops, rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off, np.zeros(n, dtype=np.int32)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_whole_batch_round_trips(tmp_path):
    ops, out, off, st = _packed(4096)
    info = bench.dump_outputs(str(tmp_path), ops, out, off, st)
    a = _load(str(tmp_path))
    assert sorted(a) == ["op_index", "proof_bytes", "proof_lengths", "status"]
    assert a["proof_bytes"].dtype == np.float32 and a["proof_lengths"].dtype == np.float64 and a["status"].dtype == np.float32
    assert info["ops_with_bytes"] == 4096 and (a["op_index"] == np.arange(4096)).all()
    assert (a["proof_bytes"].astype(np.uint8) == out).all() and (a["proof_lengths"] == np.diff(off.astype(np.int64))).all()


def test_large_batch_is_a_fixed_sample_under_the_budget(tmp_path):
    ops, out, off, st = _packed(16384)
    bench.dump_outputs(str(tmp_path / "a"), ops, out, off, st)
    a = _load(str(tmp_path / "a"))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= bench.DUMP_BUDGET_BYTES
    idx = a["op_index"].astype(np.int64)
    assert 0 < len(idx) < 16384 and (np.diff(idx) > 0).all()
    assert (a["proof_bytes"].astype(np.uint8) == np.concatenate([out[int(off[i]):int(off[i + 1])] for i in idx])).all()
    out2 = out.copy()
    out2[:] = 7                                                       # other proof bytes (another build): the same ops are sampled
    bench.dump_outputs(str(tmp_path / "b"), ops, out2, off, st)
    assert (np.load(str(tmp_path / "b" / "op_index.npy")) == a["op_index"]).all()
