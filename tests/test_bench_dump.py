"""bench.py --dump-outputs: what a plain run writes (GPU), and the seeded sample of a large batch (CPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from byzantinerandomizedconsensus_amd import _lib as L  # noqa: E402

INSTANCES = 4096
NAMES = {"stats", "round_hist", "decisions", "sample_ids", "instances", "replicas"}


class FakeEngine:
    """Engine's read interface over zeros: sample_outputs() touches nothing else."""

    def __init__(self, instances, offset):
        self.instances, self.n = instances, 64
        self.cfg = L.Config(instance_offset=offset)
        self.reads = []

    def instances_array(self, first, count):
        assert 0 <= first and first + count <= self.instances
        self.reads.append((first, count))
        return np.ctypeslib.as_array((L.InstanceResult * count)()).copy()

    def replicas_array(self, first, count):
        assert 0 <= first and first + count <= self.instances
        return np.ctypeslib.as_array((L.ReplicaResult * (count * self.n))()).reshape(count, self.n).copy()


def test_sample_of_a_large_batch_is_fixed_and_bounded():
    a = bench.sample_outputs(FakeEngine(1 << 20, 1 << 20))
    b = bench.sample_outputs(FakeEngine(1 << 20, 1 << 20))
    s = bench.DUMP_BLOCKS * bench.DUMP_BLOCK
    assert a["sample_ids"].shape == (s,) and np.array_equal(a["sample_ids"], b["sample_ids"])
    ids = a["sample_ids"]
    assert len(set(ids.tolist())) == s and np.all(np.diff(ids) > 0)          # distinct blocks, ascending
    assert ids.min() >= 1 << 20 and ids.max() < 2 << 20                       # global ids of this engine
    assert a["instances"].shape == (s, len(L.InstanceResult._fields_)) and a["instances"].dtype == np.float64
    assert a["replicas"].shape == (s, 64, len(L.ReplicaResult._fields_)) and a["replicas"].dtype == np.float32
    assert sum(v.nbytes for v in a.values()) <= 64e6
    # a batch no larger than the sample is dumped whole, and one a block larger is sampled
    small = FakeEngine(s, 0)
    assert np.array_equal(bench.sample_outputs(small)["sample_ids"], np.arange(s)) and small.reads == [(0, s)]
    assert bench.sample_outputs(FakeEngine(s + bench.DUMP_BLOCK, 0))["sample_ids"].shape == (s,)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_steps_results(tmp_path):
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--instances", str(INSTANCES), "--dump-outputs", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert not [k for k in d if k.endswith("_leg")] and "cpu_baseline" not in d     # those are --full's
    arrays = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(arrays) == NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    # the totals are the result line's
    stats = dict(zip((k for k, _ in L.Stats._fields_), arrays["stats"].tolist()))
    for k, v in d["counts"].items():
        assert stats[k] == v, k
    assert {str(r): c for r, c in enumerate(arrays["round_hist"].tolist()) if c} == d["decide_round_hist"]
    # the per-instance and per-replica arrays are the engine's own reads of the same workload
    eng = bench.make_engine("reference", INSTANCES, 0, 0, 1)
    try:
        eng.run()
        inst, repl = eng.instances_array(), eng.replicas_array()
    finally:
        eng.close()
    assert np.array_equal(arrays["sample_ids"], np.arange(INSTANCES))
    for j, (k, _) in enumerate(L.InstanceResult._fields_):
        assert np.array_equal(arrays["instances"][:, j], inst[k].astype(np.float64)), k
    for j, (k, _) in enumerate(L.ReplicaResult._fields_):
        assert np.array_equal(arrays["replicas"][:, :, j], repl[k].astype(np.float32)), k
    assert arrays["instances"][:, 6].sum() == d["counts"]["cell_steps"]
