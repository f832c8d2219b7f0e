"""Multi-process (gloo, world_size=2) tests of the distributed statistics
reduction — the CPU-testable half of the RCCL/xGMI fan-out (SURVEY.md
§5.8: cross-trial merge becomes a rank reduce)."""
import multiprocessing as mp
import os

import numpy as np
import pytest


def _dist_worker(rank, world, port, q):
    os.environ.update({
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
        "RANK": str(rank),
        "WORLD_SIZE": str(world),
    })
    import torch.distributed as dist

    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    import cimba_amd as ca
    from cimba_amd.parallel import (allreduce_datasummary,
                                    allreduce_wtdsummary, shard_range)

    # each rank summarizes its shard of a known dataset
    data = np.arange(1000, dtype=np.float64) * 0.5 + 3.0
    lo, hi = shard_range(len(data), rank, world)
    ds = ca.DataSummary()
    for v in data[lo:hi]:
        ds.add(v)
    merged = allreduce_datasummary(ds)

    ws = ca.WtdSummary()
    for v in data[lo:hi]:
        ws.add(v, 0.25 + (v % 1.0))
    wmerged = allreduce_wtdsummary(ws)

    if rank == 0:
        q.put({
            "n": merged.count(),
            "mean": merged.mean(),
            "var": merged.variance(),
            "wmean": wmerged.mean(),
            "wsum": wmerged.sumw(),
        })
    dist.destroy_process_group()


def test_allreduce_summaries_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29511
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
    data = np.arange(1000, dtype=np.float64) * 0.5 + 3.0
    w = 0.25 + (data % 1.0)
    assert res["n"] == 1000
    assert abs(res["mean"] - data.mean()) < 1e-12
    assert abs(res["var"] - data.var(ddof=1)) < 1e-9
    assert abs(res["wmean"] - (data * w).sum() / w.sum()) < 1e-12
    assert abs(res["wsum"] - w.sum()) < 1e-12


def test_shard_range():
    from cimba_amd.parallel import shard_range

    covered = []
    for r in range(3):
        lo, hi = shard_range(10, r, 3)
        covered.extend(range(lo, hi))
    assert covered == list(range(10))


def test_run_distributed_mm1_single_process():
    # single-process fallback path of the distributed experiment runner
    from cimba_amd.parallel import run_distributed_mm1

    ds, events = run_distributed_mm1(8, 5000, seed=3, use_gpu=False)
    assert ds.count() == 8
    assert 7.0 < ds.mean() < 13.0
    assert events > 8 * 5000


def _dist_mm1_worker(rank, world, port, q):
    os.environ.update({
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
        "RANK": str(rank),
        "WORLD_SIZE": str(world),
    })
    import torch.distributed as dist

    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    from cimba_amd.parallel import run_distributed_mm1

    ds, events = run_distributed_mm1(8, 3000, seed=5, use_gpu=False)
    if rank == 0:
        q.put({"n": ds.count(), "mean": ds.mean(), "events": events})
    dist.destroy_process_group()


def test_run_distributed_mm1_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_mm1_worker, args=(r, 2, 29513, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
    assert res["n"] == 8          # all shards merged
    assert 7.0 < res["mean"] < 13.0
    assert res["events"] > 8 * 3000


def test_trial_base_world_invariance():
    """Sharding by trial_base simulates the identical global trial set:
    two half-shards reproduce the full run bit-exactly."""
    import cimba_amd as ca

    full = ca.mm1_host(ntrials=16, num_objects=500, seed=1234, threads=1)
    a = ca.mm1_host(ntrials=8, num_objects=500, seed=1234, threads=1,
                    trial_base=0)
    b = ca.mm1_host(ntrials=8, num_objects=500, seed=1234, threads=1,
                    trial_base=8)
    assert a["total_events"] + b["total_events"] == full["total_events"]
    assert a["total_objects"] + b["total_objects"] == full["total_objects"]
    assert (a["per_trial_avg"] + b["per_trial_avg"]) == full["per_trial_avg"]


def test_trial_base_world_invariance_all_models():
    """The same shard/full bit-equality for MG1 and JobShop (the other
    BASELINE configs the scaling bench can run)."""
    import cimba_amd as ca

    full = ca.mg1_host(ntrials=8, num_objects=300, srv_scv=2.0, dist=2,
                       seed=77, threads=1)
    a = ca.mg1_host(ntrials=4, num_objects=300, srv_scv=2.0, dist=2,
                    seed=77, threads=1, trial_base=0)
    b = ca.mg1_host(ntrials=4, num_objects=300, srv_scv=2.0, dist=2,
                    seed=77, threads=1, trial_base=4)
    assert a["total_events"] + b["total_events"] == full["total_events"]
    assert (a["per_trial_avg"] + b["per_trial_avg"]) == full["per_trial_avg"]

    fullj = ca.jobshop_host(ntrials=6, entities=200, njobs=12, seed=5,
                            threads=1)
    aj = ca.jobshop_host(ntrials=3, entities=200, njobs=12, seed=5,
                         threads=1, trial_base=0)
    bj = ca.jobshop_host(ntrials=3, entities=200, njobs=12, seed=5,
                         threads=1, trial_base=3)
    assert aj["total_events"] + bj["total_events"] == fullj["total_events"]


def test_bench_self_launch_host():
    """`python bench.py --gpus 2 --host` must self-launch 2 ranks (no
    external torch.distributed.run) and report the ACTUAL world size
    (VERDICT r01 item 1)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run(
        [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
         "--host", "--steps", "1", "--warmup", "0", "--trials", "8",
         "--objects", "200"],
        capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    rep = json.loads(line)
    assert rep["n_gpus"] == 2
    assert rep["value"] > 0
    assert rep["config"]["parallelism"] == "trial-parallel dp2"


@pytest.mark.parametrize("model", ["mg1", "jobshop"])
def test_bench_model_flags_self_launch_host(model):
    """BASELINE configs 3-4 through the same self-launch contract."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run(
        [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
         "--host", "--model", model, "--steps", "1", "--warmup", "0",
         "--trials", "4", "--objects", "200"],
        capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads([l for l in out.stdout.splitlines()
                      if l.startswith("{")][-1])
    assert rep["n_gpus"] == 2 and rep["value"] > 0


def test_bench_dump_outputs_host(tmp_path):
    """`--dump-outputs DIR` writes the last timed step's results as
    float64 .npy files; same arguments -> identical files, and --steps
    really selects which step is the last one."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(outdir, steps):
        out = subprocess.run(
            [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1",
             "--host", "--steps", str(steps), "--warmup", "0", "--trials",
             "8", "--objects", "200", "--dump-outputs", str(outdir)],
            capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        rep = json.loads([l for l in out.stdout.splitlines()
                          if l.startswith("{")][-1])
        assert rep["steps"] == steps and rep["ms_per_step"] > 0
        return {f: np.load(os.path.join(outdir, f))
                for f in sorted(os.listdir(outdir))}

    a = run(tmp_path / "a", 2)
    b = run(tmp_path / "b", 2)
    c = run(tmp_path / "c", 1)
    assert "per_trial_avg.npy" in a and "total_events.npy" in a
    assert not any("elapsed" in k or "per_sec" in k for k in a)
    assert a["per_trial_avg.npy"].shape == (8,)
    assert a.keys() == b.keys() == c.keys()
    for k in a:
        assert a[k].dtype == np.float64
        assert np.array_equal(a[k], b[k]), k
    # step 0 and step 1 use different seeds
    assert not np.array_equal(a["per_trial_avg.npy"], c["per_trial_avg.npy"])
