"""allreduce_histogram at world size 2 over gloo: the pooled tally
histograms of two half-shards sum to the single-run histogram."""
import multiprocessing as mp
import os

import numpy as np

KW = dict(num_objects=100, arr_rate=0.9, srv_rate=1.0, seed=5, threads=1)


def _hist_worker(rank, world, port, q):
    os.environ.update({
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
        "RANK": str(rank),
        "WORLD_SIZE": str(world),
    })
    import torch.distributed as dist

    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    import cimba_amd as ca
    from cimba_amd.parallel import allreduce_histogram, shard_range

    lo, hi = shard_range(8, rank, world)
    r = ca.mm1tally_host(ntrials=hi - lo, trial_base=lo, **KW)
    local = r["tally_hist"].copy()
    # a count past 2^32 must survive the reduction
    local[1, 769] = (1 << 40) + rank
    merged = allreduce_histogram(local)
    if rank == 0:
        q.put(merged)
    dist.destroy_process_group()


def test_allreduce_histogram_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_hist_worker, args=(r, 2, 29517, q))
             for r in range(2)]
    for p in procs:
        p.start()
    merged = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
    import cimba_amd as ca

    full = ca.mm1tally_host(ntrials=8, **KW)["tally_hist"]
    assert merged.dtype == np.uint64 and merged.shape == full.shape
    assert merged[1, 769] == (1 << 41) + 1
    merged[1, 769] = full[1, 769]
    assert np.array_equal(merged, full)
    assert merged.sum() == 2 * 8 * 100


def test_allreduce_histogram_single_process():
    from cimba_amd.parallel import allreduce_histogram

    h = np.arange(2 * 770, dtype=np.uint64).reshape(2, 770)
    out = allreduce_histogram(h)
    assert out.dtype == np.uint64 and np.array_equal(out, h)
