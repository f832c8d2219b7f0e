"""Device tally stream on the GPU: the tallied M/M/1 model through every
kernel shape against the host engine (summaries byte for byte, histograms
exactly), and the pooling kernel alone."""
import functools

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C

NBINS = 770
GPU = dict(num_objects=20, arr_rate=0.9, srv_rate=1.0, seed=7)
KERNELS = ("wave", "lane", "scratch", "conv", "lds")
TOTALS = ("total_events", "total_wait", "total_objects", "per_trial_avg")
# the pooling kernel's trial slab (REDUCE_SLAB in hip/tally_kernel.hip)
SLAB = 256

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def host_ref(**kw):
    """mm1tally_host results, computed once per argument set and shared."""
    r = ca.mm1tally_host(threads=1, per_trial_hist=True, **kw)
    for k in ("tally_summaries", "tally_hist", "tally_trial_hist"):
        r[k].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def plain_gpu(ntrials):
    return ca.mm1_gpu(ntrials=ntrials, **GPU)


def check_against_host(kw):
    g = ca.mm1tally_gpu(per_trial_hist=True, **kw)
    h = host_ref(**{k: v for k, v in kw.items()
                    if k not in ("kernel", "blocks")})
    assert g["tally_first"] == h["tally_first"]
    assert g["tally_summaries"].shape == h["tally_summaries"].shape
    assert g["tally_summaries"].tobytes() == h["tally_summaries"].tobytes()
    assert np.array_equal(g["tally_trial_hist"], h["tally_trial_hist"])
    assert np.array_equal(g["tally_hist"], h["tally_hist"])
    assert g["tally_hist"].dtype == np.uint64
    plain = plain_gpu(kw["ntrials"])
    for k in TOTALS:
        assert g[k] == plain[k], k
    return g


@pytest.mark.parametrize("kernel", KERNELS)
def test_partial_last_wave_or_block(kernel):
    g = check_against_host(dict(GPU, ntrials=257, kernel=kernel))
    assert g["tally_summaries"].shape == (257, 2)
    assert np.all(g["tally_summaries"]["n"] == 20)
    assert g["tally_hist"].sum() == 257 * 2 * 20


@pytest.mark.parametrize("kernel", KERNELS)
def test_stride_loop_rebinds(kernel):
    # one block: a lane (or wave) runs several trials, so every bind must
    # reset its own headers and leave the earlier slots alone
    g = check_against_host(dict(GPU, ntrials=600, blocks=1, kernel=kernel))
    assert np.all(g["tally_summaries"]["n"] == 20)


@pytest.mark.parametrize("kernel", KERNELS)
def test_window_leaves_no_trace_outside(kernel):
    g = check_against_host(dict(GPU, ntrials=257, tally_first=100,
                                tally_count=57, kernel=kernel))
    assert g["tally_first"] == 100
    assert g["tally_summaries"].shape == (57, 2)
    assert g["tally_trial_hist"].shape == (57, 2, NBINS)
    assert g["tally_hist"].sum() == 57 * 2 * 20


@pytest.mark.parametrize("kernel", KERNELS)
def test_empty_window(kernel):
    g = ca.mm1tally_gpu(ntrials=257, tally_count=0, per_trial_hist=True,
                        kernel=kernel, **GPU)
    assert g["tally_summaries"].shape == (0, 2)
    assert g["tally_trial_hist"].shape == (0, 2, NBINS)
    assert g["tally_hist"].shape == (2, NBINS) and not g["tally_hist"].any()
    plain = plain_gpu(257)
    for k in TOTALS:
        assert g[k] == plain[k], k


# 4099 trials span 17 slabs of the pooling kernel, the last one partial
@pytest.mark.parametrize("shape", [(1, 1, NBINS), (257, 2, NBINS),
                                   (4099, 3, NBINS)])
def test_pooling_kernel_alone(shape):
    assert 4099 > SLAB
    rng = np.random.default_rng(shape[0])
    rows = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32)
    # rows of 2^32 - 1: a 32-bit accumulator would wrap
    rows[::3] = 2 ** 32 - 1
    rows[-1] = 2 ** 32 - 1
    got = _C.tally_reduce_gpu(rows)
    assert got.dtype == np.uint64 and got.shape == shape[1:]
    assert np.array_equal(got, rows.sum(axis=0, dtype=np.uint64))
    if shape[0] > 1:
        assert got.max() > 2 ** 32
