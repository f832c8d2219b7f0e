"""Hot/cold engine storage and the LDS lane kernel (lane mode 4).

CPU: the event heap's hot tier must not change a single pop.
GPU: conv_lds_kernel keeps Engine::Hot in a per-lane LDS slice; within a
trial the event order cannot depend on where the state lives, so every
comparison against the scratch kernels (modes 2 and 3) is bitwise.
"""
import os
from contextlib import contextmanager

import pytest

import cimba_amd as ca

KEYS = ("per_trial_avg", "total_wait", "total_events", "trials_ok")


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def assert_same(a, b, keys=KEYS, what=""):
    for k in keys:
        assert a[k] == b[k], (what, k)


# ---- CPU -----------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 0xDEADBEEF])
def test_hashheap_hot_tier_pop_sequence(seed):
    """One seeded push/pop/cancel/reschedule sequence, 20000 ops, against
    HashHeap<16> with 0, 1, 2 and 4 hot entries: identical pops."""
    ref = ca._C.hashheap_tier_fuzz(seed, 20000, 0)
    assert len(ref) > 2000
    for hot in (1, 2, 4):
        assert ca._C.hashheap_tier_fuzz(seed, 20000, hot) == ref, hot


def test_hashheap_tier_fuzz_rejects_other_sizes():
    with pytest.raises(ValueError):
        ca._C.hashheap_tier_fuzz(1, 10, 3)


# ---- GPU -----------------------------------------------------------------

gpu = pytest.mark.gpu


def mm1(mode, ntrials, objs, seed, **extra):
    with env(CIMBA_MM1_LANE=mode, **extra):
        r = ca.mm1_gpu(ntrials=ntrials, num_objects=objs, seed=seed, device=0)
    assert r["trials_ok"] == ntrials, (mode, r["first_bad_status"])
    return r


@gpu
def test_lds_mm1_partial_wave():
    """200 trials = three full waves + one with 8 live lanes: the lanes
    without a trial never touch their LDS slice and must not disturb
    the others."""
    lds = mm1(4, 200, 2000, 21)
    for mode in (2, 3):
        assert_same(lds, mm1(mode, 200, 2000, 21), what=mode)


@gpu
def test_lds_mm1_refill_reinitialises_lds():
    """8 workgroups of 64 lanes for 2048 trials: four wave-synchronous
    refills per lane, so init() must rebuild the whole LDS state."""
    lds = mm1(4, 2048, 2000, 99, CIMBA_CONV_BLOCKS=8)
    for mode in (2, 3):
        assert_same(lds, mm1(mode, 2048, 2000, 99), what=mode)


@gpu
def test_lds_mm1_minw2_same_results():
    """The 2-waves/SIMD instantiation computes the same trials."""
    a = mm1(4, 200, 2000, 5)
    b = mm1(4, 200, 2000, 5, CIMBA_LDS_MINW=2)
    assert_same(a, b)


@gpu
def test_lds_mg1_matches_conv():
    kw = dict(ntrials=1024, num_objects=2000, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=7, device=0)
    with env(CIMBA_MG1_LANE=4):
        lds = ca.mg1_gpu(**kw)
    with env(CIMBA_MG1_LANE=3):
        conv = ca.mg1_gpu(**kw)
    assert lds["trials_ok"] == 1024, lds["first_bad_status"]
    keys = [k for k in KEYS if k in conv] + ["avg_system_time",
                                             "avg_queue_time"]
    assert "per_trial_avg" in keys and "total_events" in keys
    assert_same(lds, conv, keys)


@gpu
def test_mm1hot1_crosses_the_tier_boundary():
    """MM1Hot1 keeps ONE heap entry hot, so its second pending event
    lives in scratch and every sift crosses the boundary."""
    hot1 = ca._C.mm1hot1_gpu(ntrials=256, num_objects=2000, seed=31, device=0)
    assert hot1["trials_ok"] == 256, hot1["first_bad_status"]
    assert_same(hot1, mm1(3, 256, 2000, 31))


@gpu
def test_lds_mm1_deterministic():
    assert_same(mm1(4, 64, 5000, 3), mm1(4, 64, 5000, 3))
