"""Split dispatch (engine.hpp dispatch_head / dispatch_body / dispatch_tail)
and the fused loop of the LDS lane kernel that is built on it (lane mode 5,
hip/deskernel_impl.hpp fused_trial_loop).

A split engine flavour does not draw and schedule an exponential hold in
the process body: CMB_HOLD_EXP records it, the body returns, and
dispatch_tail() commits it before the next event is popped.  Each lane's
draws and events therefore come in the same order as on a plain flavour,
and no result may differ in any bit.

CPU: M/M/1 and M/G/1 on the split host flavour against the plain one, run
to the end, cut by `until` in mid-trial, and ended by the event limit.
GPU: mode 5 against the voted loop (mode 4) and the host engine, at a
partial wave, over several wave-synchronous refills with a partial last
round, under an `until` that ends the lanes at different iterations, and
through the two test models that share the loop.
"""
import os
from contextlib import contextmanager

import pytest

import cimba_amd as ca

KEYS = ("per_trial_avg", "total_wait", "total_events", "trials_ok",
        "first_bad_status")
MG1_KEYS = ("per_trial_avg", "total_events", "trials_ok", "avg_system_time",
            "avg_queue_time", "first_bad_status")
ST_EVENT_LIMIT = 6
SEEDS = (3, 17, 0xC0FFEE)


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

# 200 objects at rate 0.9 (0.8 for M/G/1) take about 220 (250) time units
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("until", [1.0e308, 110.0])
def test_host_split_equals_plain_mm1(seed, until):
    kw = dict(ntrials=8, num_objects=200, seed=seed, threads=1, until=until)
    ref = ca.mm1_host(**kw)
    assert_same(ca.mm1_host(split_dispatch=True, **kw), ref)
    assert ref["trials_ok"] == 8
    if until < 1.0e308:  # every trial was cut with work left
        assert 8 * 20 < ref["total_objects"] < 8 * 190


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("until", [1.0e308, 125.0])
@pytest.mark.parametrize("dist", [0, 3])
def test_host_split_equals_plain_mg1(seed, until, dist):
    """dist 0 draws the service time with the exponential that the arrival
    hold defers, dist 3 with the normal: the two share one RNG stream."""
    kw = dict(ntrials=8, num_objects=200, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=dist, seed=seed, threads=1, until=until)
    ref = ca.mg1_host(**kw)
    assert_same(ca.mg1_host(split_dispatch=True, **kw), ref, MG1_KEYS)
    assert ref["trials_ok"] == 8
    if until < 1.0e308:
        assert ref["total_events"] < 8 * 600


@pytest.mark.parametrize("seed", SEEDS)
def test_host_split_event_limit(seed):
    """Every trial stops at its 300th event with ST_EVENT_LIMIT, the hold of
    that event committed as on the plain flavour."""
    kw = dict(ntrials=8, num_objects=200, seed=seed, threads=1, max_events=300)
    ref = ca.mm1_host(**kw)
    assert ref["trials_ok"] == 0 and ref["first_bad_status"] == ST_EVENT_LIMIT
    assert ref["total_events"] == 8 * 300
    assert_same(ca.mm1_host(split_dispatch=True, **kw), ref)
    kw = dict(ntrials=8, num_objects=200, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=seed, threads=1, max_events=300)
    ref = ca.mg1_host(**kw)
    assert ref["trials_ok"] == 0 and ref["first_bad_status"] == ST_EVENT_LIMIT
    assert_same(ca.mg1_host(split_dispatch=True, **kw), ref, MG1_KEYS)


def test_host_split_takes_no_window():
    with pytest.raises(ValueError):
        ca.mm1_host(ntrials=1, num_objects=10, split_dispatch=True,
                    queue_window=8)
    with pytest.raises(ValueError):
        ca.mg1_host(ntrials=1, num_objects=10, split_dispatch=True,
                    front_cache=True)


# ---- GPU -----------------------------------------------------------------

gpu = pytest.mark.gpu


def mm1(mode, ntrials, objs, seed, **kw):
    extra = {k: kw.pop(k) for k in list(kw) if k.startswith("CIMBA_")}
    with env(CIMBA_MM1_LANE=mode, **extra):
        return ca.mm1_gpu(ntrials=ntrials, num_objects=objs, seed=seed,
                          device=0, **kw)


def mm1_three_ways(ntrials, objs, seed, until=1.0e308, **envkw):
    host = ca.mm1_host(ntrials=ntrials, num_objects=objs, seed=seed,
                       threads=1, until=until)
    voted = mm1(4, ntrials, objs, seed, until=until, **envkw)
    fused = mm1(5, ntrials, objs, seed, until=until, **envkw)
    assert fused["trials_ok"] == ntrials, fused["first_bad_status"]
    assert_same(fused, voted, what="mode 4")
    assert_same(fused, host, what="host")
    return fused


@gpu
@pytest.mark.timeout(60)
def test_fused_partial_wave():
    """70 trials: one full wave and one with six live lanes."""
    mm1_three_ways(70, 100, 11)


@gpu
@pytest.mark.timeout(60)
def test_fused_refill_rounds():
    """One 64-lane workgroup for 200 trials: four wave-synchronous refills,
    the last with eight live lanes."""
    mm1_three_ways(200, 60, 12, CIMBA_CONV_BLOCKS=1)


@gpu
@pytest.mark.timeout(60)
def test_fused_until_cuts_lanes_apart():
    """300 objects take about 333 time units; at until = 165 each lane's
    next event passes the limit at an iteration of its own."""
    r = mm1_three_ways(64, 300, 13, until=165.0)
    assert 64 * 50 < r["total_objects"] < 64 * 250


@gpu
@pytest.mark.timeout(60)
def test_fused_mg1():
    kw = dict(ntrials=70, num_objects=100, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=14)
    host = ca.mg1_host(threads=1, **kw)
    with env(CIMBA_MG1_LANE=4):
        voted = ca.mg1_gpu(device=0, **kw)
    with env(CIMBA_MG1_LANE=5):
        fused = ca.mg1_gpu(device=0, **kw)
    assert fused["trials_ok"] == 70, fused["first_bad_status"]
    assert_same(fused, voted, MG1_KEYS, what="mode 4")
    assert_same(fused, host, MG1_KEYS, what="host")


@gpu
@pytest.mark.timeout(60)
def test_fused_test_models():
    """MM1Rec (cold statistics records) and MM1Hot1 (one hot heap entry)
    route through the same loop."""
    kw = dict(ntrials=64, num_objects=100, seed=15)
    voted = ca._C.mm1rec_gpu(device=0, lane_mode=4, **kw)
    fused = ca._C.mm1rec_gpu(device=0, lane_mode=5, **kw)
    assert fused["trials_ok"] == 64
    assert_same(fused, voted, what="mm1rec")
    with env(CIMBA_MM1_LANE=4):
        voted = ca._C.mm1hot1_gpu(device=0, **kw)
    with env(CIMBA_MM1_LANE=5):
        fused = ca._C.mm1hot1_gpu(device=0, **kw)
    assert fused["trials_ok"] == 64
    assert_same(fused, voted, what="mm1hot1")
    assert_same(fused, ca.mm1_host(threads=1, **kw), what="host")
