"""The event heap's register tier (hashheap.hpp, R = min(HOT, EVREG)) and
the LDS lane kernel built on it (lane mode 6, hip/deskernel_impl.hpp
conv_lds_regheap_kernel).

A flavour with a register tier keeps heap indices [0, R) in the heap view
instead of the hot array.  Index i is the same binary-heap position either
way, so every pop comes out in the same order and no result may differ in
any bit; the flavour's Engine::Hot is smaller by the R entries.

CPU: M/M/1 and M/G/1 on the host flavour (heap_regs=True, FlatRegTier)
against the plain one, run to the end, cut by `until` in mid-trial, and
ended by the event limit; the LDS plans of mode 6.  The heap itself is
fuzzed in lockstep against the plain heap by the stand-alone sanitizer
program csrc/host/heapregfuzz_main.cpp.
GPU: mode 6 against mode 5 and the host engine, at a partial wave, over
several wave-synchronous refills with a partial last round, under an
`until` that ends the lanes at different iterations, at the event limit,
and through the two test models: MM1Hot1 has one hot entry, so R = 1 and
its second event is cold, and every push and pop crosses from the register
to scratch.
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
def test_host_heap_regs_equals_plain_mm1(seed, until):
    kw = dict(ntrials=8, num_objects=200, seed=seed, threads=1, until=until)
    ref = ca.mm1_host(**kw)
    assert_same(ca.mm1_host(heap_regs=True, **kw), ref)
    assert ref["trials_ok"] == 8
    if until < 1.0e308:  # every trial was cut with work left
        assert 8 * 20 < ref["total_objects"] < 8 * 190


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("until", [1.0e308, 110.0])
@pytest.mark.parametrize("dist", [0, 3])
def test_host_heap_regs_equals_plain_mg1(seed, until, dist):
    kw = dict(ntrials=8, num_objects=200, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=dist, seed=seed, threads=1, until=until)
    ref = ca.mg1_host(**kw)
    assert_same(ca.mg1_host(heap_regs=True, **kw), ref, MG1_KEYS)
    assert ref["trials_ok"] == 8
    if until < 1.0e308:
        assert ref["total_events"] < 8 * 600


@pytest.mark.parametrize("seed", SEEDS)
def test_host_heap_regs_event_limit(seed):
    """Every trial stops at its 300th event with ST_EVENT_LIMIT."""
    kw = dict(ntrials=8, num_objects=200, seed=seed, threads=1, max_events=300)
    ref = ca.mm1_host(**kw)
    assert ref["trials_ok"] == 0 and ref["first_bad_status"] == ST_EVENT_LIMIT
    assert ref["total_events"] == 8 * 300
    assert_same(ca.mm1_host(heap_regs=True, **kw), ref)
    for dist in (0, 3):
        kw = dict(ntrials=8, num_objects=200, arr_rate=0.8, srv_mean=1.0,
                  srv_scv=0.25, dist=dist, seed=seed, threads=1,
                  max_events=300)
        ref = ca.mg1_host(**kw)
        assert ref["trials_ok"] == 0
        assert ref["first_bad_status"] == ST_EVENT_LIMIT
        assert_same(ca.mg1_host(heap_regs=True, **kw), ref, MG1_KEYS)


def test_host_heap_regs_takes_no_window():
    with pytest.raises(ValueError):
        ca.mm1_host(ntrials=1, num_objects=10, heap_regs=True, queue_window=8)
    with pytest.raises(ValueError):
        ca.mg1_host(ntrials=1, num_objects=10, heap_regs=True,
                    front_cache=True)


def test_regheap_lds_layout():
    """Both hot heap entries (2 x 40 B) leave the lane slice: M/M/1 goes
    from 312 B and 8 waves per CU to 232 B and 11, M/G/1 from 376 B and 6
    to 296 B and 8.  The plans of modes 4 and 5 stay what they were."""
    old, new = ca._C.lds_layout("mm1"), ca._C.lds_layout("mm1_regheap")
    assert new["hot_bytes"] == old["hot_bytes"] - 80
    assert (new["lane_stride"], new["waves_per_cu"]) == (232, 11)
    assert (old["lane_stride"], old["waves_per_cu"]) == (312, 8)
    old, new = ca._C.lds_layout("mg1"), ca._C.lds_layout("mg1_regheap")
    assert new["hot_bytes"] == old["hot_bytes"] - 80
    assert (new["lane_stride"], new["waves_per_cu"]) == (296, 8)
    assert (old["lane_stride"], old["waves_per_cu"]) == (376, 6)
    for lay in (ca._C.lds_layout("mm1_regheap"),
                ca._C.lds_layout("mg1_regheap")):
        s = lay["lane_stride"]
        assert s >= lay["hot_bytes"] and s % 8 == 0 and (s // 8) % 2 == 1
        assert lay["waves_per_cu"] == 160 * 1024 // (64 * s)
    with pytest.raises(ValueError):
        ca._C.lds_layout("mm1_regs")


# ---- GPU -----------------------------------------------------------------

gpu = pytest.mark.gpu


def mm1(mode, ntrials, objs, seed, **kw):
    extra = {k: kw.pop(k) for k in list(kw) if k.startswith("CIMBA_")}
    with env(CIMBA_MM1_LANE=mode, **extra):
        return ca.mm1_gpu(ntrials=ntrials, num_objects=objs, seed=seed,
                          device=0, **kw)


def mm1_three_ways(ntrials, objs, seed, until=1.0e308,
                   max_events=2**64 - 1, **envkw):
    host = ca.mm1_host(ntrials=ntrials, num_objects=objs, seed=seed,
                       threads=1, until=until, max_events=max_events)
    fused = mm1(5, ntrials, objs, seed, until=until, max_events=max_events,
                **envkw)
    regs = mm1(6, ntrials, objs, seed, until=until, max_events=max_events,
               **envkw)
    assert_same(regs, fused, what="mode 5")
    assert_same(regs, host, what="host")
    return regs


@gpu
@pytest.mark.timeout(60)
def test_regheap_partial_wave():
    """70 trials: one full wave and one with six live lanes."""
    r = mm1_three_ways(70, 100, 21)
    assert r["trials_ok"] == 70, r["first_bad_status"]


@gpu
@pytest.mark.timeout(60)
def test_regheap_uncapped_registers():
    """The same kernel without the 168-VGPR cap (MINW = 1)."""
    r = mm1_three_ways(70, 100, 21, CIMBA_LDS_MINW=1)
    assert r["trials_ok"] == 70, r["first_bad_status"]


@gpu
@pytest.mark.timeout(60)
def test_regheap_refill_rounds():
    """One 64-lane workgroup for 200 trials: four wave-synchronous refills,
    the last with eight live lanes; the registers of a lane carry over from
    one trial to the next and reset() must make them dead."""
    r = mm1_three_ways(200, 60, 22, CIMBA_CONV_BLOCKS=1)
    assert r["trials_ok"] == 200, r["first_bad_status"]


@gpu
@pytest.mark.timeout(60)
def test_regheap_until_cuts_lanes_apart():
    """300 objects take about 333 time units; at until = 165 each lane's
    next event passes the limit at an iteration of its own."""
    r = mm1_three_ways(64, 300, 23, until=165.0)
    assert r["trials_ok"] == 64, r["first_bad_status"]
    assert 64 * 50 < r["total_objects"] < 64 * 250


@gpu
@pytest.mark.timeout(60)
def test_regheap_event_limit():
    """100 objects are about 200 events, so a limit of 300 is passed on and
    never reached; 200 objects are about 400, and every trial stops at its
    300th event with ST_EVENT_LIMIT."""
    r = mm1_three_ways(64, 100, 24, max_events=300)
    assert r["trials_ok"] == 64 and r["total_events"] < 64 * 300
    r = mm1_three_ways(64, 200, 24, max_events=300)
    assert r["trials_ok"] == 0 and r["first_bad_status"] == ST_EVENT_LIMIT
    assert r["total_events"] == 64 * 300


@gpu
@pytest.mark.timeout(60)
def test_regheap_mg1():
    kw = dict(ntrials=70, num_objects=100, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=25)
    host = ca.mg1_host(threads=1, **kw)
    with env(CIMBA_MG1_LANE=5):
        fused = ca.mg1_gpu(device=0, **kw)
    with env(CIMBA_MG1_LANE=6):
        regs = ca.mg1_gpu(device=0, **kw)
    assert regs["trials_ok"] == 70, regs["first_bad_status"]
    assert_same(regs, fused, MG1_KEYS, what="mode 5")
    assert_same(regs, host, MG1_KEYS, what="host")


@gpu
@pytest.mark.timeout(60)
def test_regheap_mm1rec():
    """MM1Rec: the cold statistics records under the new flavour."""
    kw = dict(ntrials=64, num_objects=100, seed=26)
    fused = ca._C.mm1rec_gpu(device=0, lane_mode=5, **kw)
    regs = ca._C.mm1rec_gpu(device=0, lane_mode=6, **kw)
    assert regs["trials_ok"] == 64
    assert_same(regs, fused, what="mm1rec")


@gpu
@pytest.mark.timeout(60)
def test_regheap_mm1hot1():
    """MM1Hot1: R = 1, the second pending event is in the cold tier, so
    every push and pop moves an entry between the register and scratch."""
    kw = dict(ntrials=64, num_objects=100, seed=27)
    with env(CIMBA_MM1_LANE=5):
        fused = ca._C.mm1hot1_gpu(device=0, **kw)
    with env(CIMBA_MM1_LANE=6):
        regs = ca._C.mm1hot1_gpu(device=0, **kw)
    assert regs["trials_ok"] == 64
    assert_same(regs, fused, what="mm1hot1")
    assert_same(regs, ca.mm1_host(threads=1, **kw), what="host")
