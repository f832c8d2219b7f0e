"""The register-only sifts of the event heap (hashheap.hpp reg_push and the
short pop): a push into a heap of n < R entries and a pop from one of
n <= R work on the register tier alone, at constant indices, in front of
the generic sift_up / sift_down.  They must leave the heap array what the
generic code leaves, entry for entry, so no result may differ in any bit.

CPU: M/M/1 and M/G/1 on the host flavour with the register tier
(heap_regs=True, FlatRegTier, R = 2) against the plain one.  Both models
hold two events at most, so every push and pop of these runs takes the
short paths and none crosses the R boundary.  No host binding reaches a
flavour that holds more than R events under a register tier, so the
crossing in both directions (short path, generic sift, short path again in
one sequence), at R = 1, 2, 3 and 5 with and without a spill tier, is
covered by the shallow phase of the stand-alone lockstep fuzzer
csrc/host/heapregfuzz_main.cpp, built with address and undefined-behaviour
sanitizers.  Ties are left to that fuzzer as well: event times that tie
cannot be constructed through the model bindings, and the fuzzer draws its
keys from two values each.

GPU: lane mode 6 against mode 5 and the host engine at the smallest shapes
where a wrong register move shows: a partial wave, wave-synchronous refills
(rg[] carries over from one trial to the next), an `until` that ends the
lanes apart, the event limit, the uncapped kernel, M/G/1, and MM1Hot1,
whose R = 1 makes every second push and pop leave the short path at once.
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

@pytest.mark.parametrize("seed", SEEDS)
def test_host_reg_sifts_mm1(seed):
    """Run to the end, cut by `until` in mid-trial (200 objects at rate 0.9
    take about 220 time units), and stopped by the event limit."""
    for kw in (dict(), dict(until=110.0), dict(max_events=300)):
        kw = dict(ntrials=8, num_objects=200, seed=seed, threads=1, **kw)
        ref = ca.mm1_host(**kw)
        assert_same(ca.mm1_host(heap_regs=True, **kw), ref, what=kw)
        if "max_events" in kw:
            assert ref["first_bad_status"] == ST_EVENT_LIMIT
            assert ref["total_events"] == 8 * 300
        else:
            assert ref["trials_ok"] == 8


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dist", [0, 3])
def test_host_reg_sifts_mg1(seed, dist):
    for kw in (dict(), dict(until=110.0), dict(max_events=300)):
        kw = dict(ntrials=8, num_objects=200, arr_rate=0.8, srv_mean=1.0,
                  srv_scv=0.25, dist=dist, seed=seed, threads=1, **kw)
        ref = ca.mg1_host(**kw)
        assert_same(ca.mg1_host(heap_regs=True, **kw), ref, MG1_KEYS, what=kw)
        if "max_events" in kw:
            assert ref["first_bad_status"] == ST_EVENT_LIMIT
        else:
            assert ref["trials_ok"] == 8


def test_reg_sifts_keep_the_lds_plans():
    """The short paths add nothing to Hot: strides and waves per CU of
    mode 6 are what they were."""
    lay = ca._C.lds_layout("mm1_regheap")
    assert (lay["lane_stride"], lay["waves_per_cu"]) == (232, 11)
    lay = ca._C.lds_layout("mg1_regheap")
    assert (lay["lane_stride"], lay["waves_per_cu"]) == (296, 8)


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
def test_reg_sifts_partial_wave():
    """70 trials: one full wave and one with six live lanes."""
    r = mm1_three_ways(70, 100, 31)
    assert r["trials_ok"] == 70, r["first_bad_status"]


@gpu
@pytest.mark.timeout(60)
def test_reg_sifts_uncapped_registers():
    """The kernel without the 168-VGPR cap (MINW = 1)."""
    r = mm1_three_ways(70, 100, 31, CIMBA_LDS_MINW=1)
    assert r["trials_ok"] == 70, r["first_bad_status"]


@gpu
@pytest.mark.timeout(60)
def test_reg_sifts_refill_rounds():
    """One 64-lane workgroup for 200 trials: four refills, the last with
    eight live lanes.  A lane's rg[] carries over from its last trial, and
    the short pop leaves a dead copy in rg[0]: reset() must make both dead."""
    r = mm1_three_ways(200, 60, 32, CIMBA_CONV_BLOCKS=1)
    assert r["trials_ok"] == 200, r["first_bad_status"]


@gpu
@pytest.mark.timeout(60)
def test_reg_sifts_until_cuts_lanes_apart():
    """300 objects take about 333 time units; at until = 165 each lane's
    next event passes the limit at an iteration of its own, with one or two
    events left in the registers."""
    r = mm1_three_ways(64, 300, 33, until=165.0)
    assert r["trials_ok"] == 64, r["first_bad_status"]
    assert 64 * 50 < r["total_objects"] < 64 * 250


@gpu
@pytest.mark.timeout(60)
def test_reg_sifts_event_limit():
    """200 objects are about 400 events: every trial stops at its 300th
    with ST_EVENT_LIMIT."""
    r = mm1_three_ways(64, 200, 34, max_events=300)
    assert r["trials_ok"] == 0 and r["first_bad_status"] == ST_EVENT_LIMIT
    assert r["total_events"] == 64 * 300


@gpu
@pytest.mark.timeout(60)
def test_reg_sifts_mg1():
    kw = dict(ntrials=70, num_objects=100, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=35)
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
def test_reg_sifts_mm1hot1():
    """MM1Hot1: R = 1.  The first pending event is pushed and popped by the
    short paths, the second lives in scratch and goes the generic way, so
    the kernel changes path on every second heap operation."""
    kw = dict(ntrials=64, num_objects=100, seed=37)
    with env(CIMBA_MM1_LANE=5):
        fused = ca._C.mm1hot1_gpu(device=0, **kw)
    with env(CIMBA_MM1_LANE=6):
        regs = ca._C.mm1hot1_gpu(device=0, **kw)
    assert regs["trials_ok"] == 64
    assert_same(regs, fused, what="mm1hot1")
    assert_same(regs, ca.mm1_host(threads=1, **kw), what="host")
