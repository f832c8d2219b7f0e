"""The register-resident front of the object queues (engine.hpp qfront).

The LDS kernel's engine flavour hands a get the front it loaded at the
previous get, and loads the next one.  No result may depend on that: the
cached flavours must equal the flavours that read the ring at the get,
bit for bit.

CPU: a seeded put/get/re-init fuzz on a 4-slot ring with an 8-slot spill
segment against a collections.deque; M/M/1 and M/G/1 through the cached
host flavour (FlatFrontTier) against the default one, also time-limited,
where every trial ends with objects queued and the worker's next trial
starts with a live stale front.
GPU: the LDS kernel (mode 4, cached) against the all-scratch kernels
(modes 3 and 2, no cache) at a partial wave, at four refills per lane,
time-limited, on the spill path, and for the boundary models.
"""
import collections
import os
from contextlib import contextmanager

import pytest

import cimba_amd as ca

KEYS = ("per_trial_avg", "total_wait", "total_events", "trials_ok",
        "first_bad_status")
MG1_KEYS = ("per_trial_avg", "total_events", "trials_ok", "avg_system_time",
            "avg_queue_time", "first_bad_status")
MASK = (1 << 64) - 1
QCAP, SPILL_Q = 4, 8
ST_QUEUE_FULL = 2


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

def deque_model(seed, nops):
    """The op sequence of include/cimba/queuefuzz.hpp on a deque."""
    x = seed

    def rnd():
        nonlocal x
        x = (x + 0x9E3779B97F4A7C15) & MASK
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    q = collections.deque()
    gets, lens, status = [], [], 0
    for op in range(nops):
        r = rnd()
        nput = 5 if (op >> 6) & 1 else 11
        what = r % 16
        if (r >> 8) % 997 == 0 and q:
            q.clear()  # the next trial: init() abandons what is queued
            status = 0
        elif what < nput:
            if len(q) >= QCAP + SPILL_Q:
                if status == 0:
                    status = ST_QUEUE_FULL
            else:
                q.append(r | 1)
        elif q:
            gets.append(q.popleft())
        lens.append(len(q))
    return gets, lens, status


@pytest.mark.parametrize("seed", [1, 2, 0xDEADBEEF])
def test_queue_fuzz(seed):
    nops = 20000
    cached = ca._C.queue_front_fuzz(seed, nops, True)
    plain = ca._C.queue_front_fuzz(seed, nops, False)
    gets, lens, status = deque_model(seed, nops)
    for r in (cached, plain):
        assert list(r["gets"]) == gets
        assert list(r["lens"]) == lens
        assert r["status"] == status
    # the sequence reached every case the cache has to survive
    for case in ("wraps", "ring_full", "refill_front", "drain_put",
                 "queue_full", "reinits"):
        assert cached[case] >= 1, case
        assert cached[case] == plain[case], case
    assert max(lens) == QCAP + SPILL_Q


@pytest.mark.parametrize("seed", [1, 2, 0xDEADBEEF])
def test_host_parity_unbounded(seed):
    kw = dict(ntrials=64, num_objects=2000, seed=seed, threads=1)
    a = ca.mm1_host(front_cache=True, **kw)
    b = ca.mm1_host(**kw)
    assert a["trials_ok"] == 64
    assert_same(a, b, what="mm1")
    kw.update(arr_rate=0.8, srv_mean=1.0, srv_scv=0.25, dist=3)
    a = ca.mg1_host(front_cache=True, **kw)
    b = ca.mg1_host(**kw)
    assert a["trials_ok"] == 64
    assert_same(a, b, MG1_KEYS, what="mg1")


def test_host_parity_time_limited():
    """Arrivals at twice the service rate, stopped at t = 500: about 1000
    arrived, about 500 served, about 500 queued when the trial ends (some
    trials pass the 512-slot ring and abort with ST_QUEUE_FULL, which the
    two flavours must agree on too).  One worker runs all trials on one
    engine, so each trial starts with the previous trial's front."""
    kw = dict(ntrials=64, num_objects=2000, arr_rate=2.0, seed=5, threads=1,
              until=500.0)
    a = ca.mm1_host(front_cache=True, **kw)
    b = ca.mm1_host(**kw)
    assert_same(a, b)
    # the limit really cut the trials short: about 500 of 2000 served
    assert 300 * 64 < a["total_objects"] < 700 * 64


# ---- GPU -----------------------------------------------------------------

gpu = pytest.mark.gpu


def mm1(mode, ntrials, objs, seed, check_ok=True, **kw):
    extra = {k: kw.pop(k) for k in list(kw) if k.startswith("CIMBA_")}
    with env(CIMBA_MM1_LANE=mode, **extra):
        r = ca.mm1_gpu(ntrials=ntrials, num_objects=objs, seed=seed, device=0,
                       **kw)
    if check_ok:
        assert r["trials_ok"] == ntrials, (mode, r["first_bad_status"])
    return r


@gpu
def test_partial_wave():
    """200 trials: three full waves plus one with 8 live lanes."""
    lds = mm1(4, 200, 2000, 21)
    for mode in (3, 2):
        assert_same(lds, mm1(mode, 200, 2000, 21), what=mode)


@gpu
def test_refill():
    """8 workgroups of 64 lanes for 2048 trials: four trials per lane."""
    lds = mm1(4, 2048, 2000, 99, CIMBA_CONV_BLOCKS=8)
    for mode in (3, 2):
        assert_same(lds, mm1(mode, 2048, 2000, 99), what=mode)


@gpu
def test_time_limited_refill():
    """The refill shape, stopped at t = 500 with about 500 objects queued:
    every lane starts its next trial with a live stale front and must not
    see it."""
    kw = dict(arr_rate=2.0, until=500.0, check_ok=False)
    lds = mm1(4, 2048, 2000, 99, CIMBA_CONV_BLOCKS=8, **kw)
    assert_same(lds, mm1(3, 2048, 2000, 99, **kw), what=3)
    assert 300 * 2048 < lds["total_objects"] < 700 * 2048
    # host libm and device OCML draws differ at rare ulp boundaries, after
    # which that trial diverges (tests/test_gpu.py): most trials are
    # bitwise equal and the divergent ones are counted
    h = ca.mm1_host(ntrials=2048, num_objects=2000, arr_rate=2.0, seed=99,
                    until=500.0)
    gp, hp = lds["per_trial_avg"], h["per_trial_avg"]
    assert len(gp) == len(hp) == 2048
    divergent = sum(1 for a, b in zip(gp, hp) if a != b)
    print(f"divergent {divergent}/2048")
    assert divergent <= 2048 // 4, f"{divergent}/2048 trials diverged"
    rel_ev = abs(lds["total_events"] - h["total_events"]) / h["total_events"]
    assert rel_ev < 0.01


@gpu
def test_mg1_spill_every_get_refills():
    """The overloaded shape of test_mg1_queue_spill_on_lds_kernel: past the
    1024-slot ring every get refills the ring from the spill segment."""
    kw = dict(ntrials=128, num_objects=3000, arr_rate=2.0, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=11, device=0)
    with env(CIMBA_MG1_LANE=4):
        lds = ca.mg1_gpu(**kw)
    with env(CIMBA_MG1_LANE=3):
        conv = ca.mg1_gpu(**kw)
    assert lds["trials_ok"] == 128, lds["first_bad_status"]
    assert_same(lds, conv, MG1_KEYS)


@gpu
def test_boundary_models():
    """One hot heap entry, and the recording queue, on the cached kernel."""
    hot1 = ca._C.mm1hot1_gpu(ntrials=256, num_objects=2000, seed=31, device=0)
    assert hot1["trials_ok"] == 256, hot1["first_bad_status"]
    assert_same(hot1, mm1(3, 256, 2000, 31))
    rec4 = ca._C.mm1rec_gpu(ntrials=256, num_objects=2000, seed=31, device=0,
                            lane_mode=4)
    rec3 = ca._C.mm1rec_gpu(ntrials=256, num_objects=2000, seed=31, device=0,
                            lane_mode=3)
    assert rec4["trials_ok"] == 256, rec4["first_bad_status"]
    assert_same(rec4, rec3)
