"""The register window over the first W entries of the object queues
(engine.hpp QWindowState), the generalisation of the one-entry front that
tests/test_queue_front.py covers.

A windowed engine flavour keeps logical positions below W in registers:
a put there issues no ring store, a get hands out position 0, shifts the
window and loads the entry that enters at position W-1.  No result may
depend on W: every windowed flavour must equal the flavour that reads the
ring at the get, bit for bit.

CPU: a seeded put/get/re-init fuzz on an 8-slot ring with an 8-slot spill
segment against a collections.deque, at W = 0, 2, 4 and 7 (the widest an
8-slot ring permits; a request for more is clamped to it); M/M/1 and
M/G/1 through windowed host flavours against the default one at a long
queue, at a short one, and time-limited, where every trial ends with
objects queued and the worker's next trial starts over live stale
registers.
GPU: the LDS kernel (mode 4, windowed) against the all-scratch converged
kernel (mode 3, no window) at a partial wave with a short queue and at
four trials per lane with long excursions past W.
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
QCAP, SPILL_Q = 8, 8
MAX_W = QCAP - 1
ST_QUEUE_FULL = 2
CASES = ("win_put", "ring_put", "tail_load", "short_get", "tail_wrap",
         "refill_out", "drain_put", "queue_full", "reinit_win", "reinit_ring")


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
    """The op sequence of include/cimba/queuewinfuzz.hpp on a deque."""
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
        if (r >> 8) % 251 == 0 and q:
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
def test_queue_window_fuzz(seed):
    nops = 20000
    gets, lens, status = deque_model(seed, nops)
    assert max(lens) == QCAP + SPILL_Q and min(lens) == 0
    for w in (0, 2, 4, MAX_W, 64):
        eff = min(w, MAX_W)  # a wider request is clamped to QCAP - 1
        r = ca._C.queue_window_fuzz(seed, nops, w, eff)
        assert r["window"] == eff, w
        assert list(r["gets"]) == gets, w
        assert list(r["lens"]) == lens, w
        assert r["status"] == status, w
        if w == 0:
            continue
        # the sequence reached every case a window of this width has to
        # survive, and the counts are the sequence's own: the plain
        # flavour, asked for the same width, reports the same ones
        plain = ca._C.queue_window_fuzz(seed, nops, 0, eff)
        for case in CASES:
            assert r[case] >= 1, (w, case)
            assert r[case] == plain[case], (w, case)


# M/G/1 caps its window (MG1::Cfg::QWIN_MAX = 4), so for it 8 and 16 run
# the capped width, the one its LDS kernel uses
WINDOWS = (2, 8, 16)


def host_parity(fn, keys, **kw):
    ref = fn(**kw)
    for w in WINDOWS:
        assert_same(fn(queue_window=w, **kw), ref, keys, what=w)
    return ref


@pytest.mark.parametrize("arr_rate", [0.9, 0.3])
def test_host_parity(arr_rate):
    """rho 0.9: the queue crosses every W constantly.  rho 0.3: it rarely
    leaves the window and drains often."""
    kw = dict(ntrials=64, num_objects=2000, seed=7, threads=1)
    r = host_parity(ca.mm1_host, KEYS, arr_rate=arr_rate, **kw)
    assert r["trials_ok"] == 64
    r = host_parity(ca.mg1_host, MG1_KEYS, arr_rate=arr_rate, srv_mean=1.0,
                    srv_scv=0.25, dist=3, **kw)
    assert r["trials_ok"] == 64


def test_host_parity_time_limited():
    """Arrivals at twice the service rate, stopped at t = 500: about 500
    objects are queued when a trial ends, and the one worker's next trial
    starts on the same engine over a full window of stale registers."""
    r = host_parity(ca.mm1_host, KEYS, ntrials=64, num_objects=2000,
                    arr_rate=2.0, seed=5, threads=1, until=500.0)
    assert 300 * 64 < r["total_objects"] < 700 * 64


def test_host_window_argument_checked():
    with pytest.raises(ValueError):
        ca.mm1_host(ntrials=1, num_objects=10, queue_window=3)
    with pytest.raises(ValueError):
        ca.mm1_host(ntrials=1, num_objects=10, front_cache=True,
                    queue_window=8)


# ---- GPU -----------------------------------------------------------------

gpu = pytest.mark.gpu


def mm1(mode, ntrials, objs, seed, **kw):
    extra = {k: kw.pop(k) for k in list(kw) if k.startswith("CIMBA_")}
    with env(CIMBA_MM1_LANE=mode, **extra):
        r = ca.mm1_gpu(ntrials=ntrials, num_objects=objs, seed=seed, device=0,
                       **kw)
    assert r["trials_ok"] == ntrials, (mode, r["first_bad_status"])
    return r


@gpu
def test_partial_wave_short_queue():
    """200 trials at rho 0.3: three full waves plus one with 8 live
    lanes, on a queue that seldom leaves the window."""
    lds = mm1(4, 200, 2000, 21, arr_rate=0.3)
    assert_same(lds, mm1(3, 200, 2000, 21, arr_rate=0.3))


@gpu
def test_refill_long_queue():
    """8 workgroups of 64 lanes for 2048 trials at rho 0.97: four trials
    per lane, long excursions past W in both directions, and a stale
    window at every refill of a lane."""
    lds = mm1(4, 2048, 2000, 99, arr_rate=0.97, CIMBA_CONV_BLOCKS=8)
    assert_same(lds, mm1(3, 2048, 2000, 99, arr_rate=0.97))
