"""The time-weighted statistics records and the queue spill cursors live
outside the hot toolkit headers (engine.hpp WtdRec, QSpillCursors).

CPU: the LDS plan that the move buys, and statistics equal to what the
engine computed with the records still inside the headers (values
recorded from that engine under tests/golden/).
GPU: MM1Rec records on the LDS kernel, whose statistics record sits in
scratch; the LDS kernel, the all-scratch conv kernel and the host engine
must agree.  Spill models keep their cursors in the hot header.
"""
import json
import os
import subprocess
from contextlib import contextmanager

import pytest

import cimba_amd as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
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


@pytest.fixture(scope="module")
def host_golden():
    with open(os.path.join(GOLDEN, "hot_shrink_host.json")) as f:
        return json.load(f)


# ---- CPU -----------------------------------------------------------------

def test_lds_layout_mm1():
    p = ca._C.lds_layout("mm1")
    assert p["hot_bytes"] <= 312
    assert p["lane_stride"] == 312
    assert p["waves_per_cu"] == 8
    # eight one-wave workgroups fit the CU's 160 KiB of LDS
    assert 8 * 64 * p["lane_stride"] <= 160 * 1024


def test_lds_layout_mg1():
    p = ca._C.lds_layout("mg1")
    assert p["hot_bytes"] <= p["lane_stride"]
    assert p["lane_stride"] % 8 == 0 and (p["lane_stride"] // 8) % 2 == 1
    assert p["waves_per_cu"] == 160 * 1024 // (64 * p["lane_stride"])
    assert p["waves_per_cu"] >= 5
    # the shipped plan
    assert (p["hot_bytes"], p["lane_stride"], p["waves_per_cu"]) == MG1_PLAN


MG1_PLAN = (368, 376, 6)


def test_lds_layout_rejects_other_models():
    with pytest.raises(ValueError):
        ca._C.lds_layout("jobshop")


@pytest.mark.parametrize("seed", [1, 2, 0xDEADBEEF])
def test_recording_model_host_matches_golden(host_golden, seed):
    """Time-weighted mean queue length per trial, bit for bit what the
    engine gave while the record was part of the queue header."""
    g = host_golden
    r = ca._C.mm1rec_host(ntrials=g["ntrials"], num_objects=g["num_objects"],
                          seed=seed)
    assert r["trials_ok"] == g["ntrials"]
    want = [float.fromhex(x) for x in g["mm1rec_mean_qlen"][str(seed)]]
    assert r["per_trial_avg"] == want
    # rho = 0.9: L_q = rho^2 / (1 - rho) = 8.1; short trials, loose sanity
    assert all(1.0 < x < 40.0 for x in want)


@pytest.mark.parametrize("seed", [1, 2, 0xDEADBEEF])
def test_mm1_host_unchanged(host_golden, seed):
    g = host_golden
    r = ca.mm1_host(ntrials=g["ntrials"], num_objects=g["num_objects"],
                    seed=seed, threads=1)
    want = [float.fromhex(x) for x in g["mm1_avg_system_time"][str(seed)]]
    assert r["per_trial_avg"] == want


def test_recording_does_not_change_the_trial():
    """Recording observes; the event sequence is MM1's."""
    a = ca._C.mm1rec_host(ntrials=8, num_objects=2000, seed=5)
    b = ca.mm1_host(ntrials=8, num_objects=2000, seed=5, threads=1)
    assert a["total_events"] == b["total_events"]


def test_capi_all_four_kinds_recording(tmp_path):
    """Queue, resource, pool and buffer statistics of one seeded C-API
    trial (tests/capi_recording.c), printed as hex floats: the recorded
    output of the engine that kept the records in the headers."""
    import cimba_amd  # noqa: F401  (builds libcimba.so)

    libdir = os.path.join(ROOT, "cimba_amd")
    assert os.path.exists(os.path.join(libdir, "libcimba.so"))
    exe = str(tmp_path / "capi_recording")
    r = subprocess.run(
        ["gcc", "-std=c11", "-O2", "-Wall", "-Werror",
         "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "capi_recording.c"),
         "-L", libdir, "-lcimba", f"-Wl,-rpath,{libdir}", "-lm", "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    with open(os.path.join(GOLDEN, "hot_shrink_capi_recording.txt")) as f:
        want = f.read()
    assert out.stdout == want
    for kind in ("queue", "resource", "pool", "buffer"):
        assert f"\n{kind} " in out.stdout


# ---- GPU -----------------------------------------------------------------

gpu = pytest.mark.gpu


def rec(mode, ntrials, objs, seed, **extra):
    with env(**extra):
        r = ca._C.mm1rec_gpu(ntrials=ntrials, num_objects=objs, seed=seed,
                             device=0, lane_mode=mode)
    assert r["trials_ok"] == ntrials, (mode, r["first_bad_status"])
    return r


def assert_matches_host(g, ntrials, objs, seed):
    """The equality of tests/test_gpu.py's M/M/1 host comparison: host
    libm and device OCML draws differ only at rare ulp boundaries, after
    which that trial diverges; most trials are bitwise equal and the
    divergent ones are counted."""
    h = ca._C.mm1rec_host(ntrials=ntrials, num_objects=objs, seed=seed,
                          threads=0)
    assert h["trials_ok"] == ntrials
    gp, hp = g["per_trial_avg"], h["per_trial_avg"]
    assert len(gp) == len(hp) == ntrials
    divergent = sum(1 for a, b in zip(gp, hp) if a != b)
    print(f"divergent {divergent}/{ntrials}")
    assert divergent <= ntrials // 4, f"{divergent}/{ntrials} trials diverged"
    rel_ev = abs(g["total_events"] - h["total_events"]) / h["total_events"]
    assert rel_ev < 0.01


@gpu
def test_recording_partial_wave():
    """200 trials: three full waves plus one with 8 live lanes."""
    lds = rec(4, 200, 2000, 21)
    assert_same(lds, rec(3, 200, 2000, 21))
    assert all(x > 0.0 for x in lds["per_trial_avg"])
    assert_matches_host(lds, 200, 2000, 21)


@gpu
def test_recording_refill_rebuilds_cold_statistics():
    """8 workgroups of 64 lanes for 2048 trials: four refills per lane,
    and init() must reset the statistics record in scratch each time."""
    lds = rec(4, 2048, 2000, 99, CIMBA_CONV_BLOCKS=8)
    assert_same(lds, rec(3, 2048, 2000, 99))
    assert_matches_host(lds, 2048, 2000, 99)


def mm1(mode, ntrials, objs, seed, **extra):
    with env(CIMBA_MM1_LANE=mode, **extra):
        r = ca.mm1_gpu(ntrials=ntrials, num_objects=objs, seed=seed, device=0)
    assert r["trials_ok"] == ntrials, (mode, r["first_bad_status"])
    return r


@gpu
def test_mm1_lds_matches_scratch_kernels():
    lds = mm1(4, 200, 2000, 21)
    for mode in (2, 3):
        assert_same(lds, mm1(mode, 200, 2000, 21), what=mode)
    lds = mm1(4, 2048, 2000, 99, CIMBA_CONV_BLOCKS=8)
    for mode in (2, 3):
        assert_same(lds, mm1(mode, 2048, 2000, 99), what=mode)


MG1_KEYS = ("per_trial_avg", "total_events", "trials_ok", "avg_system_time",
            "avg_queue_time")


def mg1(mode, **kw):
    with env(CIMBA_MG1_LANE=mode):
        r = ca.mg1_gpu(device=0, **kw)
    assert r["trials_ok"] == kw["ntrials"], (mode, r["first_bad_status"])
    return r


@gpu
def test_mg1_lds_matches_conv():
    kw = dict(ntrials=1024, num_objects=2000, arr_rate=0.8, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=7)
    assert_same(mg1(4, **kw), mg1(3, **kw), MG1_KEYS)


@gpu
def test_mg1_queue_spill_on_lds_kernel():
    """Arrivals at twice the service rate: after 3000 objects about 1500
    wait, past the 1024-slot ring, so every trial runs the queue's spill
    segment, whose cursors stay in the hot header of a SPILL_Q model."""
    kw = dict(ntrials=128, num_objects=3000, arr_rate=2.0, srv_mean=1.0,
              srv_scv=0.25, dist=3, seed=11)
    lds = mg1(4, **kw)
    assert_same(lds, mg1(3, **kw), MG1_KEYS)
    # mean wait in queue of an overloaded run: ~ 3000 / 2 / 2 time units
    assert lds["avg_queue_time"] > 300.0
