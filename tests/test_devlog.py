"""Device log stream (include/cimba/devlog.hpp): in-trial log records from
the logged M/M/1 model, on the host engine and through every GPU kernel
shape.  The host engine is the reference for the GPU cases: records and
emission counts must come back bit for bit."""
import functools

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C, devlog

ARRIVE, START, DEPART = 1, 2, 3
USER_START = 1 << 4
TOTALS = ("total_events", "total_wait", "total_objects", "per_trial_avg")
BASE = dict(num_objects=200, arr_rate=0.9, srv_rate=1.0, seed=7)
TINY = dict(BASE, ntrials=1, num_objects=3, log_count=1, threads=1)
ABORT = dict(arr_rate=4.0, srv_rate=1.0, num_objects=4000, seed=7,
             log_capacity=8)
GPU = dict(num_objects=20, arr_rate=0.9, srv_rate=1.0, seed=7)
KERNELS = ("wave", "lane", "scratch", "conv")


def same_records(a, b):
    """Bit-for-bit equality, field by field (NaN-safe, padding-blind)."""
    return (a.dtype == b.dtype and a.shape == b.shape and
            all(a[n].tobytes() == b[n].tobytes() for n in a.dtype.names))


@functools.lru_cache(maxsize=None)
def host_ref(**kw):
    """mm1log_host results, computed once per argument set and shared."""
    r = ca.mm1log_host(threads=1, **kw)
    r["log_records"].setflags(write=False)
    r["log_emitted"].setflags(write=False)
    return r


def host_ref_for(kw):
    return host_ref(**{k: v for k, v in kw.items()
                       if k not in ("kernel", "blocks", "device")})


# ---- CPU ------------------------------------------------------------------

def test_no_perturbation():
    plain = ca.mm1_host(ntrials=16, threads=1, **BASE)
    for log in (dict(log_count=0), dict(log_count=16),
                dict(log_count=16, log_capacity=1)):
        r = ca.mm1log_host(ntrials=16, threads=1, **BASE, **log)
        for k in TOTALS:
            assert r[k] == plain[k], (log, k)


def test_hand_checkable_content():
    r = ca.mm1log_host(log_capacity=64, **TINY)
    rec = r["log_records"]
    assert len(rec) == 9
    assert list(r["log_emitted"]) == [9]
    assert list(rec["seq"]) == list(range(9))
    assert np.all(np.diff(rec["t"]) >= 0)
    for code in (ARRIVE, START, DEPART):
        assert np.count_nonzero(rec["code"] == code) == 3
    arrive = rec[rec["code"] == ARRIVE]
    assert list(arrive["value"]) == [0, 1, 2]
    assert np.all(arrive["proc"] == 0)
    assert np.all(rec[rec["code"] != ARRIVE]["proc"] == 1)
    assert np.all(arrive["flags"] == _C.LOG_INFO)
    assert np.all(rec[rec["code"] == START]["flags"] == USER_START)
    # the depart payload is the exact term the model adds to its sum
    total = np.float64(0.0)
    for bits in rec[rec["code"] == DEPART]["value"]:
        total += np.uint64(bits).view(np.float64)
    assert float(total).hex() == float(r["total_wait"]).hex()


def test_ring_keeps_last_records():
    full = ca.mm1log_host(log_capacity=64, **TINY)
    r = ca.mm1log_host(log_capacity=4, **TINY)
    assert list(r["log_emitted"]) == [9]
    assert len(r["log_records"]) == 4
    assert same_records(r["log_records"], full["log_records"][-4:])


def test_mask():
    r = ca.mm1log_host(log_capacity=64, log_mask=USER_START, **TINY)
    rec = r["log_records"]
    assert list(r["log_emitted"]) == [3]
    assert list(rec["code"]) == [START] * 3
    assert list(rec["seq"]) == [0, 1, 2]


def test_window_and_world_size_invariance():
    a = ca.mm1log_host(ntrials=10, threads=1, log_first=5, log_count=3, **BASE)
    b = ca.mm1log_host(ntrials=3, trial_base=5, threads=1, log_first=5,
                       log_count=3, **BASE)
    assert len(a["log_records"]) > 0
    assert set(a["log_records"]["trial"]) == {5, 6, 7}
    assert same_records(a["log_records"], b["log_records"])
    assert np.array_equal(a["log_emitted"], b["log_emitted"])
    assert a["log_first"] == b["log_first"] == 5
    c = ca.mm1log_host(ntrials=10, threads=1, log_first=8, log_count=10,
                       **BASE)
    assert c["log_first"] == 8 and len(c["log_emitted"]) == 2
    assert set(c["log_records"]["trial"]) == {8, 9}


def test_abort_line():
    r = ca.mm1log_host(ntrials=1, threads=1, log_count=1, **ABORT)
    assert r["first_bad_status"] == 2  # ST_QUEUE_FULL
    rec = r["log_records"]
    assert len(rec) == 8 and r["log_emitted"][0] > 8
    last, prev = rec[-1], rec[-2]
    assert last["flags"] == _C.LOG_ERROR
    assert last["code"] == 2 and last["proc"] == -1
    assert last["vtype"] == 1 and last["value"] == 2
    assert last["t"] >= prev["t"]


def test_formatter_and_replay(capfd):
    r = ca.mm1log_host(log_capacity=64, **TINY)
    rec = r["log_records"]
    lines = devlog.format_lines(r, name="mm1log", seed=TINY["seed"])
    assert len(lines) == 9
    names = {ARRIVE: "arrive", START: "start", DEPART: "depart"}
    for x, line in zip(rec, lines):
        if x["vtype"] == 2:
            val = "%.17g" % np.uint64(x["value"]).view(np.float64)
        else:
            val = "%d" % x["value"]
        tag = "info" if x["flags"] == _C.LOG_INFO else "user"
        want = "[%d] [%016x] %.6f proc%d %s: %s value=%s" % (
            x["trial"], ca.trial_seed(TINY["seed"], int(x["trial"])), x["t"],
            x["proc"], tag, names[int(x["code"])], val)
        assert line == want
    # the abort record: engine context, signed value, status name
    ab = ca.mm1log_host(ntrials=1, threads=1, log_count=1, **ABORT)
    x = ab["log_records"][-1]
    assert devlog.format_lines(ab, name="mm1log", seed=7)[-1] == (
        "[0] [%016x] %.6f engine error: queue_full value=2"
        % (ca.trial_seed(7, 0), x["t"]))

    # replay goes through the host logger's gate: INFO masked off, the
    # user bit on -> only the three `start` lines print
    saved = _C.logger_flags()
    capfd.readouterr()
    try:
        _C.logger_flags_off(_C.LOG_INFO)
        _C.logger_flags_on(USER_START)
        walked = devlog.replay(r, name="mm1log", seed=TINY["seed"])
    finally:
        _C.logger_flags_off(0xFFFFFFFF)
        _C.logger_flags_on(saved)
    err = capfd.readouterr().err.splitlines()
    assert walked == 9
    assert not [ln for ln in err if " info: " in ln]
    assert err == [ln for ln in lines if " user: " in ln] and len(err) == 3


def test_guards():
    big = dict(log_count=2**20, log_capacity=64)  # 2 GiB of records
    with pytest.raises(ValueError):
        ca.mm1log_host(ntrials=1, num_objects=3, **big)
    # raised before any device call, so this needs no GPU
    with pytest.raises(ValueError):
        ca.mm1log_gpu(ntrials=1, num_objects=3, **big)
    with pytest.raises(ValueError):
        ca.mm1log_gpu(ntrials=1, num_objects=3, kernel="warp")
    # exactly 1 GiB as requested is allowed (and clips to the one trial run)
    ok = ca.mm1log_host(ntrials=1, num_objects=3, threads=1,
                        log_count=2**19, log_capacity=64)
    assert len(ok["log_emitted"]) == 1


def test_registry():
    from cimba_amd.models import run

    r = run("mm1log", backend="cpu", ntrials=2, num_objects=50, seed=4,
            threads=1, log_count=2)
    assert r["trials_ok"] == 2 and len(r["log_emitted"]) == 2


# ---- GPU ------------------------------------------------------------------

def check_against_host(kw):
    g = ca.mm1log_gpu(**kw)
    h = host_ref_for(kw)
    assert g["log_first"] == h["log_first"]
    assert np.array_equal(g["log_emitted"], h["log_emitted"])
    assert g["log_emitted"].tobytes() == h["log_emitted"].tobytes()
    assert same_records(g["log_records"], h["log_records"])
    return g, h


def check_totals_match_mm1_gpu(g, ntrials, **model):
    plain = ca.mm1_gpu(ntrials=ntrials, **model)
    for k in TOTALS:
        assert g[k] == plain[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_partial_last_wave_or_block(kernel):
    kw = dict(GPU, ntrials=257, log_count=257, log_capacity=64, kernel=kernel)
    g, _ = check_against_host(kw)
    assert len(g["log_emitted"]) == 257 and np.all(g["log_emitted"] == 60)
    check_totals_match_mm1_gpu(g, 257, **GPU)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_stride_loop_reuse(kernel):
    kw = dict(GPU, ntrials=300, blocks=1, log_first=250, log_count=20,
              log_capacity=64, kernel=kernel)
    g, _ = check_against_host(kw)
    assert set(g["log_records"]["trial"]) == set(range(250, 270))
    check_totals_match_mm1_gpu(g, 300, **GPU)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_overflow(kernel):
    kw = dict(GPU, ntrials=257, log_count=257, log_capacity=4, kernel=kernel)
    g, _ = check_against_host(kw)
    assert len(g["log_records"]) == 257 * 4
    check_totals_match_mm1_gpu(g, 257, **GPU)


@pytest.mark.gpu
def test_gpu_abort_line():
    kw = dict(ABORT, ntrials=65, log_count=65, kernel="conv")
    g = ca.mm1log_gpu(**kw)
    h = host_ref_for(kw)
    assert g["first_bad_status"] == 2 and g["trials_ok"] == 0
    assert np.array_equal(g["log_emitted"], h["log_emitted"])
    grec, hrec = g["log_records"], h["log_records"]
    for trial in range(65):
        gl = grec[grec["trial"] == trial][-1:]
        hl = hrec[hrec["trial"] == trial][-1:]
        assert len(gl) == 1 and gl["flags"][0] == _C.LOG_ERROR
        assert gl["proc"][0] == -1 and gl["code"][0] == 2
        assert same_records(gl, hl), trial


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_empty_window(kernel):
    g = ca.mm1log_gpu(ntrials=257, log_count=0, kernel=kernel, **GPU)
    assert len(g["log_records"]) == 0 and len(g["log_emitted"]) == 0
    check_totals_match_mm1_gpu(g, 257, **GPU)
