"""Device tally stream (include/cimba/tally.hpp) on the host engine: the
bin function, exact per-trial histograms and moments of the tallied M/M/1
model, window handling, quantiles and guards.

The oracle is independent of the tally code: mm1log_host with the same
seed runs the same draws and logs every observation (log_capacity >=
3 * num_objects), and the bin function is re-implemented here in numpy
from its specification."""
import functools
import math
import os
import subprocess
import time

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C, tally

NBINS = 770
BASE = dict(num_objects=200, arr_rate=0.9, srv_rate=1.0, seed=7)
NTRIALS = 16
TOTALS = ("total_events", "total_wait", "total_objects", "per_trial_avg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


def bin_oracle(x):
    """Bin index per the specification, -1 for NaN (no bin)."""
    x = np.asarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    mid = (1 + (bits >> np.uint64(48)).astype(np.int64)
           - ((1023 - 24) << 4))
    with np.errstate(invalid="ignore"):
        out = np.where(x >= 2.0 ** 24, NBINS - 1, mid)
        out = np.where(~(x >= 2.0 ** -24), 0, out)
    return np.where(np.isnan(x), -1, out).astype(np.int64)


@functools.lru_cache(maxsize=None)
def oracle_observations():
    """Per trial: (tally-0 observations, tally-1 observations), in order,
    from the logged model's records.  Computed once, never modified."""
    r = ca.mm1log_host(ntrials=NTRIALS, threads=1, log_count=NTRIALS,
                       log_capacity=3 * BASE["num_objects"], **BASE)
    rec = r["log_records"]
    assert np.all(r["log_emitted"] == 3 * BASE["num_objects"])
    obs = []
    for t in range(NTRIALS):
        mine = rec[rec["trial"] == t]
        dep = mine[mine["code"] == 3]
        start = mine[mine["code"] == 2]
        x0 = dep["value"].copy().view(np.float64)
        x1 = start["t"] - start["value"].copy().view(np.float64)
        x0.setflags(write=False)
        x1.setflags(write=False)
        obs.append((x0, x1))
    return tuple(obs)


def summary_fields(ds):
    return dict(zip(("n", "mean", "m2", "m3", "m4", "min", "max"), ds.raw()))


# ---- bin function -----------------------------------------------------------

def test_bin_function_named_values():
    lo, hi = 2.0 ** -24, 2.0 ** 24
    cases = [(0.0, 0), (-0.0, 0), (-1.0, 0), (5e-324, 0),
             (np.nextafter(lo, 0), 0), (lo, 1), (1.0, 385),
             (np.nextafter(2.0, 0), 400), (np.nextafter(hi, 0), 768),
             (hi, 769), (np.inf, 769), (np.nan, -1)]
    x = np.array([c[0] for c in cases])
    want = np.array([c[1] for c in cases])
    assert np.array_equal(_C.tally_bin(x), want)
    assert np.array_equal(bin_oracle(x), want)


def test_bin_function_edges_and_random():
    e = _C.tally_edges()
    assert e.shape == (NBINS + 1,) and e[0] == 0.0 and np.isinf(e[-1])
    assert e[1] == 2.0 ** -24 and e[385] == 1.0 and e[769] == 2.0 ** 24
    assert np.all(np.diff(e) > 0)
    assert np.array_equal(tally.edges(), e)
    lower = e[1:NBINS]
    assert np.array_equal(_C.tally_bin(lower), np.arange(1, NBINS))
    assert np.array_equal(_C.tally_bin(np.nextafter(lower, 0)),
                          np.arange(0, NBINS - 1))
    # relative bin width at most 1/16
    assert np.all(np.diff(e[1:NBINS]) / e[1:NBINS - 1] <= 1.0 / 16)
    rng = np.random.default_rng(11)
    x = 2.0 ** rng.uniform(-30.0, 30.0, 100_000)
    both = np.concatenate([lower, np.nextafter(lower, 0), x])
    assert np.array_equal(_C.tally_bin(both), bin_oracle(both))
    assert len(set(_C.tally_bin(x))) == NBINS  # every bin exercised


# ---- exact host content -------------------------------------------------------

@pytest.mark.parametrize("threads", [1, 4])
def test_exact_host_content(threads):
    obs = oracle_observations()
    r = ca.mm1tally_host(ntrials=NTRIALS, threads=threads,
                         per_trial_hist=True, **BASE)
    plain = ca.mm1_host(ntrials=NTRIALS, threads=1, **BASE)
    th, hist, summ = (r["tally_trial_hist"], r["tally_hist"],
                      r["tally_summaries"])
    assert r["tally_first"] == 0
    assert th.shape == (NTRIALS, 2, NBINS) and th.dtype == np.uint32
    assert hist.shape == (2, NBINS) and hist.dtype == np.uint64
    assert summ.shape == (NTRIALS, 2)
    assert summ.dtype.names == ("n", "mean", "m2", "m3", "m4", "min", "max",
                                "nan")
    assert sum(len(o[0]) for o in obs) == 3200
    assert sum(len(o[1]) for o in obs) == 3200
    for t in range(NTRIALS):
        for k in range(2):
            x = obs[t][k]
            want = np.bincount(bin_oracle(x), minlength=NBINS)
            assert np.array_equal(th[t, k], want), (t, k)
            ds = ca.DataSummary()
            for v in x:
                ds.add(float(v))
            for name, v in summary_fields(ds).items():
                got = summ[t, k][name]
                assert np.float64(v).tobytes() == got.tobytes(), (t, k, name)
            assert summ[t, k]["nan"] == 0
    assert np.array_equal(hist, th.sum(axis=0, dtype=np.uint64))
    # every trial ran to completion, so its obj_cnt is num_objects
    assert r["trials_ok"] == NTRIALS
    assert np.all(summ["n"] == BASE["num_objects"])
    assert summ["n"][:, 0].sum() == r["total_objects"]
    for k in TOTALS:
        assert r[k] == plain[k], k
    assert hist[1, 0] == 500  # arrivals that found the server idle
    used = np.nonzero(hist[0])[0]
    assert used[0] == 265 and used[-1] == 472


def test_no_perturbation():
    plain = ca.mm1_host(ntrials=NTRIALS, threads=1, **BASE)
    for count in (0, None, 3):
        r = ca.mm1tally_host(ntrials=NTRIALS, threads=1, tally_count=count,
                             **BASE)
        for k in TOTALS:
            assert r[k] == plain[k], (count, k)
        assert len(r["tally_summaries"]) == {0: 0, None: NTRIALS, 3: 3}[count]


def test_window_and_world_size_invariance():
    kw = dict(threads=1, per_trial_hist=True, **BASE)
    full = ca.mm1tally_host(ntrials=16, **kw)
    a = ca.mm1tally_host(ntrials=8, trial_base=0, **kw)
    b = ca.mm1tally_host(ntrials=8, trial_base=8, **kw)
    assert (a["tally_first"], b["tally_first"]) == (0, 8)
    for key in ("tally_summaries", "tally_trial_hist"):
        both = np.concatenate([a[key], b[key]])
        assert both.tobytes() == full[key].tobytes(), key
    assert np.array_equal(a["tally_hist"] + b["tally_hist"],
                          full["tally_hist"])
    # a window that sticks out at both ends of the run clips to it
    c = ca.mm1tally_host(ntrials=4, trial_base=6, tally_first=3,
                         tally_count=100, **kw)
    assert c["tally_first"] == 6 and len(c["tally_summaries"]) == 4
    assert c["tally_trial_hist"].tobytes() == \
        full["tally_trial_hist"][6:10].tobytes()
    # an inner window
    d = ca.mm1tally_host(ntrials=16, tally_first=5, tally_count=3, **kw)
    assert d["tally_first"] == 5
    assert d["tally_summaries"].tobytes() == \
        full["tally_summaries"][5:8].tobytes()
    assert np.array_equal(
        d["tally_hist"],
        full["tally_trial_hist"][5:8].sum(axis=0, dtype=np.uint64))
    # no per-trial histogram unless asked for
    assert "tally_trial_hist" not in ca.mm1tally_host(ntrials=2, threads=1,
                                                      **BASE)


# ---- python surface ---------------------------------------------------------

@pytest.mark.parametrize("q", [0.5, 0.9, 0.99])
def test_quantile_within_the_bin_of_the_order_statistic(q):
    x = np.sort(np.concatenate([o[0] for o in oracle_observations()]))
    r = ca.mm1tally_host(ntrials=NTRIALS, threads=1, **BASE)
    exact = x[math.ceil(q * len(x)) - 1]
    b = int(bin_oracle(np.array([exact]))[0])
    e = tally.edges()
    est = tally.quantile(r["tally_hist"][0], q)
    assert e[b] <= est <= e[b + 1], (q, exact, est)


def test_quantile_end_bins_fivenum_and_merge():
    row = np.zeros(NBINS, dtype=np.uint64)
    assert math.isnan(tally.quantile(row, 0.5))
    row[0], row[769] = 6, 4
    assert tally.quantile(row, 0.5) == 0.0
    assert tally.quantile(row, 0.9) == 2.0 ** 24
    with pytest.raises(ValueError):
        tally.quantile(row, 0.0)
    x = np.concatenate([o[0] for o in oracle_observations()])
    r = ca.mm1tally_host(ntrials=NTRIALS, threads=1, **BASE)
    ds = tally.merged_summary(r, 0)
    assert ds.count() == len(x)
    assert ds.minimum() == x.min() and ds.maximum() == x.max()
    assert abs(ds.mean() - x.mean()) <= 1e-12 * x.mean()
    assert abs(ds.variance() - x.var(ddof=1)) <= 1e-10 * x.var(ddof=1)
    five = tally.fivenum(r["tally_hist"][0], ds)
    assert five[0] == x.min() and five[4] == x.max()
    assert list(five) == sorted(five)
    # tally 1: a sixth of the waits are exact zeros, so min == 0
    assert tally.merged_summary(r, 1).minimum() == 0.0


# ---- guards -------------------------------------------------------------------

def test_guards():
    # 200000 trials x 2 tallies x 3144 B > 1 GiB: refused before any
    # allocation, so this returns at once
    t0 = time.perf_counter()
    with pytest.raises(ValueError):
        ca.mm1tally_host(ntrials=200_000, num_objects=1, tally_count=200_000)
    with pytest.raises(ValueError):
        ca.mm1tally_host(ntrials=200_000, num_objects=1)  # None = all
    # raised before any device call, so these need no GPU
    with pytest.raises(ValueError):
        ca.mm1tally_gpu(ntrials=200_000, num_objects=1, tally_count=200_000)
    with pytest.raises(ValueError):
        ca.mm1tally_gpu(ntrials=1, num_objects=3, kernel="warp")
    assert time.perf_counter() - t0 < 5.0
    # the largest window that fits is accepted as requested and clips
    fit = (1 << 30) // 3144 // 2
    ok = ca.mm1tally_host(ntrials=1, num_objects=3, threads=1,
                          tally_count=fit)
    assert len(ok["tally_summaries"]) == 1
    with pytest.raises(ValueError):
        ca.mm1tally_host(ntrials=1, num_objects=3, tally_count=fit + 1)
    with pytest.raises(ValueError):
        _C.tally_reduce_gpu(np.zeros((1, 9, NBINS), dtype=np.uint32))


def test_registry():
    from cimba_amd.models import EXAMPLES, MODELS, run

    assert "mm1tally" in EXAMPLES and "mm1tally" not in MODELS
    r = run("mm1tally", backend="cpu", ntrials=2, num_objects=50, seed=4,
            threads=1)
    assert r["trials_ok"] == 2 and r["tally_summaries"].shape == (2, 2)
    assert r["tally_hist"].sum() == 2 * 2 * 50


BAD_ID_SNIPPET = """
#include "cimba/runner.hpp"
#include "models/mm1_tally.hpp"
int main() {
    auto store = std::make_unique<cmb::Engine<cmb_models::MM1Tally>::Storage>();
    cmb::Engine<cmb_models::MM1Tally> E(*store);
    CMB_TALLY(TALLY_ID, 1.0);
    return 0;
}
"""


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="no clang++")
def test_constant_id_out_of_range_does_not_compile(tmp_path):
    src = tmp_path / "tally_id.cpp"
    src.write_text(BAD_ID_SNIPPET)
    csrc = os.path.join(ROOT, "cimba_amd", "csrc")

    def syntax_only(tally_id):
        return subprocess.run(
            [CLANGXX, "-std=c++17", "-fsyntax-only", f"-DTALLY_ID={tally_id}",
             "-I" + csrc, "-I" + os.path.join(csrc, "include"), str(src)],
            capture_output=True, text=True, timeout=300)

    assert syntax_only(1).returncode == 0
    bad = syntax_only(2)  # MM1Tally has two tallies
    assert bad.returncode != 0
    assert "CMB_TALLY id is not below Cfg::DEVICE_TALLY" in bad.stderr


# ---- host code under sanitizers -----------------------------------------------

@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="no clang++")
def test_tally_selfcheck_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tally_selfcheck")
    cc = subprocess.run(
        [CLANGXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "cimba_amd", "csrc", "include"),
         os.path.join(ROOT, "scripts", "tally_selfcheck.cpp"),
         os.path.join(ROOT, "cimba_amd", "csrc", "host", "support.cpp"),
         "-lpthread", "-o", exe],
        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=env)
    assert run.returncode == 0, (run.stdout, run.stderr[-3000:])
    assert "tally selfcheck OK" in run.stdout
