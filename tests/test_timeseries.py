"""Time-weighted order statistics (cimba_amd/timeseries.py): the GPU tiers
and the host path against plain Python -- weights from the definition,
sorted() on (isnan, value, not signbit, weight), a running sum.  Times,
start and end lie on a grid of 2^-10 below 2^20, so every partial sum of
durations is exact in double in any order and every comparison is exact:
bit for bit where the reference is a number, NaN where it is NaN."""
import functools
import math

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C, timeseries as ts

BACKENDS = [False, pytest.param(True, marks=pytest.mark.gpu)]
W, B = _C.TSTAT_WAVE_MAX, _C.TSTAT_BLOCK_MAX
Q = (0, 0.1, 0.25, 0.5, 0.75, 0.999, 1)
NBINS = 7
GRID = 2.0 ** -10
# (T, N, lengths, row stride, pattern, window); window "full" is a scalar end
# past every time and no start, "cut" is per-row start and end arrays: start
# strictly inside sample 10, end at the time of sample 3 N / 4
CASES = (
    # lane and K edges of the wave tier, the tier threshold, register-
    # blocking edges and the largest row of the block tier
    [(3, n, None, n, "normal", "full") for n in (
        1, 2, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1, 2047, 2048, 2049,
        B - 1, B)] +
    # every pattern once per tier
    [(3, n, None, n, p, "full") for n in (300, 2049)
     for p in ("levels", "equal", "ascending", "descending")] +
    # ragged rows, a wider stride and the window, once per tier; T = 5 puts
    # rows of two blocks into one wave-tier launch
    [(5, 300, (0, 1, 17, 299, 300), 333, "levels", "cut"),
     (5, 2049, (0, 1, 1025, 2048, 2049), 2100, "normal", "cut")])


@functools.lru_cache(maxsize=None)
def history(name, T, width):
    """The one seeded input generator: values and times.  Read-only.  One
    increment in eight is zero (a dropped sample); increment 11 is not."""
    rng = np.random.default_rng(100 * T + width)
    x = rng.standard_normal((T, width))
    if name == "levels":
        x = rng.integers(0, 7, (T, width)).astype(np.float64)
    elif name == "equal":
        x = np.full((T, width), 3.25)
    elif name in ("ascending", "descending"):
        x = np.sort(x, axis=1)
        x = x if name == "ascending" else x[:, ::-1].copy()
    dt = rng.integers(1, 64, (T, width)) * (rng.integers(0, 8, (T, width)) > 0)
    dt[:, 11:12] = 4
    t = np.cumsum(dt, axis=1) * GRID
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def window(t, N, kind):
    if kind == "full":
        return -np.inf, 600.0
    return t[:, min(10, N - 1)] + GRID, t[:, 3 * N // 4].copy()


def reference(x, t, end, start=-np.inf, lengths=None, q=Q, nbins=NBINS):
    """n, total, quantiles, hist, values, cum from the definitions."""
    T, N = x.shape
    start, end = np.broadcast_to(start, T), np.broadcast_to(end, T)
    n, total = np.zeros(T), np.zeros(T)
    qs = np.full((T, len(q)), np.nan)
    hist = np.zeros((T, nbins))
    vals, cum = np.full((T, N), np.nan), np.full((T, N), np.nan)
    for r in range(T):
        m = N if lengths is None else min(lengths[r], N)
        pairs = []
        for i in range(m):
            a = np.maximum(t[r, i], start[r])
            b = np.minimum(t[r, i + 1] if i + 1 < m else end[r], end[r])
            if b - a > 0:
                pairs.append((float(x[r, i]), float(b - a)))
        pairs.sort(key=lambda p: (math.isnan(p[0]),
                                  0.0 if math.isnan(p[0]) else p[0],
                                  not np.signbit(p[0]), p[1]))
        n[r] = k = len(pairs)
        if k == 0:
            continue
        vals[r, :k] = v = np.array([p[0] for p in pairs])
        wt = np.array([p[1] for p in pairs])
        acc = 0.0
        for i in range(k):
            acc += pairs[i][1]
            cum[r, i] = acc
        total[r] = acc
        for i, qi in enumerate(q):
            qs[r, i] = v[np.argmax(cum[r, :k] >= np.float64(qi) * acc)]
        if np.isfinite(v[0]) and np.isfinite(v[-1]):
            width = (v[-1] - v[0]) / nbins if v[-1] > v[0] else 1.0
            b = np.clip((v - v[0]) / width, 0, nbins - 1).astype(np.int64)
            hist[r] = [math.fsum(wt[b == j]) for j in range(nbins)]
    return n, total, qs, hist, vals, cum


def run(case, gpu, **kw):
    T, N, lengths, stride, pat, win = case
    x, t = (a[:, :N] for a in history(pat, T, stride))
    start, end = window(t, N, win)
    return ts.time_stats(x, t, end, start_time=start, lengths=lengths,
                         gpu=gpu, **(kw or dict(q=Q, nbins=NBINS,
                                                want_sorted=True)))


@functools.lru_cache(maxsize=None)
def case_ref(case):
    T, N, lengths, stride, pat, win = case
    x, t = (a[:, :N] for a in history(pat, T, stride))
    start, end = window(t, N, win)
    return reference(x, t, end, start, lengths)


def same_doubles(got, want):
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64),
                          want[~nan].view(np.uint64))


def check(res, ref):
    for key, want in zip(("n", "total", "quantiles", "hist", "values", "cum"),
                         ref):
        same_doubles(res[key], want)


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-N%d-%s-stride%d-"
                         "%s-%s" % (c[0], c[1], "ragged" if c[2] else "full",
                                    c[3], c[4], c[5]))
def test_time_stats(case, gpu):
    res = run(case, gpu)
    check(res, case_ref(case))
    if case[5] == "cut":
        assert res["n"][0] == 0 and res["n"][-1] < case[1]


@pytest.mark.parametrize("gpu", BACKENDS)
def test_longer_than_block_tier(gpu):
    case = (3, B + 1, None, B + 1, "normal", "full")
    if gpu:
        with pytest.raises(ValueError, match=str(B)):
            run(case, True)
    else:
        check(run(case, False), case_ref(case))


@pytest.mark.parametrize("gpu", BACKENDS)
def test_special_values(gpu):
    x, t = (a.copy() for a in history("levels", 4, 70))
    t[0, :5] = t[0, 0] + np.array((0, 3, 7, 9, 12)) * GRID  # weights 3 4 2 3
    x[0, :4] = (0.0, -0.0, -0.0, 0.0)
    x[1, np.flatnonzero(np.diff(t[1]) > 0)[[3, 40]]] = np.nan, np.inf
    t[3, 5] = np.nan
    start = np.array([-np.inf, -np.inf, 600.0, 1.0])
    ref = reference(x, t, 600.0, start)
    res = ts.time_stats(x, t, 600.0, start_time=start, q=Q, nbins=NBINS,
                        want_sorted=True, gpu=gpu)
    check(res, ref)
    v, qs = res["values"], res["quantiles"]
    zeros = v[0] == 0.0
    assert list(np.signbit(v[0][zeros])[:2]) == [True, True]
    assert not np.signbit(v[0][zeros])[2:].any()
    n1 = int(res["n"][1])
    assert np.isnan(v[1, n1 - 1]) and v[1, n1 - 2] == np.inf
    assert np.isnan(qs[1, -1]) and not res["hist"][1].any()
    assert res["n"][2] == 0 and res["total"][2] == 0
    assert np.isnan(qs[2]).all() and not res["hist"][2].any()
    assert res["hist"][3].sum() == res["total"][3] > 0


@pytest.mark.parametrize("gpu", BACKENDS)
def test_outputs_optional_and_bad_arguments(gpu):
    case = (3, 65, None, 65, "normal", "full")
    full = run(case, gpu)
    for keys, kw in ((("values", "cum"), {"want_sorted": True}),
                     (("quantiles",), {"q": Q}), (("hist",), {"nbins": NBINS})):
        one = run(case, gpu, **kw)
        assert set(one) == {"n", "total", "elapsed_ms", *keys}
        for key in keys + ("n", "total"):
            assert one[key].tobytes() == full[key].tobytes()
    x, t = history("normal", 3, 65)
    for xx, tt, kw in ((x, t, {"q": (1.5,)}), (x, t, {"nbins": -1}),
                       (x[0], t[0], {"q": Q}), (x[:0], t[:0], {"q": Q}),
                       (x, t[:, :64], {"q": Q})):
        with pytest.raises(ValueError):
            ts.time_stats(xx, tt, 600.0, gpu=gpu, **kw)


def test_median_matches_timeseries():
    x, t = (a[:1] for a in history("levels", 3, 301))
    series = _C.Timeseries()
    for xi, ti in zip(x[0], t[0]):
        series.add(xi, ti)
    assert ts.median(x, t, 600.0, gpu=False)[0] == series.median(600.0)
    assert ts.fivenum(x, t, 600.0, gpu=False).tobytes() == \
        reference(x, t, 600.0, q=ts.FIVENUM_Q)[2].tobytes()
    assert ts.histogram(x, t, 600.0, 7, gpu=False).tobytes() == \
        reference(x, t, 600.0)[3].tobytes()


@pytest.mark.gpu
def test_gpu_log_to_fivenum():
    r = ca.mm1log_gpu(ntrials=4, num_objects=300, seed=7, log_count=4,
                      log_capacity=1024)
    level, t, lengths = ts.level_from_log(r, _C.LC_ARRIVE, _C.LC_DEPART)
    assert level.shape == t.shape and len(lengths) == 4 and lengths.min() > 300
    end = t[np.arange(4), lengths - 1]
    five = ts.fivenum(level, t, end, lengths=lengths, gpu=True)
    assert five.shape == (4, 5) and (five[:, 0] == 0).all()
    assert np.all(np.diff(five, axis=1) >= 0)
    for i, m in enumerate(lengths):
        wt, lv = np.diff(t[i, :m]), level[i, :m - 1]
        total = math.fsum(wt)
        for q, v in zip(ts.FIVENUM_Q, five[i]):
            below = math.fsum(wt[lv < v])
            upto = math.fsum(wt[lv <= v])
            assert below <= q * total * (1 + 1e-9)
            assert upto >= q * total * (1 - 1e-9)
