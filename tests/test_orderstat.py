"""Order statistics (cimba_amd/orderstat.py): the GPU sorting tiers and the
host path against plain Python and numpy -- sorted() under the total order
(-0.0 before +0.0, NaN last), the Dataset quantile and histogram formulas
in float64.  Every comparison is exact: sorted values and quantiles bit for
bit where they are numbers and NaN where the reference is NaN, counts and
lengths equal."""
import functools
import math

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C, correlogram as cg, orderstat as os_

BACKENDS = [False, pytest.param(True, marks=pytest.mark.gpu)]
W, B = _C.OSTAT_WAVE_MAX, _C.OSTAT_BLOCK_MAX
RAGGED = (0, 1, 17, 299, 300)
Q = (0, 0.1, 0.25, 0.5, 0.75, 0.999, 1)
NBINS = 7
# (T, N, lengths, skip, row stride, pattern)
CASES = (
    # lane and K edges of the wave tier, register-blocking edges of the
    # block tier, three chunks padded to four, two global launches a merge
    [(3, n, None, 0, n, "normal") for n in (
        1, 2, 3, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1, 2047, 2048,
        2049, B - 1, B, B + 1, 2 * B + 1, 8 * B + 5)] +
    # ragged and skip (skip 20 empties the rows of length 0, 1 and 17)
    [(5, 300, RAGGED, skip, 300, "normal") for skip in (0, 16, 20)] +
    [(5, 300, RAGGED, 16, 333, "normal")] +
    # every pattern once per tier
    [(3, n, None, 0, n, p) for n in (300, 2049, 2 * B + 1)
     for p in ("ascending", "descending", "equal", "mod7")])


@functools.lru_cache(maxsize=None)
def pattern(name, T, width):
    """The one seeded input generator.  Read-only."""
    rng = np.random.default_rng(100 * T + width)
    x = rng.standard_normal((T, width))
    if name == "ascending":
        x = np.sort(x, axis=1)
    elif name == "descending":
        x = np.sort(x, axis=1)[:, ::-1].copy()
    elif name == "equal":
        x = np.full((T, width), 3.25)
    elif name == "mod7":
        x = (rng.integers(0, 1000, (T, width)) % 7).astype(np.float64)
    x.setflags(write=False)
    return x


def reference(x, lengths=None, skip=0, q=Q, nbins=NBINS):
    """n, sorted, quantiles, hist from the definitions."""
    T, N = x.shape
    n = np.zeros(T)
    srt = np.full((T, N), np.nan)
    qs = np.full((T, len(q)), np.nan)
    hist = np.zeros((T, nbins), dtype=np.int64)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for t in range(T):
            row = x[t, skip:N if lengths is None else min(lengths[t], N)]
            xs = np.array(sorted(row, key=lambda v: (
                math.isnan(v), v, not np.signbit(v))), dtype=np.float64)
            n[t] = m = len(xs)
            if m == 0:
                continue
            srt[t, :m] = xs
            for i, qi in enumerate(q):
                pos = np.float64(qi) * np.float64(m - 1)
                lo = int(pos)
                frac = pos - np.float64(lo)
                qs[t, i] = xs[-1] if lo + 1 >= m else (
                    xs[lo] * (one - frac) + xs[lo + 1] * frac)
            if np.isfinite(xs[0]) and np.isfinite(xs[-1]):
                w = (xs[-1] - xs[0]) / nbins if xs[-1] > xs[0] else one
                b = np.clip((xs - xs[0]) / w, 0, nbins - 1).astype(np.int64)
                hist[t] = np.bincount(b, minlength=nbins)
    return n, srt, qs, hist


@functools.lru_cache(maxsize=None)
def case_ref(case):
    T, N, lengths, skip, stride, pat = case
    return reference(pattern(pat, T, stride)[:, :N], lengths, skip)


def same_doubles(got, want):
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64),
                          want[~nan].view(np.uint64))


def check(res, ref):
    n, srt, qs, hist = ref
    assert np.array_equal(res["n"], n)
    same_doubles(res["sorted"], srt)
    same_doubles(res["quantiles"], qs)
    assert np.array_equal(res["hist"], hist)


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-N%d-%s-skip%d-"
                         "stride%d-%s" % (c[0], c[1], "ragged" if c[2]
                                          else "full", c[3], c[4], c[5]))
def test_order_stats(case, gpu):
    T, N, lengths, skip, stride, pat = case
    x = pattern(pat, T, stride)[:, :N]
    res = os_.order_stats(x, q=Q, nbins=NBINS, want_sorted=True,
                          lengths=lengths, skip=skip, gpu=gpu)
    check(res, case_ref(case))


@pytest.mark.parametrize("gpu", BACKENDS)
def test_special_values(gpu):
    x = pattern("normal", 5, 70).copy()
    tiny = 5e-324
    x[0, :8] = (0.0, -0.0, tiny, -tiny, -0.0, 0.0, 1e-310, -1.7e308)
    x[1, 3], x[2, 60], x[4, 7] = np.inf, -np.inf, 1.7e308
    x[3, 5], x[3, 69], x[3, 20] = np.nan, -np.nan, np.inf
    ref = reference(x)
    res = os_.order_stats(x, q=Q, nbins=NBINS, want_sorted=True, gpu=gpu)
    check(res, ref)
    s = res["sorted"]
    zeros = s[0][s[0] == 0.0]
    assert list(np.signbit(zeros)) == [True, True, False, False]
    assert np.isnan(s[3, -2:]).all() and s[3, -3] == np.inf
    assert not res["hist"][1:4].any()
    assert (res["hist"][[0, 4]].sum(axis=1) == 70).all()
    assert np.isnan(res["quantiles"][3, -1])
    assert res["quantiles"][1, -1] == np.inf


@pytest.mark.parametrize("gpu", BACKENDS)
def test_outputs_optional_and_bad_arguments(gpu):
    x = pattern("normal", 3, 65)
    full = os_.order_stats(x, q=Q, nbins=NBINS, want_sorted=True, gpu=gpu)
    for key, kw in (("sorted", {"want_sorted": True}), ("quantiles", {"q": Q}),
                    ("hist", {"nbins": NBINS})):
        one = os_.order_stats(x, gpu=gpu, **kw)
        assert set(one) == {"n", "elapsed_ms", key}
        assert one[key].tobytes() == full[key].tobytes()
    for series, kw in ((x, {"q": (1.5,)}), (x, {"nbins": -1}),
                       (x[0], {"q": Q}), (x[:0], {"q": Q})):
        with pytest.raises(ValueError):
            os_.order_stats(series, gpu=gpu, **kw)
    check(os_.order_stats(x, q=Q, nbins=NBINS, want_sorted=True, gpu=gpu),
          reference(x))


def test_matches_dataset():
    x = pattern("normal", 3, 301)[:1]
    ds = _C.Dataset()
    for v in x[0]:
        ds.add(v)
    assert tuple(os_.fivenum(x, gpu=False)[0]) == ds.fivenum()
    assert os_.median(x, gpu=False)[0] == ds.median()
    assert list(os_.histogram(x, 10, gpu=False)[0]) == list(ds.histogram(10))
    assert list(os_.sort_rows(x, gpu=False)[0]) == sorted(x[0])


@pytest.mark.gpu
def test_gpu_log_to_fivenum():
    r = ca.mm1log_gpu(ntrials=4, num_objects=300, seed=7, log_count=4,
                      log_capacity=1024)
    x, lengths = cg.series_from_log(r, _C.LC_DEPART)
    assert x.shape == (4, 300)
    g = os_.fivenum(x, lengths=lengths, skip=20, gpu=True)
    h = os_.fivenum(x, lengths=lengths, skip=20, gpu=False)
    assert g.shape == (4, 5) and g.tobytes() == h.tobytes()
    assert np.all(np.diff(g, axis=1) >= 0.0)
