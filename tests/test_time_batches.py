"""Regular-grid time averages (timeseries.time_batches): the host path and
both GPU tiers against a plain double loop over samples and batches in exact
rational arithmetic on the double edges ``start + j * w``.  In the exact
cases values are integers up to 2^10 and times, start and end lie on a grid
of 2^-10 below 2^10 with ``end - start`` a multiple of ``K * 2^-10``, so
every edge, product and partial sum fits 53 bits: bit for bit."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from cimba_amd import _C, steadystate as ss, timeseries as ts

BACKENDS = [False, pytest.param(True, marks=pytest.mark.gpu)]
W, C = _C.TBATCH_WAVE_MAX, _C.TBATCH_CHUNK
GRID = 2.0 ** -10
KEYS = ("n", "width", "integral", "covered", "means")
# (T, N, K, lengths, window).  Windows: "full" is [0, end] with the first
# sample at 0 and a scalar end past every time, w a power of two; "late" is
# [-end, end], so the first half of the batches is empty; "cut" is per row,
# start on the time of sample 2, edge 1 on the time of a later sample and
# the end before the last sample; "off" is "cut" with rows 0, 1 and 2 off.
CASES = (
    # N + K around the tier edge; T = 3 leaves a workgroup of the wave tier
    # a row short; K = 7 is no power of two
    [(3, W - K - 1 + d, K, None, "cut") for K in (7,) for d in (0, 1, 2)] +
    # m + K around one chunk and past two with K = 2: a batch open across
    # chunks.  N + K - 1 merge steps: C - 2, C (one full chunk), C + 1, 2C + 4
    [(2, n, 2, None, "cut") for n in (C - 3, C - 1, C, 2 * C + 3)] +
    # one batch; one sample spanning hundreds of batches, in one chunk and
    # across three
    [(2, 40, 1, None, "full"), (2, 3, 1000, None, "full"),
     (2, 3, 5000, None, "late")] +
    # ragged rows per tier, leading empty batches, off rows
    [(5, 300, 16, (0, 1, 17, 299, 300), "cut"),
     (5, 2100, 64, (0, 1, 1025, 2048, 2100), "cut"),
     (3, 300, 16, None, "full"), (3, 300, 16, None, "late"),
     (3, 2100, 64, None, "late"), (5, 300, 16, None, "off"),
     (5, 2100, 7, None, "off")])
# non-dyadic values, exponential gaps: one shape per tier
ROUNDING = [(3, 300, 16), (2, 2500, 48)]


@functools.lru_cache(maxsize=None)
def build(T, N, K, window, dyadic=True):
    """The one input builder: values, times, start, end.  Read-only.  One gap
    in eight is zero (tied times); from 64 samples on, row 1 has a NaN time
    in the middle and one at its end."""
    rng = np.random.default_rng(1000 * N + 10 * K + T)
    if not dyadic:
        x = rng.standard_normal((T, N))
        t = np.cumsum(rng.exponential(1.0, (T, N)), axis=1)
        return x, t, 0.7, float(t[:, 3 * N // 4].min())
    x = rng.integers(-1024, 1025, (T, N)).astype(np.float64)
    gap = rng.integers(1, 17, (T, N)) * (rng.integers(0, 8, (T, N)) > 0)
    gap[:, 0] = 0
    u = np.cumsum(gap, axis=1)  # times in units of GRID
    if window in ("full", "late"):
        per = 2 ** math.ceil(math.log2((int(u.max()) + 1) / K + 1))
        end = K * per * GRID
        start = 0.0 if window == "full" else -end
    else:
        per = np.maximum(u[:, 2 + (3 * N // 4) // K] - u[:, 2], 1)
        start = u[:, 2] * GRID
        end = (u[:, 2] + K * per) * GRID
    if window == "off":
        end[0] = start[0]
        start[1] = -np.inf
        end[2] = np.nan
    t = u * GRID
    if N >= 64 and T > 1:
        t[1, N // 2] = t[1, N - 1] = np.nan
    for a in (x, t):
        a.setflags(write=False)
    return x, t, start, end


@functools.lru_cache(maxsize=None)
def reference(T, N, K, lengths, window, dyadic=True):
    """n, width, integral, covered, means as correctly rounded doubles of the
    exact sums, and per batch the piece count and the exact sum of |x| ov."""
    x, t, start, end = build(T, N, K, window, dyadic)
    start, end = np.broadcast_to(start, T), np.broadcast_to(end, T)
    out = {k: np.zeros((T, K)) for k in ("integral", "covered", "pieces",
                                         "abs")}
    out.update(n=np.zeros(T), width=np.full(T, np.nan),
               means=np.full((T, K), np.nan))
    for r in range(T):
        s, e = start[r], end[r]
        if not (np.isfinite(s) and np.isfinite(e) and e > s):
            continue
        w = (e - s) / np.float64(K)
        edges = [s + np.float64(j) * w for j in range(K)] + [e]
        m = N if lengths is None else min(lengths[r], N)
        nxt = [t[r, i + 1] if i + 1 < m else e for i in range(m)]
        out["width"][r] = w
        out["n"][r] = sum(min(nxt[i], e) > max(t[r, i], s) for i in range(m))
        for j in range(K):
            integral = covered = absx = Fraction(0)
            for i in range(m):
                a, b = max(t[r, i], edges[j]), min(nxt[i], edges[j + 1])
                if b > a:  # False when either time is NaN
                    ov = Fraction(b) - Fraction(a)
                    integral += Fraction(x[r, i]) * ov
                    absx += abs(Fraction(x[r, i])) * ov
                    covered += ov
                    out["pieces"][r, j] += 1
            out["integral"][r, j] = float(integral)
            out["covered"][r, j] = float(covered)
            out["abs"][r, j] = float(absx)
            if covered:
                out["means"][r, j] = float(integral / covered)
    return out


def run(T, N, K, lengths, window, gpu, dyadic=True):
    x, t, start, end = build(T, N, K, window, dyadic)
    return ts.time_batches(x, t, end, K, start_time=start, lengths=lengths,
                           gpu=gpu)


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[1]}x{c[2]}-{c[4]}")
def test_exact(case, gpu):
    got, want = run(*case, gpu), reference(*case)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("T, N, K", ROUNDING)
def test_rounding(T, N, K, gpu):
    got = run(T, N, K, None, "free", gpu, dyadic=False)
    want = reference(T, N, K, None, "free", dyadic=False)
    tol = (want["pieces"] + 3) * 2.0 ** -53
    err_i = np.abs(got["integral"] - want["integral"])
    err_c = np.abs(got["covered"] - want["covered"])
    print("max error / bound:", (err_i / (tol * want["abs"])).max(),
          (err_c / (tol * want["covered"])).max())
    assert np.all(err_i <= tol * want["abs"])
    assert np.all(err_c <= tol * want["covered"])
    np.testing.assert_array_equal(got["n"], want["n"])


@pytest.mark.parametrize("gpu", BACKENDS)
def test_feeds_batch_means(gpu):
    """The output is a series the steady-state module takes as it is: the
    mean of the batch means is the time average over the whole window."""
    got = run(1, 300, 16, None, "full", gpu)  # one row: no NaN time, no gap
    mean = ss.batch_means(got["means"], 1, levels=3, gpu=gpu)["mean"][:, 0]
    want = got["integral"].sum(1) / got["covered"].sum(1)
    assert np.all(np.abs(mean - want) <= 4 * np.spacing(np.abs(want)))


@pytest.mark.parametrize("gpu", BACKENDS)
def test_arguments(gpu):
    x, t = np.zeros((3, 5)), np.tile(np.arange(5.0), (3, 1))
    for bad in (lambda: ts.time_batches(x, t, 5.0, 0, gpu=gpu),
                lambda: ts.time_batches(x, t, 5.0, 65537, gpu=gpu),
                lambda: ts.time_batches(x[0], t[0], 5.0, 4, gpu=gpu),
                lambda: ts.time_batches(x, t[:, :4], 5.0, 4, gpu=gpu),
                lambda: ts.time_batches(x, t, 5.0, 4, start_time=np.zeros(4),
                                        gpu=gpu)):
        with pytest.raises(ValueError):
            bad()
    got = ts.time_batches(x[:0], t[:0], 5.0, 4, gpu=gpu)
    assert got["n"].shape == got["width"].shape == (0,)
    assert all(got[k].shape == (0, 4) for k in KEYS[2:])
    assert ts.batch_means_of(x[:0], t[:0], 5.0, 4, gpu=gpu).shape == (0, 4)
