"""Steady state (cimba_amd/steadystate.py): the MSER-m cut and the batch-
means ladder, GPU kernels and host loops, against numpy in longdouble.

The reference forms every batch mean in float64 in the stated order
(left-to-right sum, one division; pairwise (a + b) / 2 up the ladder), so
counts, cuts and batch means are exact.  Its sums are longdouble.  For MSER
they are reversed cumulative sums of y - shift and (y - shift)^2 (shift = the
row's mean: M2 does not depend on it, and after it the subtraction
S2 - S1^2 / c loses a few of longdouble's 11 spare bits, no more).

Ladder, per level with k means y (tests/test_correlogram.py with n = k):
    tol_mean = k 2^-53 mean|y|
    tol_sse, tol_c1 = k 2^-52 (sum |d_j||d_{j+lag}| + mean|y| sum |d_j|)
    tol_dsq = (k + 2) 2^-52 dsq   (one rounding in each difference and
              square, k in any order of summation, all terms positive)

MSER, suffix of c = k - d means, M2 its centred sum of squares, A = max|y|,
u = 2^-53.  Moments2::merge rounds seven times on the way to M2 (d, d^2, two
products, a quotient, two sums) and four times on the way to the mean; a
merge averages the mean errors it is given, so a mean that went through D
merges is off by at most 4 D u A.  2^-52 = 2u pays for the second-order
terms, and two more roundings are in M2 / c^2.

Host: one mean at a time, c merges.  Step i adds t_i = d_i^2 i / (i + 1),
and the t_i sum to M2 exactly (Welford), so the five roundings of t_i cost
5 u M2 in all and the two sums 2 u M2 a step.  The running mean's error,
at most 4 c u A, enters t_i through 2 |d_i| i / (i + 1) times it; by
Cauchy-Schwarz sum |d_i| i / (i + 1) <= sqrt(c M2).  Linear in c:
    tol_stat(d) = c 2^-52 (9 M2 + 8 A sqrt(c M2)) / c^2
GPU: a tree.  Pieces merged at one depth are disjoint, so their own M2 add
up to at most M2: 7 u M2 a depth.  The two means' errors, 8 D u A, enter
through 2 |d| n_a n_b / n_x, and n_a n_b |d| / n_x <= sum |y - mean| / 2 over
the piece, at most 2 sqrt(c M2) over a depth.  The depth is four in the
lane, six across the wave, one per chunk behind, one for the carry and four
in the rescan, D = ceil(k / 256) + 15:
    tol_stat(d) = D 2^-52 (9 M2 + 16 D A sqrt(c M2)) / c^2
Both: tol_mean(d) = D 2^-51 A, D = c on the host.  d must be as good as the
reference's within the two tolerances, stat within tol of the reference at
the d that was returned."""
import functools

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C, correlogram as cg, steadystate as st

LD = np.longdouble
BACKENDS = [False, pytest.param(True, marks=pytest.mark.gpu)]
CH, WMAX = _C.SSTAT_CHUNK, _C.SSTAT_WAVE_MAX
ROUND = CH * _C.SSTAT_BLOCK_WAVES
M_DIRECT = _C.SSTAT_M_STAGE + 1  # summed from global memory, not via LDS
# lanes, a lane's four registers, one chunk, two chunks (the carry)
WAVE_K = (0, 1, 2, 3, 4, 5, 63, 64, 65, 128, CH - 1, CH, CH + 1,
          2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH + 1)


def width(m, k):
    """k batches and m - 1 observations over: n < m, n no multiple of m"""
    return k * m + m - 1


# (m, N): wave tier edges, the tier threshold, one round of the block tier
SHAPES = (
    [(m, width(m, k)) for m in (1, 5, 8) for k in WAVE_K] +
    [(m, n) for m in (1, 5, 8) for n in (WMAX - 1, WMAX, WMAX + 1)] +
    [(1, width(1, 9 * ROUND + e)) for e in (-1, 0, 1)] +
    [(m, width(m, 2 * ROUND + e)) for m in (5, 8) for e in (-1, 0, 1)] +
    [(M_DIRECT, width(M_DIRECT, k)) for k in (65, 2 * CH + 1, ROUND + 1)])
# (T, N, m, lengths, skip, row stride), once per tier
RAGGED = ((5, 700, 5, (0, 1, 705, 333, 700), (0, 5, 17, 400, 700), 733),
          (5, 9000, 5, (0, 1, 9005, 4000, 9000), (0, 3, 50, 4100, 8000), 9100))


@functools.lru_cache(maxsize=None)
def series(T, n):
    """AR(1), rho = 0.9, offset +10, plus a transient 8 exp(-s / 50), so the
    MSER curve has a minimum inside.  Read-only."""
    rng = np.random.default_rng(1000 * T + n)
    e = rng.standard_normal((T, max(n, 1)))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - 0.81)
    for s in range(1, x.shape[1]):
        x[:, s] = 0.9 * x[:, s - 1] + e[:, s]
    x += 10.0 + 8.0 * np.exp(-np.arange(x.shape[1]) / 50.0)
    x.setflags(write=False)
    return x[:, :n]


def rows(x, lengths, skip):
    skip = np.broadcast_to(skip, len(x))
    for t, row in enumerate(x):
        end = len(row) if lengths is None else min(lengths[t], len(row))
        yield t, skip[t], row[min(skip[t], end):end]


def level0(xs, m):
    b = xs[:len(xs) // m * m].reshape(-1, m)
    s = np.zeros(len(b))
    for i in range(m):
        s = s + b[:, i]
    return s / m


def mser_ref(y, gpu):
    """curve, its tolerance, ybar_d and its tolerance for d = 0 .. k // 2"""
    k, dmax = len(y), len(y) // 2
    shift = LD(np.nanmean(y))
    z = y.astype(LD) - shift
    c = (k - np.arange(dmax + 1)).astype(LD)
    s1 = np.cumsum(z[::-1])[::-1][:dmax + 1]
    m2 = np.maximum(np.cumsum((z * z)[::-1])[::-1][:dmax + 1] - s1 * s1 / c, 0)
    amax = LD(np.nanmax(np.abs(y)))
    spread = amax * np.sqrt(c * m2)
    D = LD(-(-k // CH) + 15)
    tol = (D * (9 * m2 + 16 * D * spread) if gpu else
           c * (9 * m2 + 8 * spread)) * LD(2.0) ** -52 / (c * c)
    return (m2 / (c * c), tol, shift + s1 / c,
            (D + 0 * c if gpu else c) * LD(2.0) ** -51 * amax)


def check_mser(res, x, m, lengths=None, skip=0, gpu=False):
    for t, sk, xs in rows(x, lengths, skip):
        y = level0(xs, m)
        k, dmax = len(y), len(y) // 2
        assert (res["n"][t], res["k"][t]) == (len(xs), k)
        d = int(res["d"][t])
        assert res["cut"][t] == sk + d * m and d <= dmax
        if "curve" in res:
            assert np.all(np.isnan(res["curve"][t, dmax + 1 if k else 0:]))
        if k == 0 or np.any(np.isnan(y[dmax:])):
            assert d == 0 and np.isnan(res["stat"][t])
            assert np.isnan(res["mean"][t])
            continue
        curve, tol, mean, tol_mean = mser_ref(y, gpu)
        best = int(np.nanargmin(curve))
        assert not np.isnan(curve[d])
        assert curve[d] <= curve[best] + tol[d] + tol[best], (t, d, best)
        assert abs(res["stat"][t] - curve[d]) <= tol[d]
        assert abs(res["mean"][t] - mean[d]) <= tol_mean[d]
        if "curve" in res:
            got = res["curve"][t, :dmax + 1]
            assert np.array_equal(np.isnan(got), np.isnan(curve))
            ok = ~np.isnan(curve)
            assert np.all(np.abs(got[ok] - curve[ok]) <= tol[ok])


def check_ladder(res, x, m, levels, lengths=None, skip=0):
    assert res["k"].shape == (len(x), levels)
    for t, _, xs in rows(x, lengths, skip):
        y = level0(xs, m)
        for lv in range(levels):
            if lv:
                y = (y[0:len(y) // 2 * 2:2] + y[1::2]) / 2
            k = len(y)
            got = [res[key][t, lv] for key in ("mean", "sse", "c1", "dsq")]
            assert res["k"][t, lv] == k
            if k == 0:
                assert np.isnan(got[0]) and got[1:] == [0.0, 0.0, 0.0]
                continue
            yl = y.astype(LD)
            absy = np.abs(yl).sum() / k
            mean = yl.sum() / k
            d = yl - mean
            ref = [mean, (d * d).sum(), (d[:-1] * d[1:]).sum(),
                   ((yl[1:] - yl[:-1]) ** 2).sum()]
            spread = absy * np.abs(d).sum()
            tol = [k * LD(2.0) ** -53 * absy,
                   k * LD(2.0) ** -52 * ((d * d).sum() + spread),
                   k * LD(2.0) ** -52 * (np.abs(d[:-1] * d[1:]).sum() +
                                         spread) if k > 1 else 0,
                   (k + 2) * LD(2.0) ** -52 * ref[3]]
            for name, g, r, tl in zip(("mean", "sse", "c1", "dsq"), got, ref,
                                      tol):
                assert abs(g - r) <= tl, (name, t, lv, k, float(g - r))


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("m,n", SHAPES)
def test_mser(m, n, gpu):
    x = series(3, n)
    check_mser(st.mser(x, m, want_curve=True, gpu=gpu), x, m, gpu=gpu)
    res = st.mser(x, m, gpu=gpu)
    assert "curve" not in res
    check_mser(res, x, m, gpu=gpu)


# seven levels at every shape; one and two (other branches of the kernel,
# whatever m is) at m = 5; twelve where the cascade has chunks to pair
LADDER = ([(m, n, 7) for m, n in SHAPES] +
          [(m, n, lv) for m, n in SHAPES if m == 5 for lv in (1, 2)] +
          [(m, n, 12) for m, n in SHAPES if n // m >= 2 * CH])


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("m,n,levels", LADDER)
def test_batch_means(m, n, levels, gpu):
    x = series(3, n)
    check_ladder(st.batch_means(x, m, levels=levels, gpu=gpu), x, m, levels)


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("case", RAGGED, ids=("wave", "block"))
def test_ragged_strided(case, gpu):
    T, N, m, lengths, skip, stride = case
    x = series(T, stride)[:, :N]
    skip = np.array(skip, dtype=np.uint32)
    check_mser(st.mser(x, m, lengths=lengths, skip=skip, want_curve=True,
                       gpu=gpu), x, m, lengths, skip, gpu)
    check_mser(st.mser(x, m, lengths=lengths, skip=7, gpu=gpu), x, m,
               lengths, 7, gpu)
    check_ladder(st.batch_means(x, m, levels=10, lengths=lengths, skip=skip,
                                gpu=gpu), x, m, 10, lengths, skip)


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("n", (40, 2 * CH * 4 + 8, WMAX + 40))
def test_tie_and_nan_rules(n, gpu):
    """No tolerance: a constant row; a step after three batches; a NaN in
    the first quarter of a constant row (the first d past it) and of a row
    with a plain minimum (the reference's d); a NaN in the second half."""
    m, k = 4, n // 4
    q = k // 8
    x = np.full((5, n), 1.5)
    x[1, 3 * m:] = 0.0
    x[1, :3 * m] = 1.0
    x[3:] = series(2, n)
    x[2:4, q * m + 1] = np.nan
    x[4, (k // 2) * m + 2] = np.nan
    res = st.mser(x, m, want_curve=True, gpu=gpu)
    assert res["d"].tolist()[:3] == [0, 3, q + 1] and res["d"][4] == 0
    assert res["stat"].tolist()[:3] == [0.0, 0.0, 0.0]
    assert res["mean"].tolist()[:3] == [1.5, 0.0, 1.5]
    assert np.isnan(res["stat"][4]) and np.isnan(res["mean"][4])
    assert np.all(np.isnan(res["curve"][2:4, :q + 1]))
    assert not np.any(np.isnan(res["curve"][2:4, q + 1:k // 2 + 1]))
    assert np.all(np.isnan(res["curve"][4]))
    curve, tol, _, _ = mser_ref(level0(x[3], m), gpu)
    best = int(np.nanargmin(curve))
    others = np.delete(curve, best)
    assert np.nanmin(others) - curve[best] > 4 * np.nanmax(tol)  # a plain one
    assert res["d"][3] == best and best > q
    check_mser({key: v[3:] for key, v in res.items() if key != "elapsed_ms"},
               x[3:], m, gpu=gpu)


@pytest.mark.parametrize("gpu", BACKENDS)
def test_bad_arguments_then_valid(gpu):
    x = series(3, 40)
    for call in (lambda: st.mser(x, 0, gpu=gpu),
                 lambda: st.batch_means(x, 0, gpu=gpu),
                 lambda: st.batch_means(x, 5, levels=0, gpu=gpu),
                 lambda: st.batch_means(x, 5, levels=17, gpu=gpu),
                 lambda: st.mser(x[0], 5, gpu=gpu),
                 lambda: st.batch_means(x[:0], 5, gpu=gpu),
                 lambda: st.mser(x, 5, skip=[1, 2], gpu=gpu)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        st.mser(x, 5, skip=1.5, gpu=gpu)
    check_mser(st.mser(x, 5, gpu=gpu), x, 5, gpu=gpu)
    check_ladder(st.batch_means(x, 5, levels=16, gpu=gpu), x, 5, 16)


def test_derived_statistics():
    x = series(3, 700)
    res = st.batch_means(x, 5, levels=8, gpu=False)
    k, sse = res["k"], res["sse"]
    assert np.all(np.isnan(st.variance(res)[k < 2]))
    ok = k >= 2
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(st.variance(res)[ok], (sse / (k - 1))[ok])
        assert np.array_equal(st.stderr(res)[ok], np.sqrt(sse / (k - 1) / k)[ok])
        assert np.array_equal(st.lag1(res)[ok], (res["c1"] / sse)[ok])
        assert np.array_equal(st.von_neumann(res)[ok], (res["dsq"] / sse)[ok])
    assert np.all(st.lag1(res)[sse <= 0] == 0.0)


@pytest.mark.gpu
def test_gpu_deterministic():
    x = series(3, WMAX + 1)
    for call in (lambda: st.mser(x, 5, want_curve=True, gpu=True),
                 lambda: st.batch_means(x, 5, levels=12, gpu=True)):
        a, b = call(), call()
        for key in a:
            if key != "elapsed_ms":
                assert a[key].tobytes() == b[key].tobytes()


@pytest.mark.gpu
def test_gpu_log_to_standard_error():
    r = ca.mm1log_gpu(ntrials=4, num_objects=300, seed=7, log_count=4,
                      log_capacity=2048)
    x, lengths = cg.series_from_log(r, _C.LC_DEPART)
    res = st.mser(x, 5, lengths=lengths, gpu=True)
    assert res["cut"].shape == (4,) and np.all(res["cut"] < lengths)
    check_mser(res, x, 5, lengths, gpu=True)
    host = st.mser(x, 5, lengths=lengths, gpu=False)
    check_mser(host, x, 5, lengths, gpu=False)
    lad = st.batch_means(x, 5, levels=4, lengths=lengths, skip=res["cut"],
                         gpu=True)
    assert st.stderr(lad).shape == (4, 4)
    check_ladder(lad, x, 5, 4, lengths, res["cut"])
    check_ladder(st.batch_means(x, 5, levels=4, lengths=lengths,
                                skip=res["cut"], gpu=False),
                 x, 5, 4, lengths, res["cut"])
