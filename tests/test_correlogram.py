"""Correlogram (cimba_amd/correlogram.py): per-trial lag sums from the MFMA
kernel and from the host loops against numpy in longdouble, straight from
the definition c_k = sum_s d_s d_{s+k}, d = x - mean.

Per-lag tolerance, derived (n = effective length of the row):
    tol_k = n * 2^-52 * (sum_s |d_s||d_{s+k}| + mean|x| * sum_s |d_s|)
The first term is the worst case of any summation order over n rounded
products; the second bounds what the f64 rounding of the mean puts into
partial sums of d.  The mean is held to n * 2^-53 * mean|x|, n exactly.
Lags at or past n have empty sums, so their tolerance is 0: exactly 0.0."""
import functools

import numpy as np
import pytest

import cimba_amd as ca
from cimba_amd import _C, correlogram as cg

LD = np.longdouble
BACKENDS = [False, pytest.param(True, marks=pytest.mark.gpu)]
RAGGED = (0, 1, 17, 299, 300)
# (T, N, maxlag, lengths, skip, row stride)
CASES = (
    # segment and step edges
    [(3, n, lag, None, 0, n) for n in (1, 2, 3, 15, 16, 17, 63, 64, 65)
     for lag in (1, 15, 16, 17)] +
    # chunk edges and halo
    [(3, n, lag, None, 0, n) for n in (2047, 2048, 2049, 5000)
     for lag in (63, 64, 255)] +
    # rows long enough for the sixteen-wave mean kernel (16384 and up)
    [(3, 16383, 16, None, 0, 16383), (3, 16384, 16, None, 0, 16384),
     (3, 16500, 15, (0, 100, 16500), 16, 16500)] +
    # more lags than data
    [(3, 17, 64, None, 0, 17), (3, 3, 255, None, 0, 3)] +
    # ragged and skip (skip 20 empties the rows of length 0, 1 and 17)
    [(5, 300, 64, RAGGED, skip, 300) for skip in (0, 16, 20)] +
    # non-contiguous input: a [T, N] view of wider rows
    [(3, 2049, 17, None, 0, 2100), (5, 300, 16, RAGGED, 16, 333)])


@functools.lru_cache(maxsize=None)
def ar1(T, width):
    """AR(1), rho = 0.9, offset +10, so the mean matters.  Read-only."""
    rng = np.random.default_rng(1000 * T + width)
    e = rng.standard_normal((T, width))
    x = np.empty((T, width))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - 0.81)
    for s in range(1, width):
        x[:, s] = 0.9 * x[:, s - 1] + e[:, s]
    x += 10.0
    x.setflags(write=False)
    return x


def reference(x, maxlag, lengths=None, skip=0):
    """n, mean, c, tol_mean, tol_c in longdouble, from the definition."""
    T, N = x.shape
    n = np.zeros(T)
    mean = np.full(T, np.nan, dtype=LD)
    tol_mean = np.zeros(T, dtype=LD)
    c = np.zeros((T, maxlag + 1), dtype=LD)
    tol = np.zeros((T, maxlag + 1), dtype=LD)
    for t in range(T):
        xs = x[t, skip:N if lengths is None else min(lengths[t], N)].astype(LD)
        n[t] = m = len(xs)
        if m == 0:
            continue
        mean[t] = xs.sum() / m
        d = xs - mean[t]
        absx = np.abs(xs).sum() / m
        tol_mean[t] = m * LD(2.0) ** -53 * absx
        for k in range(min(maxlag + 1, m)):
            c[t, k] = (d[:m - k] * d[k:]).sum()
            tol[t, k] = m * LD(2.0) ** -52 * (
                (np.abs(d[:m - k]) * np.abs(d[k:])).sum() +
                absx * np.abs(d).sum())
    return n, mean, c, tol_mean, tol


@functools.lru_cache(maxsize=None)
def case_ref(case):
    T, N, maxlag, lengths, skip, stride = case
    return reference(ar1(T, stride)[:, :N], maxlag, lengths, skip)


def check(res, ref):
    n, mean, c, tol_mean, tol = ref
    assert np.array_equal(res["n"], n)
    empty = n == 0
    assert np.all(np.isnan(res["mean"][empty]))
    assert np.all(np.abs(res["mean"].astype(LD) - mean)[~empty]
                  <= tol_mean[~empty])
    err = np.abs(res["c"].astype(LD) - c)
    assert np.all(err <= tol), (float((err / np.maximum(tol, LD(1e-300))).max()),
                                np.argwhere(err > tol)[:4].tolist())


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-N%d-L%d-%s-skip%d-"
                         "stride%d" % (c[0], c[1], c[2], "ragged" if c[3]
                                       else "full", c[4], c[5]))
def test_lag_sums(case, gpu):
    T, N, maxlag, lengths, skip, stride = case
    x = ar1(T, stride)[:, :N]
    res = cg.lag_sums(x, maxlag, lengths=lengths, skip=skip, gpu=gpu)
    assert res["c"].shape == (T, maxlag + 1)
    check(res, case_ref(case))


@pytest.mark.parametrize("gpu", BACKENDS)
@pytest.mark.parametrize("view", ["transposed", "reversed"])
def test_lag_sums_copied_view(view, gpu):
    """Views that cannot be read in place (columns not adjacent, rows in
    descending order) are copied to a dense array first."""
    x = ar1(3, 300)
    v = np.asfortranarray(x) if view == "transposed" else x[::-1]
    assert v.strides[1] != 8 or v.strides[0] < 0
    check(cg.lag_sums(v, 17, skip=3, gpu=gpu), reference(v, 17, skip=3))


@pytest.mark.parametrize("gpu", BACKENDS)
def test_bad_arguments_then_valid(gpu):
    x = ar1(3, 17)
    for series, maxlag in ((x, 0), (x, 256), (x[:0], 4)):
        with pytest.raises(ValueError):
            cg.lag_sums(series, maxlag, gpu=gpu)
    check(cg.lag_sums(x, 4, gpu=gpu), reference(x, 4))


@pytest.mark.gpu
def test_gpu_deterministic():
    x = ar1(3, 5000)
    a, b = (cg.lag_sums(x, 255, gpu=True) for _ in range(2))
    for key in ("n", "mean", "c"):
        assert a[key].tobytes() == b[key].tobytes()


@pytest.mark.gpu
def test_gpu_log_to_correlogram():
    r = ca.mm1log_gpu(ntrials=4, num_objects=300, seed=7, log_count=4,
                      log_capacity=1024)
    assert r["log_emitted"].max() <= 1024  # the ring lost nothing
    x, lengths = cg.series_from_log(r, _C.LC_DEPART)
    assert x.shape == (4, 300) and list(lengths) == [300] * 4
    g = cg.lag_sums(x, 32, lengths=lengths, skip=20, gpu=True)
    h = cg.lag_sums(x, 32, lengths=lengths, skip=20, gpu=False)
    tol = reference(x, 32, lengths, 20)[4]
    assert np.array_equal(g["n"], h["n"])
    assert np.all(np.abs(g["c"].astype(LD) - h["c"].astype(LD)) <= tol)
    assert cg.pooled_acf(g)[0] > 0.0


def test_acf_pacf_match_dataset():
    x = ar1(3, 300)[:1]
    ds = _C.Dataset()
    for v in x[0]:
        ds.add(v)
    res = cg.lag_sums(x, 20, gpu=False)
    _, _, c, _, tol = reference(x, 20)
    # both sides hold c_k within tol_k and c_0 within tol_0, and |r_k| <= 1,
    # so their quotients differ by at most 2 (tol_k + tol_0) / c_0
    bound = 2 * (tol[0, 1:] + tol[0, 0]) / c[0, 0]
    r = cg.acf(res)
    assert r.shape == (1, 20)
    assert np.all(np.abs(r[0] - np.array(ds.acf(20))) <= bound)
    assert abs(cg.pooled_acf(res)[0] - r[0, 0]) <= bound[0]
    assert list(_C.pacf_from_acf(ds.acf(20))) == list(ds.pacf(20))
    assert cg.pacf(r).shape == (1, 20)
    assert cg.inflation([0.5, 0.25, -0.1, 0.9]) == 2.5
    assert not cg.acf({"c": np.zeros((2, 4))}).any()


def test_series_from_log():
    rows = [  # (trial, seq, code, vtype, value); window = trials 5, 6, 7
        (5, 0, 1, 0, 0), (5, 1, 3, 2, 1.5), (5, 2, 2, 1, 0), (5, 3, 3, 2, 2.5),
        (5, 4, 3, 2, -3.5), (6, 0, 1, 0, 1), (6, 1, 2, 1, 0),
        (7, 0, 3, 2, 8.0), (7, 1, 1, 0, 2), (7, 2, 3, 2, 9.0)]
    rec = np.zeros(len(rows), dtype=[("trial", "u8"), ("seq", "u4"),
                                     ("code", "u2"), ("vtype", "u1"),
                                     ("value", "u8")])
    for o, (trial, seq, code, vtype, value) in zip(rec, rows):
        bits = np.float64(value).view(np.uint64) if vtype == 2 else value
        o["trial"], o["seq"], o["code"], o["vtype"], o["value"] = (
            trial, seq, code, vtype, bits)
    result = {"log_records": rec, "log_first": 5,
              "log_emitted": np.array([5, 2, 3], dtype=np.uint32)}
    x, lengths = cg.series_from_log(result, 3)
    assert lengths.dtype == np.uint32 and list(lengths) == [3, 0, 2]
    assert x.tolist() == [[1.5, 2.5, -3.5], [0, 0, 0], [8.0, 9.0, 0]]
    with pytest.raises(ValueError):
        cg.series_from_log(result, 1)
    # trial 7 emitted more than its ring kept: a truncated series is refused
    result["log_emitted"] = np.array([5, 2, 9], dtype=np.uint32)
    with pytest.raises(ValueError, match="lost records"):
        cg.series_from_log(result, 3)
