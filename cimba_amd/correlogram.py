"""Correlogram of many output series at once: lag sums, ACF, PACF.

``lag_sums`` takes a dense ``[T, N]`` float64 array, one row per trial,
and returns for every row its effective length ``n``, its ``mean`` and the
centred raw lag sums ``c[t, k] = sum_s (x_s - mean)(x_{s+k} - mean)`` for
``k = 0..maxlag`` -- the definition ``Dataset.acf`` uses (full-series mean,
no 1/n).  On a GPU the sums come from an MFMA kernel, one wave per 2048
observations of a row; without one, from plain host loops.

From a launch to a correlogram:

    r = cimba_amd.mm1log_gpu(ntrials=1024, num_objects=2000, seed=7,
                             log_count=1024, log_capacity=8192)
    x, lengths = correlogram.series_from_log(r, _C.LC_DEPART)
    rho = correlogram.pooled_acf(
        correlogram.lag_sums(x, 64, lengths=lengths, skip=200))
"""
import numpy as np

from . import _C


def lag_sums(series, maxlag, lengths=None, skip=0, gpu=None, device=0):
    """Per-row ``n``, ``mean`` and lag sums ``c[T, maxlag + 1]`` (a dict,
    with the ``elapsed_ms`` of the computation alone).

    ``lengths[t]`` shortens row ``t`` (ragged rows), ``skip`` drops the
    first observations of every row (warm-up): the series of row ``t`` is
    ``series[t, skip:min(lengths[t], N)]``.  Lags at or past ``n`` are 0.0;
    an empty series has a NaN mean.  ``gpu=None`` picks the GPU when one
    is visible."""
    if gpu is None:
        from . import has_gpu
        gpu = has_gpu()
    if gpu:
        return _C.lag_sums_gpu(series, maxlag, lengths=lengths, skip=skip,
                               device=device)
    return _C.lag_sums_host(series, maxlag, lengths=lengths, skip=skip)


def acf(result):
    """Per-row autocorrelations ``r[t, k-1] = c_k / c_0`` for k = 1..L;
    a row with ``c_0 <= 0`` is all zeros, as in ``Dataset.acf``."""
    c = np.asarray(result["c"], dtype=np.float64)
    c0 = c[:, :1]
    ok = c0 > 0.0
    return np.where(ok, c[:, 1:] / np.where(ok, c0, 1.0), 0.0)


def pooled_acf(result):
    """One correlogram for all rows: ``sum_t c_k / sum_t c_0``, k = 1..L
    (zeros when the pooled ``c_0`` is not positive)."""
    c = np.asarray(result["c"], dtype=np.float64).sum(axis=0)
    if not c[0] > 0.0:
        return np.zeros(len(c) - 1)
    return c[1:] / c[0]


def pacf(r):
    """Partial autocorrelations from autocorrelations ``r_1..r_L`` (one
    row, or one per row of a 2-D array) by Durbin-Levinson."""
    r = np.asarray(r, dtype=np.float64)
    if r.ndim == 1:
        return np.asarray(_C.pacf_from_acf(r), dtype=np.float64)
    return np.array([_C.pacf_from_acf(row) for row in r], dtype=np.float64)


def inflation(r):
    """``1 + 2 * sum r_k``, truncated at the first non-positive ``r_k``:
    the factor by which the variance of a mean of correlated observations
    exceeds ``sigma^2 / n``."""
    total = 0.0
    for rk in np.asarray(r, dtype=np.float64):
        if not rk > 0.0:
            break
        total += float(rk)
    return 1.0 + 2.0 * total


def complete_log(result):
    """``log_records``, the number of trials in the log window and its
    first trial; a ValueError when a trial's log ring lost records."""
    rec = result["log_records"]
    emitted = np.asarray(result["log_emitted"], dtype=np.int64)
    count = len(emitted)
    first = np.uint64(result["log_first"])
    kept = np.bincount((rec["trial"] - first).astype(np.int64),
                       minlength=count)
    lost = np.flatnonzero(kept < emitted)
    if len(lost):
        raise ValueError(
            f"the log ring lost records in {len(lost)} trial(s), the first "
            f"at row {lost[0]}: {emitted[lost[0]]} emitted, "
            f"{kept[lost[0]]} kept; use a larger log_capacity")
    return rec, count, first


def series_from_log(result, code):
    """Dense ``[count, n_max]`` float64 array and ``lengths`` (uint32) from
    the ``log_records`` of one record ``code`` with double payloads, in
    ``(trial, seq)`` order.  Row ``i`` is trial ``log_first + i`` of the
    log window; a trial with no such record gets length 0.

    A trial whose log ring overflowed keeps only its most recent records,
    so its row would be a truncated series that looks complete: that is a
    ValueError (run again with a larger ``log_capacity``)."""
    rec, count, first = complete_log(result)
    rec = rec[rec["code"] == code]
    if len(rec) and not np.all(rec["vtype"] == _C.LOGV_F64):
        raise ValueError(f"records of code {code} do not carry doubles")
    rec = rec[np.lexsort((rec["seq"], rec["trial"]))]
    row = (rec["trial"] - first).astype(np.int64)
    lengths = np.bincount(row, minlength=count).astype(np.uint32)
    start = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64)
    col = np.arange(len(rec), dtype=np.int64) - start[row]
    x = np.zeros((count, int(lengths.max()) if count else 0))
    x[row, col] = np.ascontiguousarray(rec["value"]).view(np.float64)
    return x, lengths
