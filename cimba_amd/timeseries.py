"""Time-weighted order statistics of many state histories at once:
quantiles, median, five-number summary and time-in-state histogram.

Number in system, queue length, units in use, buffer level: piecewise-
constant histories, where an observation counts for as long as it held.
``time_stats`` takes values ``[T, N]`` and the times ``[T, N]`` at which they
were taken (non-decreasing along a row), one row per trial, and a window
``[start_time, end_time]`` per row or for all rows.  Sample ``i`` of a row
of ``m = min(lengths[r], N)`` samples holds from ``max(t_i, start)`` to
``min(t_{i+1}, end)`` (the last one to ``end``); it is kept iff that
duration is positive, which drops zero durations, NaN times (with the
sample before them) and everything outside the window.  ``start_time`` is
the warm-up cut, by time.

Kept (value, duration) pairs are sorted (``-0.0`` before ``+0.0``, NaN
values last, ties by duration) and ``cum`` is the running sum of sorted
durations.  The quantile for ``q`` is the value of the first pair with
``cum >= q * total``: no interpolation, a history takes only the values it
took; ``q = 0.5`` is ``Timeseries.median``.  ``hist`` is the time spent in
each of ``nbins`` equal-width bins over the row's own [min, max].

On a GPU one launch loads a row, builds the weights, sorts the pairs in a
bitonic network, scans the weights and selects the quantiles: one wave per
row in registers up to ``_C.TSTAT_WAVE_MAX`` samples, one workgroup per row
in LDS up to ``_C.TSTAT_BLOCK_MAX``; longer rows are host only.  Without a
GPU, ``std::sort`` and a sequential sum per row.  The GPU sums in another
order.  When every partial sum of durations is exact in double both paths
give identical bits.  Otherwise they may differ in which of two
neighbouring order statistics is picked when ``cum`` lies within rounding
of ``q * total``, and in the last bits of ``total``, ``cum`` and ``hist``.

From a launch to the time-weighted five-number summary of number in system:

    r = cimba_amd.mm1log_gpu(ntrials=1024, num_objects=2000, seed=7,
                             log_count=1024, log_capacity=8192)
    level, t, lengths = timeseries.level_from_log(r, _C.LC_ARRIVE,
                                                  _C.LC_DEPART)
    end = t[np.arange(len(t)), lengths - 1]
    five = timeseries.fivenum(level, t, end, lengths=lengths)

``time_batches`` is the bridge to everything that takes an equally spaced
series.  It cuts each row's window into ``nbatches`` equal intervals
(``width = (end - start) / nbatches``, edge ``j`` at ``start + j * width``,
the last one at ``end``) and averages the history over each: ``integral``
is the sum of value times overlap over the samples that overlap the
interval, ``covered`` the sum of the overlaps and ``means`` their quotient,
NaN where nothing is covered (before the first sample).  A row whose window
is empty or not finite has zero integrals, NaN means and a NaN width.  On a
GPU the samples and the grid edges of a row are merged and the steps of the
merge, not the samples or the intervals, are dealt out evenly to the lanes:
one wave per row while ``N + nbatches <= _C.TBATCH_WAVE_MAX``, else one
workgroup per row walking chunks of ``_C.TBATCH_CHUNK`` steps, so rows may
be of any length.  The GPU adds the pieces of an interval in another order
than the host; when every partial sum is exact both give identical bits.

From the same launch to where steady state starts and L with its standard
error, with no loop over trials:

    nis = timeseries.batch_means_of(level, t, end, 256, lengths=lengths)
    cut = steadystate.mser(nis, m=1)["cut"]
    bm = steadystate.batch_means(nis, batch=1, skip=cut)
    L, se = bm["mean"][:, 0], steadystate.stderr(bm)[:, 0]
"""
import numpy as np

from . import _C
from .correlogram import complete_log

FIVENUM_Q = (0.0, 0.25, 0.5, 0.75, 1.0)


def time_stats(values, times, end_time, start_time=-np.inf, q=None, nbins=0,
               want_sorted=False, lengths=None, gpu=None, device=0):
    """Per-row ``n`` (kept samples) and ``total`` (their time) and, each only
    when asked for, ``quantiles`` ``[T, len(q)]``, ``hist`` (float64
    ``[T, nbins]``) and ``values`` and ``cum`` ``[T, N]`` (NaN at and past
    ``n``), as a dict with the ``elapsed_ms`` of the computation alone.

    Every ``q`` lies in [0, 1], at most 64 of them; ``nbins`` is at most
    4096.  A row with nothing kept has ``total`` 0.0, NaN quantiles and a
    zero histogram.  ``gpu=None`` picks the GPU when one is visible and the
    rows fit it; ``gpu=True`` with rows longer than ``_C.TSTAT_BLOCK_MAX``
    is a ValueError."""
    if gpu is None:
        from . import has_gpu
        gpu = has_gpu() and np.shape(values)[-1] <= _C.TSTAT_BLOCK_MAX
    fn = _C.time_stats_gpu if gpu else _C.time_stats_host
    return fn(values, times, end_time, start_time=start_time, q=q,
              nbins=nbins, want_sorted=want_sorted, lengths=lengths,
              device=device)


def quantiles(values, times, end_time, q, **kw):
    """``[T, len(q)]`` time-weighted quantiles."""
    return time_stats(values, times, end_time, q=np.atleast_1d(q),
                      **kw)["quantiles"]


def median(values, times, end_time, **kw):
    """Per-row time-weighted median, ``[T]`` (``Timeseries.median``)."""
    return quantiles(values, times, end_time, (0.5,), **kw)[:, 0]


def fivenum(values, times, end_time, **kw):
    """``[T, 5]``: min, Q1, median, Q3, max by time; NaN for an empty row."""
    return quantiles(values, times, end_time, FIVENUM_Q, **kw)


def histogram(values, times, end_time, nbins, **kw):
    """float64 ``[T, nbins]``: time spent in each equal-width bin over the
    row's own [min, max]."""
    return time_stats(values, times, end_time, nbins=nbins, **kw)["hist"]


def time_batches(values, times, end_time, nbatches, start_time=0.0,
                 lengths=None, gpu=None, device=0):
    """Time averages over ``nbatches`` (1 to 65536) equal intervals of each
    row's window ``[start_time, end_time]``: per-row ``n`` (kept samples, as
    ``time_stats``) and ``width``, and ``integral``, ``covered`` and
    ``means``, float64 ``[T, nbatches]``, as a dict with the ``elapsed_ms``
    of the computation alone.

    ``start_time`` defaults to 0.0, where the clock starts: a grid needs an
    origin.  ``gpu=None`` picks the GPU when one is visible; rows may be of
    any length."""
    if gpu is None:
        from . import has_gpu
        gpu = has_gpu()
    fn = _C.time_batches_gpu if gpu else _C.time_batches_host
    return fn(values, times, end_time, start_time=start_time,
              nbatches=nbatches, lengths=lengths, device=device)


def batch_means_of(values, times, end_time, nbatches, **kw):
    """``[T, nbatches]`` time averages: an equally spaced series for
    ``steadystate.mser``, ``steadystate.batch_means`` and
    ``correlogram.lag_sums``."""
    return time_batches(values, times, end_time, nbatches, **kw)["means"]


def _dense(rec, first, count, columns):
    """Records in ``(trial, seq)`` order to ``[count, n_max]`` arrays, one
    per column, and ``lengths``."""
    row = (rec["trial"] - first).astype(np.int64)
    lengths = np.bincount(row, minlength=count).astype(np.uint32)
    begin = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64)
    col = np.arange(len(rec), dtype=np.int64) - begin[row]
    out = []
    for c in columns:
        a = np.zeros((count, int(lengths.max()) if count else 0))
        a[row, col] = c
        out.append(a)
    return out, lengths


def history_from_log(result, code):
    """``series_from_log`` with the records' times: ``values, times,
    lengths``, both arrays ``[count, n_max]``.  A trial whose log ring
    lost records is a ValueError."""
    rec, count, first = complete_log(result)
    rec = rec[rec["code"] == code]
    if len(rec) and not np.all(rec["vtype"] == _C.LOGV_F64):
        raise ValueError(f"records of code {code} do not carry doubles")
    rec = rec[np.lexsort((rec["seq"], rec["trial"]))]
    (x, t), lengths = _dense(
        rec, first, count,
        (np.ascontiguousarray(rec["value"]).view(np.float64), rec["t"]))
    return x, t, lengths


def level_from_log(result, up_codes, down_codes, initial=0):
    """A running level per trial from the records of ``up_codes`` (+1) and
    ``down_codes`` (-1), merged in ``(trial, seq)`` order, starting at
    ``initial``: ``values, times, lengths``.  With ``LC_ARRIVE`` up and
    ``LC_DEPART`` down this is ``mm1log_gpu``'s number in system.  A trial
    whose log ring lost records is a ValueError."""
    rec, count, first = complete_log(result)
    up = np.isin(rec["code"], np.atleast_1d(up_codes))
    down = np.isin(rec["code"], np.atleast_1d(down_codes))
    step = up.astype(np.int64) - down.astype(np.int64)
    keep = up | down
    rec, step = rec[keep], step[keep]
    order = np.lexsort((rec["seq"], rec["trial"]))
    rec, step = rec[order], step[order]
    row = (rec["trial"] - first).astype(np.int64)
    run = np.cumsum(step)
    n_row = np.bincount(row, minlength=count)
    begin = np.concatenate(([0], np.cumsum(n_row)[:-1])).astype(np.int64)
    before = np.concatenate(([0], run))[begin]  # sum of the rows above
    level = initial + run - before[row]
    (x, t), lengths = _dense(rec, first, count, (level, rec["t"]))
    return x, t, lengths
