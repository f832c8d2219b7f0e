"""Order statistics of many output series at once: sort, quantiles,
five-number summary, histogram.

``order_stats`` takes a dense ``[T, N]`` float64 array, one row per trial,
sorts every row and reads quantiles and an equal-width histogram off the
sorted rows, with the arithmetic of ``Dataset.quantile`` and
``Dataset.histogram``.  On a GPU the sort is a bitonic network on 64-bit
keys in three tiers, picked from the longest possible row: one wave per row
in registers (up to ``_C.OSTAT_WAVE_MAX`` values), one workgroup per row in
LDS (up to ``_C.OSTAT_BLOCK_MAX``), and LDS chunks merged through global
memory beyond that; without one, ``std::sort`` per row.  Both paths give
the same bits.

The order is total: ``-0.0`` before ``+0.0``, every NaN last.  A row that
holds a NaN or an infinity has NaN or infinite upper quantiles by IEEE
arithmetic and an all-zero histogram.

From a launch to a five-number summary per trial:

    r = cimba_amd.mm1log_gpu(ntrials=1024, num_objects=2000, seed=7,
                             log_count=1024, log_capacity=8192)
    x, lengths = correlogram.series_from_log(r, _C.LC_DEPART)
    five = orderstat.fivenum(x, lengths=lengths, skip=200)
"""
import numpy as np

from . import _C

FIVENUM_Q = (0.0, 0.25, 0.5, 0.75, 1.0)


def order_stats(series, q=None, nbins=0, want_sorted=False, lengths=None,
                skip=0, gpu=None, device=0):
    """Per-row ``n`` and, each only when asked for, ``sorted`` ``[T, N]``
    (NaN at and past ``n``), ``quantiles`` ``[T, len(q)]`` and ``hist``
    (int64 ``[T, nbins]``), as a dict with the ``elapsed_ms`` of the
    computation alone.

    The series of row ``t`` is ``series[t, skip:min(lengths[t], N)]``, as
    in ``correlogram.lag_sums``.  Every ``q`` lies in [0, 1], at most 64 of
    them; ``nbins`` is at most 4096.  An empty row has NaN quantiles and a
    zero histogram.  ``gpu=None`` picks the GPU when one is visible."""
    if gpu is None:
        from . import has_gpu
        gpu = has_gpu()
    if gpu:
        return _C.order_stats_gpu(series, q=q, nbins=nbins,
                                  want_sorted=want_sorted, lengths=lengths,
                                  skip=skip, device=device)
    return _C.order_stats_host(series, q=q, nbins=nbins,
                               want_sorted=want_sorted, lengths=lengths,
                               skip=skip)


def sort_rows(series, **kw):
    """Every row ascending, ``[T, N]``; NaN at and past the row's length."""
    return order_stats(series, want_sorted=True, **kw)["sorted"]


def quantiles(series, q, **kw):
    """``[T, len(q)]`` quantiles by linear interpolation between the two
    nearest order statistics (``Dataset.quantile``)."""
    return order_stats(series, q=np.atleast_1d(q), **kw)["quantiles"]


def median(series, **kw):
    """Per-row median, ``[T]``."""
    return quantiles(series, (0.5,), **kw)[:, 0]


def fivenum(series, **kw):
    """``[T, 5]``: min, Q1, median, Q3, max; NaN for an empty row."""
    return quantiles(series, FIVENUM_Q, **kw)


def histogram(series, nbins, **kw):
    """int64 ``[T, nbins]``: equal-width bins over each row's own
    [min, max] (``Dataset.histogram``)."""
    return order_stats(series, nbins=nbins, **kw)["hist"]
