"""Device tally stream: quantiles and merged moments from a tallied model.

A model that opts in (``Cfg::DEVICE_TALLY = K``) returns, for the trials of
its tally window, ``tally_summaries`` (a structured array ``[count, K]``
with fields ``n, mean, m2, m3, m4, min, max, nan``), ``tally_hist`` (the
pooled histogram, ``uint64[K, 770]``), ``tally_first`` and, on request,
``tally_trial_hist`` (``uint32[count, K, 770]``).  The histogram is
log-binned: 48 octaves from 2^-24 to 2^24 with 16 bins each, so a quantile
read from it is within 1/16 of the true order statistic.

    r = cimba_amd.mm1tally_gpu(ntrials=65536, num_objects=2000, seed=7)
    p50, p90, p99 = (tally.quantile(r["tally_hist"][0], q)
                     for q in (0.5, 0.9, 0.99))
    mean = tally.merged_summary(r, 0).mean()

Aborted trials stay in the pooled histogram and the summaries with what
they observed before the abort; ``trials_ok`` tells whether there were any.
"""
import math

import numpy as np

from . import _C

NBINS = _C.TALLY_NBINS


def edges():
    """The 771 bin edges: bin ``b`` is ``[edges()[b], edges()[b + 1])``.

    Bin 0 reports a lower edge of 0.0 although it also holds every
    negative observation; the last edge is ``+inf``."""
    return _C.tally_edges()


def quantile(hist_row, q):
    """Estimate the ``q`` quantile (0 < q <= 1) from one histogram row.

    The estimate targets the order statistic of rank ``ceil(q * n)`` and
    is linear inside the bin that holds it, so it lies within that bin's
    edges.  Two bins have no finite width to interpolate in: when the
    rank falls into bin 0 (zero, negative or below 2^-24) the result is
    0.0, and when it falls into bin 769 (2^24 and above) the result is
    2^24, a lower bound.  An empty row gives NaN."""
    if not 0.0 < q <= 1.0:
        raise ValueError(f"q must be in (0, 1], got {q!r}")
    h = np.asarray(hist_row, dtype=np.uint64)
    if h.shape != (NBINS,):
        raise ValueError(f"expected one histogram row of {NBINS} bins")
    cum = np.cumsum(h)
    n = int(cum[-1])
    if n == 0:
        return math.nan
    rank = min(max(math.ceil(q * n), 1), n)
    b = int(np.searchsorted(cum, rank, side="left"))
    e = edges()
    if b == 0:
        return 0.0
    if b == NBINS - 1:
        return float(e[b])
    before = int(cum[b - 1])
    frac = (rank - before - 0.5) / int(h[b])
    return float(e[b] + frac * (e[b + 1] - e[b]))


def fivenum(hist_row, summary):
    """(min, lower quartile, median, upper quartile, max) of one tally.

    The quartiles come from the histogram row; the minimum and maximum
    are exact, from ``summary`` (a ``DataSummary``, e.g. from
    ``merged_summary``)."""
    return (summary.minimum(), quantile(hist_row, 0.25),
            quantile(hist_row, 0.5), quantile(hist_row, 0.75),
            summary.maximum())


def merged_summary(result, k):
    """The per-trial summaries of tally ``k`` merged in trial order into
    one ``DataSummary`` (exact pairwise merge)."""
    merged = _C.DataSummary()
    for s in result["tally_summaries"][:, k]:
        merged.merge(_C.DataSummary.from_raw(
            float(s["n"]), float(s["mean"]), float(s["m2"]), float(s["m3"]),
            float(s["m4"]), float(s["min"]), float(s["max"])))
    return merged
