"""Steady-state output analysis of many series at once: where the warm-up
ends (MSER-m) and how precise the mean is (batch means).

Both take a dense ``[T, N]`` float64 array, one row per trial.  Row ``r`` is
``series[r, skip_r : min(lengths[r], N)]``, ``n_r`` values; ``skip`` is one
number or one per row, so the ``cut`` that ``mser`` finds can be handed to
``batch_means`` (and, per group of rows, to ``lag_sums``) as ``skip``.

Batch means of size ``m``: ``k = n_r // m`` of them, trailing observations
dropped, ``y_j = (x_{jm} + ... + x_{jm+m-1}) / m`` summed left to right.
Level ``l + 1`` of the doubling ladder halves the count and averages
neighbours, ``(y_{2j} + y_{2j+1}) / 2``; level ``l`` has batches of
``m * 2**l``.  Every batch mean has the same bits on the host and the GPU.

On a GPU a row is walked in chunks of ``_C.SSTAT_CHUNK`` batch means with a
few doubles of carried state, so there is no longest row: one wave per row
up to ``_C.SSTAT_WAVE_MAX`` observations (``N``), a workgroup per row beyond.
Without a GPU, sequential loops per row.  The two add in different orders,
so sums agree to rounding, not to the bit.

From a launch to the standard error of the steady-state mean:

    r = cimba_amd.mm1log_gpu(ntrials=1024, num_objects=2000, seed=7,
                             log_count=1024, log_capacity=8192)
    x, lengths = correlogram.series_from_log(r, _C.LC_DEPART)
    cut = steadystate.mser(x, m=5, lengths=lengths)["cut"]
    res = steadystate.batch_means(x, 5, levels=6, lengths=lengths, skip=cut)
    se, r1 = steadystate.stderr(res), steadystate.lag1(res)

and read ``se`` at the first level whose ``r1`` is no longer clearly
positive.
"""
import numpy as np

from . import _C


def _on_gpu(gpu):
    if gpu is None:
        from . import has_gpu
        gpu = has_gpu()
    return gpu


def mser(series, m=5, lengths=None, skip=0, want_curve=False, gpu=None,
         device=0):
    """MSER-m truncation (White and Spratt) per row, as a dict with the
    ``elapsed_ms`` of the computation alone.

    Over the batch means ``y_0..y_{k-1}`` and ``d = 0..k // 2``,
    ``stat(d) = sum_{j>=d} (y_j - ybar_d)^2 / (k - d)^2``.  ``d`` is the
    smallest minimiser among the ``stat(d)`` that are not NaN, ``stat`` and
    ``mean`` are ``stat(d)`` and ``ybar_d``; with no such ``d`` (``k == 0``,
    a NaN in the second half) ``d`` is 0 and both are NaN.  ``cut`` is
    ``skip_r + d * m``, the observation at which steady state starts.
    ``n``, ``k``, ``d`` and ``cut`` are uint32, ``stat`` and ``mean``
    float64; ``want_curve`` adds ``curve``, float64 ``[T, N // (2 m) + 1]``
    with ``stat(d)`` and NaN past ``k // 2``.  ``gpu=None`` picks the GPU
    when one is visible."""
    if _on_gpu(gpu):
        return _C.mser_gpu(series, m=m, lengths=lengths, skip=skip,
                           want_curve=want_curve, device=device)
    return _C.mser_host(series, m=m, lengths=lengths, skip=skip,
                        want_curve=want_curve)


def batch_means(series, batch, levels=1, lengths=None, skip=0, gpu=None,
                device=0):
    """Sums over the batch means of every level ``l < levels`` of the
    doubling ladder (``1 <= levels <= 16``), float64 ``[T, levels]`` each:
    ``k`` their count, ``mean``, ``sse = sum (y_j - mean)^2``,
    ``c1 = sum (y_j - mean)(y_{j+1} - mean)`` and
    ``dsq = sum (y_{j+1} - y_j)^2``, von Neumann's numerator, summed on its
    own: from ``sse``, ``c1`` and the end terms it would cancel for just the
    correlated series it is used on.  A level with ``k == 0`` has a NaN
    mean and sums of 0.0.  Level ``l`` has batches of ``batch * 2**l``.
    The dict also carries the ``elapsed_ms`` of the computation alone."""
    if _on_gpu(gpu):
        return _C.batch_means_gpu(series, batch, levels=levels,
                                  lengths=lengths, skip=skip, device=device)
    return _C.batch_means_host(series, batch, levels=levels, lengths=lengths,
                               skip=skip)


def variance(result):
    """Sample variance of the batch means, ``sse / (k - 1)``; NaN for
    ``k < 2``."""
    k = result["k"]
    ok = k >= 2
    return np.where(ok, result["sse"] / np.where(ok, k - 1.0, 1.0), np.nan)


def stderr(result):
    """Standard error of the row's mean from each level's batch means,
    ``sqrt(variance / k)``.  A half-width is this times a Student-t quantile
    with ``k - 1`` degrees of freedom, which is left to the caller."""
    k = result["k"]
    return np.sqrt(variance(result) / np.where(k >= 2, k, 1.0))


def lag1(result):
    """Lag-1 autocorrelation of the batch means, ``c1 / sse``; 0.0 where
    ``sse <= 0``, as ``correlogram.acf``."""
    sse = result["sse"]
    ok = sse > 0.0
    return np.where(ok, result["c1"] / np.where(ok, sse, 1.0), 0.0)


def von_neumann(result):
    """Von Neumann's ratio ``sum (y_{j+1} - y_j)^2 / sse`` (about 2 for
    uncorrelated batch means); 0.0 where ``sse <= 0``."""
    sse = result["sse"]
    ok = sse > 0.0
    return np.where(ok, result["dsq"] / np.where(ok, sse, 1.0), 0.0)
