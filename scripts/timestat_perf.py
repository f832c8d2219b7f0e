"""Timing of the time-weighted order statistics against the host path and
against the unweighted sort of orderstat (profiles/r14_timestat.md).

    python scripts/timestat_perf.py [--reps 5] [--base-reps 2] [--small]

Shapes: 65 536 x 300 (wave tier) and 65 536 x 2 000 (block tier, 2048
pairs), then 16 384 x 4 096 and 8 192 x 8 192: the same number of pairs as
two 64 KB workgroups per CU and as one 128 KB workgroup per CU.  Every call
asks for Q and 7 bins.  Per row of output:

    kernel_ms   device events around the kernels alone (elapsed_ms)
    call_ms     wall clock of the whole call: upload, kernels, download
    host_ms     time_stats(gpu=False), elapsed_ms of the host loops
    ostat_ms    orderstat.order_stats(gpu=True) on the same values with the
                same Q and bins: kernel time of the unweighted sort
    ns_per_pair kernel_ms over T * n_pad padded pairs
    q_differ    quantiles that differ from the host path's (the times are
                not on a dyadic grid, so sums round differently)

each time as min / median / max over the repetitions.  Needs a GPU: no
fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cimba_amd as ca  # noqa: E402
from cimba_amd import _C, orderstat, timeseries  # noqa: E402

Q = (0, 0.1, 0.25, 0.5, 0.75, 0.999, 1)
NBINS = 7


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4),
            "max": round(v[-1], 4)}


def timed(fn, reps):
    fn()  # warm-up: code object, allocator
    kernel, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        call.append((time.perf_counter() - t0) * 1e3)
        kernel.append(r["elapsed_ms"])
    return spread(kernel), spread(call), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2,
                    help="repetitions of the host baseline")
    ap.add_argument("--small", action="store_true", help="1/16 of the rows")
    a = ap.parse_args()
    if not ca.has_gpu():
        raise SystemExit("timestat_perf: no HIP device visible")
    div = 16 if a.small else 1
    B = _C.TSTAT_BLOCK_MAX
    shapes = [(65536 // div, 300), (65536 // div, 2000),
              (16384 // div, 4096), (8192 // div, 8192)]
    for T, N in shapes:
        if N > B:
            continue
        rng = np.random.default_rng(7)
        x = rng.integers(0, 12, (T, N)).astype(np.float64)
        t = np.cumsum(rng.exponential(1.0, (T, N)), axis=1)
        end = t[:, -1] + 1.0
        n_pad = 64
        while n_pad < N:
            n_pad *= 2
        kernel, call, g = timed(lambda: timeseries.time_stats(
            x, t, end, q=Q, nbins=NBINS, gpu=True), a.reps)
        okernel, ocall, _ = timed(lambda: orderstat.order_stats(
            x, q=Q, nbins=NBINS, gpu=True), a.reps)
        host = []
        for _ in range(a.base_reps):
            h = timeseries.time_stats(x, t, end, q=Q, nbins=NBINS, gpu=False)
            host.append(h["elapsed_ms"])
        same = (g["quantiles"] == h["quantiles"]) | (
            np.isnan(g["quantiles"]) & np.isnan(h["quantiles"]))
        print(json.dumps({
            "T": T, "N": N, "n_pad": n_pad,
            "tier": "wave" if N <= _C.TSTAT_WAVE_MAX else "block",
            "kernel_ms": kernel, "call_ms": call, "host_ms": spread(host),
            "ostat_ms": okernel, "ostat_call_ms": ocall,
            "ns_per_pair": round(kernel["median"] * 1e6 / (T * n_pad), 4),
            "weight_cost": round(kernel["median"] / okernel["median"], 3),
            "q_differ": int((~same).sum()),
            "total_rel_diff": float(np.max(np.abs(
                g["total"] - h["total"]) / h["total"]))}), flush=True)


if __name__ == "__main__":
    main()
