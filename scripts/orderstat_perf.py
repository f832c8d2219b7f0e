"""Timing of the order-statistics kernels against numpy and the host path
(profiles/r13_orderstat.md).

    python scripts/orderstat_perf.py [--reps 5] [--base-reps 2] [--small]

Five shapes, one per regime: 65 536 x 300 (wave tier), 65 536 x 2 000 and
1 024 x 16 384 (block tier: 16 384 only when BLOCK_MAX allows, else chunk),
4 x 2^20 and 1 x 2^24 (chunk tier).  Each is run twice: sorted output only,
and five-number summary only.  Per row of output:

    kernel_ms   device events around the kernels alone (elapsed_ms)
    call_ms     wall clock of the whole call: upload, kernels, download
    npsort_ms   np.sort(x, axis=1) on the same array (sorted-only rows)
    host_ms     order_stats(gpu=False), elapsed_ms of the host loops
    gbs         bytes that must move (keys in, requested output out) over
                kernel_ms

each as min / median / max over the repetitions.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cimba_amd as ca  # noqa: E402
from cimba_amd import _C, orderstat  # noqa: E402

MODES = {"sorted": {"want_sorted": True},
         "fivenum": {"q": orderstat.FIVENUM_Q}}


def tier(N):
    if N <= _C.OSTAT_WAVE_MAX:
        return "wave"
    return "block" if N <= _C.OSTAT_BLOCK_MAX else "chunk"


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4),
            "max": round(v[-1], 4)}


def time_gpu(x, kw, reps):
    orderstat.order_stats(x, gpu=True, **kw)  # warm-up: code object, allocator
    kernel, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = orderstat.order_stats(x, gpu=True, **kw)
        call.append((time.perf_counter() - t0) * 1e3)
        kernel.append(r["elapsed_ms"])
    return spread(kernel), spread(call), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2,
                    help="repetitions of the two host baselines")
    ap.add_argument("--small", action="store_true",
                    help="1/16 of the rows or of the row length")
    a = ap.parse_args()
    if not ca.has_gpu():
        raise SystemExit("orderstat_perf: no HIP device visible")
    div = 16 if a.small else 1
    shapes = ((65536 // div, 300), (65536 // div, 2000), (1024 // div, 16384),
              (4, (1 << 20) // div), (1, (1 << 24) // div))
    for T, N in shapes:
        x = np.random.default_rng(7).standard_normal((T, N))
        for mode, kw in MODES.items():
            kernel, call, g = time_gpu(x, kw, max(a.reps, 5))
            out_bytes = T * N * 8 if mode == "sorted" else T * 5 * 8
            row = {"T": T, "N": N, "tier": tier(N), "mode": mode,
                   "kernel_ms": kernel, "call_ms": call,
                   "gbs": round((T * N * 8 + out_bytes) /
                                (kernel["median"] * 1e6), 1)}
            host = []
            for _ in range(a.base_reps):
                h = orderstat.order_stats(x, gpu=False, **kw)
                host.append(h["elapsed_ms"])
            row["host_ms"] = spread(host)
            key = "sorted" if mode == "sorted" else "quantiles"
            row["equal_host"] = g[key].tobytes() == h[key].tobytes()
            if mode == "sorted":
                ns = []
                for _ in range(a.base_reps):
                    t0 = time.perf_counter()
                    s = np.sort(x, axis=1)
                    ns.append((time.perf_counter() - t0) * 1e3)
                row["npsort_ms"] = spread(ns)
                row["equal_npsort"] = bool(np.array_equal(g["sorted"], s))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
