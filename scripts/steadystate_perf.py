"""Timing of the MSER cut and the batch-means ladder against the host path
and against numpy (profiles/r15_steadystate.md).

    python scripts/steadystate_perf.py [--reps 5] [--base-reps 2] [--small]

Shapes: 65 536 x 2 000 (wave tier), then 64 x 1 000 000 and 8 x 8 000 000
(block tier).  Each for mser(m=5) and batch_means(batch=5, levels=8).  Per
row of output:

    kernel_ms   device events around the kernel alone (elapsed_ms)
    call_ms     wall clock of the whole call: upload, kernel, download
    host_ms     the same call with gpu=False, elapsed_ms of the host loops
    numpy_ms    the obvious numpy formulation: reshape-mean for the batch
                means, reversed cumulative sums of y and y^2 for the MSER
                curve, one two-pass sum per level for the ladder
    gb_per_s    bytes the algorithm needs (every observation of complete
                batches once, 8 T k m) over the median kernel time
    hbm_share   gb_per_s over the 8 000 GB/s an MI355X is specified for
    differ      rows whose d differs from the host's (MSER), or the largest
                relative difference of sse against the host's (ladder)

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
from cimba_amd import _C, steadystate  # noqa: E402

M, LEVELS = 5, 8
HBM_GB_S = 8000.0


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


def numpy_mser(x):
    T, N = x.shape
    k = N // M
    y = x[:, :k * M].reshape(T, k, M).mean(axis=2)
    c = (k - np.arange(k // 2 + 1)).astype(np.float64)
    s1 = np.cumsum(y[:, ::-1], axis=1)[:, ::-1][:, :k // 2 + 1]
    s2 = np.cumsum((y * y)[:, ::-1], axis=1)[:, ::-1][:, :k // 2 + 1]
    return np.argmin((s2 - s1 * s1 / c) / (c * c), axis=1)


def numpy_ladder(x):
    T, N = x.shape
    k = N // M
    y = x[:, :k * M].reshape(T, k, M).mean(axis=2)
    out = []
    for _ in range(LEVELS):
        d = y - y.mean(axis=1, keepdims=True)
        out.append(((d * d).sum(axis=1), (d[:, :-1] * d[:, 1:]).sum(axis=1)))
        y = (y[:, 0:y.shape[1] // 2 * 2:2] + y[:, 1::2]) / 2
    return out


def wall(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return spread(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-reps", type=int, default=2,
                    help="repetitions of the host and numpy baselines")
    ap.add_argument("--small", action="store_true", help="1/16 of the data")
    a = ap.parse_args()
    if not ca.has_gpu():
        raise SystemExit("steadystate_perf: no HIP device visible")
    div = 16 if a.small else 1
    for T, N in ((65536 // div, 2000), (64, 1000000 // div),
                 (8, 8000000 // div)):
        rng = np.random.default_rng(7)
        x = rng.standard_normal((T, N))
        x += 10.0 + 8.0 * np.exp(-np.arange(N) / 50.0)
        gbytes = 8.0 * T * (N // M * M) / 1e9
        calls = {
            "mser": (lambda gpu: steadystate.mser(x, M, gpu=gpu), numpy_mser),
            "batch_means": (lambda gpu: steadystate.batch_means(
                x, M, levels=LEVELS, gpu=gpu), numpy_ladder)}
        for name, (fn, base) in calls.items():
            kernel, call, g = timed(lambda: fn(True), a.reps)
            host = []
            for _ in range(a.base_reps):
                h = fn(False)
                host.append(h["elapsed_ms"])
            if name == "mser":
                differ = int((g["d"] != h["d"]).sum())
            else:
                differ = float(np.max(np.abs(g["sse"] - h["sse"]) / h["sse"]))
            rate = gbytes / (kernel["median"] * 1e-3)
            print(json.dumps({
                "what": name, "T": T, "N": N,
                "tier": "wave" if N <= _C.SSTAT_WAVE_MAX else "block",
                "kernel_ms": kernel, "call_ms": call,
                "host_ms": spread(host),
                "numpy_ms": wall(lambda: base(x), a.base_reps),
                "gb_per_s": round(rate, 1),
                "hbm_share": round(rate / HBM_GB_S, 4),
                "differ": differ}), flush=True)


if __name__ == "__main__":
    main()
