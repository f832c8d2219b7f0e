"""Timing of timeseries.time_batches against the host path and against the
memory traffic it needs (profiles/r18_time_batches.md).

    python scripts/timebatch_perf.py [--reps 5] [--small]

Shapes (T, N, K): 65 536 x 2 000 with K = 64 (dense: 31 samples per batch),
65 536 x 64 with K = 2 000 (sparse: 31 batches per sample) and 64 x 2^20
with K = 1 024 (long rows).  All take the block tier.  Per row of output:

    kernel_ms   device events around the kernel alone (elapsed_ms)
    call_ms     wall clock of the whole call: upload, kernel, download
    host_ms     the same call with gpu=False, elapsed_ms of the host loop
    gb_per_s    bytes the algorithm needs (16 per sample read, 24 per batch
                written) over the median kernel time
    hbm_share   gb_per_s over the bandwidth of a device-to-device copy of
                1 GiB measured in the same process (copy_gb_per_s)
    differ      largest |gpu - host| of the means over max(|host|, 1)

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
from cimba_amd import timeseries  # noqa: E402


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4),
            "max": round(v[-1], 4)}


def copy_bandwidth():
    """GB/s of a device-to-device copy (read plus write) of 1 GiB."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")  # the runtime the extension loaded
    size, d2d = ctypes.c_size_t(1 << 30), 3  # hipMemcpyDeviceToDevice
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()

    def ok(rc):
        if rc != 0:
            raise SystemExit(f"timebatch_perf: hip error {rc}")

    ok(hip.hipMalloc(ctypes.byref(src), size))
    ok(hip.hipMalloc(ctypes.byref(dst), size))
    ok(hip.hipMemset(src, 1, size))
    t = []
    for _ in range(6):  # the first is the warm-up
        ok(hip.hipDeviceSynchronize())
        t0 = time.perf_counter()
        ok(hip.hipMemcpy(dst, src, size, d2d))
        ok(hip.hipDeviceSynchronize())
        t.append(time.perf_counter() - t0)
    ok(hip.hipFree(src))
    ok(hip.hipFree(dst))
    return 2.0 * (1 << 30) / 1e9 / sorted(t[1:])[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1/16 of the data")
    a = ap.parse_args()
    if not ca.has_gpu():
        raise SystemExit("timebatch_perf: no HIP device visible")
    hbm = copy_bandwidth()
    div = 16 if a.small else 1
    for T, N, K in ((65536 // div, 2000, 64), (65536 // div, 64, 2000),
                    (64, (1 << 20) // div, 1024)):
        rng = np.random.default_rng(7)
        x = np.cumsum(rng.integers(-1, 2, (T, N)), axis=1).astype(np.float64)
        t = np.cumsum(rng.exponential(1.0, (T, N)), axis=1)
        end = float(t[:, -1].min())

        def fn(gpu):
            return timeseries.time_batches(x, t, end, K, gpu=gpu)

        fn(True)  # warm-up: code object, allocator
        kernel, call = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            g = fn(True)
            call.append((time.perf_counter() - t0) * 1e3)
            kernel.append(g["elapsed_ms"])
        h = fn(False)
        kernel, call = spread(kernel), spread(call)
        rate = (16.0 * T * N + 24.0 * T * K) / 1e9 / (kernel["median"] * 1e-3)
        print(json.dumps({
            "T": T, "N": N, "K": K, "kernel_ms": kernel, "call_ms": call,
            "host_ms": round(h["elapsed_ms"], 2), "gb_per_s": round(rate, 1),
            "copy_gb_per_s": round(hbm, 1), "hbm_share": round(rate / hbm, 4),
            "differ": float(np.nanmax(
                np.abs(g["means"] - h["means"]) /
                np.maximum(np.abs(h["means"]), 1.0)))}), flush=True)


if __name__ == "__main__":
    main()
