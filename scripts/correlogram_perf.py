"""Timing of the correlogram kernels against the host loops
(profiles/r11_correlogram.md).

    python scripts/correlogram_perf.py [--reps 5] [--no-host] [--small]

Two shapes at 64 lags: 65 536 series of 2 000 observations (one launch of
M/M/1 replications) and 20 series of 10^6 (long single runs), then the
same arrays at 63 / 64 / 127 / 255 lags, which walk the MB = 5 / 6 / 9 / 17
tiers of the lag kernel.  GPU times are the kernels alone (device events);
uploads and downloads are not in them.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cimba_amd as ca  # noqa: E402
from cimba_amd import correlogram as cg  # noqa: E402


def ar1(T, N, seed):
    """AR(1), rho = 0.9, offset +10."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, T))
    x[0] /= np.sqrt(1.0 - 0.81)
    for s in range(1, N):
        x[s] += 0.9 * x[s - 1]
    return np.ascontiguousarray(x.T) + 10.0


def mb_tier(maxlag):
    """The lag kernel's accumulator tiles (cmb::corr::mb_tier)."""
    for top, mb in ((15, 2), (63, 5), (79, 6), (127, 9)):
        if maxlag <= top:
            return mb
    return 17


def work(T, N, maxlag):
    """Operations and bytes the blocked algorithm needs, from the shapes:
    one 16x16x4 f64 MFMA is 2048 flop and one 512-byte LDS operand read;
    the rows are read twice (mean, lag sums)."""
    chunks = -(-N // 2048)
    steps = sum(-(-min(2048, N - 2048 * c) // 64) for c in range(chunks))
    mfma = T * steps * mb_tier(maxlag)
    partial = T * chunks * (maxlag + 1) * 8
    return {"mb": mb_tier(maxlag), "mfma_gflop": mfma * 2048 / 1e9,
            "lds_read_gb": mfma * 512 / 1e9,
            "hbm_gb": (2 * T * N * 8 + (2 * partial if chunks > 1
                                        else partial)) / 1e9}


def time_gpu(x, maxlag, reps):
    cg.lag_sums(x, maxlag, gpu=True)  # warm-up: code object, allocator
    ms = sorted(cg.lag_sums(x, maxlag, gpu=True)["elapsed_ms"]
                for _ in range(reps))
    return {"min_ms": ms[0], "median_ms": ms[len(ms) // 2], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--small", action="store_true",
                    help="1/16 of the trials and of the long rows")
    a = ap.parse_args()
    if not ca.has_gpu():
        raise SystemExit("correlogram_perf: no HIP device visible")
    div = 16 if a.small else 1
    for name, T, N in (("launch", 65536 // div, 2000),
                       ("long", 20, 1000000 // div)):
        x = ar1(T, N, 7)
        for maxlag in (64, 63, 127, 255):
            row = {"shape": name, "T": T, "N": N, "maxlag": maxlag,
                   **work(T, N, maxlag), **time_gpu(x, maxlag, a.reps)}
            if maxlag == 64 and not a.no_host:
                g = cg.lag_sums(x, maxlag, gpu=True)
                h = cg.lag_sums(x, maxlag, gpu=False)
                row["host_ms"] = h["elapsed_ms"]
                row["host_over_gpu"] = h["elapsed_ms"] / row["median_ms"]
                row["max_rel_diff_c0"] = float(np.max(
                    np.abs(g["c"][:, 0] - h["c"][:, 0]) / h["c"][:, 0]))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
