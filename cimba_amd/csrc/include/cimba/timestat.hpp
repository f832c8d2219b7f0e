// Time-weighted order statistics of piecewise-constant state histories,
// shared by the host and the GPU path (hip/timestat_kernel.hip): the weight
// of a sample, the order on (value, weight) pairs, quantile selection by
// cumulative weight, the time-in-state histogram, the tier constants of the
// kernels and the plain host path.  The batched form of Timeseries::median
// (dataset.hpp).
//
// Row r of x[T][stride] and t[T][stride] holds m = min(len[r], N) samples
// (len may be null).  Sample i holds from a = max(t_i, start_r) to
// b = min(i + 1 < m ? t_{i+1} : end_r, end_r), both NaN when either operand
// is; it is kept iff its weight b - a is positive.  So a NaN time drops its
// own sample and the one before it, whose duration it leaves unknown.
//
// Kept pairs are ordered by (key_of(x), weight) and cum_k is the running sum
// of the sorted weights.  A quantile is the value of the first pair with
// cum_k >= q * total: no interpolation, a state history takes only the
// values it took.
#pragma once

#include "orderstat.hpp"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace cmb {
namespace tstat {

// Longest padded row of the wave tier (one wave, eight pairs per lane) and
// of the block tier (one workgroup, the row's pairs resident in 128 KB of
// LDS).  Longer rows are served by the host path only.
constexpr uint32_t WAVE_MAX = 512;
constexpr uint32_t BLOCK_MAX = 8192;
// Weight bits of padding slots and dropped samples.  With KEY_PAD as the
// key the pair sorts after every kept pair, a kept NaN value included: a
// kept weight is a positive double, and those order as their bits do.
constexpr uint64_t W_PAD = ~0ull;

CMB_INLINE double quiet_nan() { return u64_as_double(0x7ff8000000000000ull); }

// Duration of a sample at time ti whose successor (or the row's end) is at
// time nx, inside the window [start, end].  NaN when any of them is.
CMB_INLINE double sample_weight(double ti, double nx, double start,
                                double end) {
    const double a = ti < start ? start : ti;
    const double b = nx > end ? end : nx;
    return (start != start || end != end) ? quiet_nan() : b - a;
}

CMB_INLINE bool pair_less(uint64_t ka, uint64_t wa, uint64_t kb, uint64_t wb) {
    return ka < kb || (ka == kb && wa < wb);
}

inline bool args_ok(uint64_t T, uint64_t N, uint64_t stride, const double* q,
                    uint32_t nq, uint32_t nbins) {
    return ostat::args_ok(T, N, stride, q, nq, nbins);
}

// The GPU path: the row fits the block tier and T padded rows the workspace.
inline bool grid_ok(uint64_t T, uint64_t N) {
    return N <= BLOCK_MAX && ostat::grid_ok(T, N, 0);
}

// Value of the first of n sorted pairs whose cumulative weight reaches
// q * total (one rounded multiply); NaN when none does (an empty row).
CMB_INLINE double quantile_cum(const double* vals, const double* cum,
                               uint64_t n, double total, double q) {
    const double target = q * total;
    for (uint64_t k = 0; k < n; ++k)
        if (cum[k] >= target) return vals[k];
    return quiet_nan();
}

// cumulative weight of the first i sorted pairs
CMB_INLINE double cum_before(const double* cum, uint64_t i) {
    return i ? cum[i - 1] : 0.0;
}

// first index in [0, n) whose bin exceeds b, n if none
CMB_INLINE uint64_t first_above(const double* xs, uint64_t n, double lo,
                                double w, uint32_t nbins, uint32_t b) {
    uint64_t a = 0, z = n;
    while (a < z) {
        const uint64_t mid = a + (z - a) / 2;
        if (ostat::hist_bin(xs[mid], lo, w, nbins) > b)
            z = mid;
        else
            a = mid + 1;
    }
    return a;
}

// Time spent in bin b of nbins equal-width bins over [vals[0], vals[n-1]]:
// the difference of cum at the bin's two boundaries in the sorted row.
CMB_INLINE double hist_time(const double* vals, const double* cum, uint64_t n,
                            uint32_t nbins, uint32_t b) {
    if (!ostat::hist_row_ok(vals, n)) return 0.0;
    const double lo = vals[0];
    const double w = ostat::hist_width(lo, vals[n - 1], nbins);
    const uint64_t hi_edge = first_above(vals, n, lo, w, nbins, b);
    const uint64_t lo_edge = b ? first_above(vals, n, lo, w, nbins, b - 1) : 0;
    return cum_before(cum, hi_edge) - cum_before(cum, lo_edge);
}

// std::sort on pairs per row, a sequential running sum, then the functions
// above.  n_out[T], total_out[T]; quant_out[T][nq], hist_out[T][nbins],
// vals_out[T][N] and cum_out[T][N] (NaN at and past n_r) may each be null.
// Returns 0, or -1 on bad arguments.
inline int time_stats_host(const double* x, const double* t, uint64_t T,
                           uint64_t N, uint64_t stride, const uint32_t* len,
                           const double* start, const double* end,
                           const double* q, uint32_t nq, uint32_t nbins,
                           double* n_out, double* total_out, double* quant_out,
                           double* hist_out, double* vals_out,
                           double* cum_out) {
    if (!args_ok(T, N, stride, q, nq, nbins)) return -1;
    std::vector<std::pair<uint64_t, uint64_t>> pairs;
    std::vector<double> vals, cum;
    for (uint64_t r = 0; r < T; ++r) {
        const uint64_t m = corr::effective_n(N, len, r, 0);
        const double* xr = x + r * stride;
        const double* tr = t + r * stride;
        pairs.clear();
        for (uint64_t i = 0; i < m; ++i) {
            const double w = sample_weight(
                tr[i], i + 1 < m ? tr[i + 1] : end[r], start[r], end[r]);
            if (w > 0.0)
                pairs.emplace_back(ostat::key_of(xr[i]), double_as_u64(w));
        }
        std::sort(pairs.begin(), pairs.end());
        const uint64_t n = pairs.size();
        vals.resize(n);
        cum.resize(n);
        double acc = 0.0;
        for (uint64_t k = 0; k < n; ++k) {
            acc += u64_as_double(pairs[k].second);
            vals[k] = ostat::key_to_double(pairs[k].first);
            cum[k] = acc;
        }
        n_out[r] = (double)n;
        total_out[r] = acc;
        for (uint64_t k = 0; k < N; ++k) {
            if (vals_out) vals_out[r * N + k] = k < n ? vals[k] : quiet_nan();
            if (cum_out) cum_out[r * N + k] = k < n ? cum[k] : quiet_nan();
        }
        if (quant_out)
            for (uint32_t i = 0; i < nq; ++i)
                quant_out[r * nq + i] =
                    quantile_cum(vals.data(), cum.data(), n, acc, q[i]);
        if (hist_out)
            for (uint32_t b = 0; b < nbins; ++b)
                hist_out[r * nbins + b] =
                    hist_time(vals.data(), cum.data(), n, nbins, b);
    }
    return 0;
}

}  // namespace tstat
}  // namespace cmb
