// Regular-grid time averages of piecewise-constant state histories, shared
// by the host and the GPU path (hip/timebatch_kernel.hip): the grid of a
// row, the merge of sample times and grid edges that lists a row's pieces,
// the tier constants of the kernel and the plain host path.  The bridge from
// a history (values, times) to an equally spaced series [T, K] that
// steadystate.hpp and correlogram.hpp take as it is.
//
// Row r of x[T][stride] and t[T][stride] holds m = min(len[r], N) samples
// (len may be null) and has a window [start_r, end_r].  A row is off when
// either bound is not finite or end <= start: its batches have integral =
// covered = 0, mean NaN and its width is NaN.  Otherwise w = (end - start) /
// K, edge b_j = start + j * w for j < K and b_K = end.
//
// Sample i holds from t_i to nx_i = t_{i+1} (end for the last one).  Its
// overlap with batch j is ov = tstat::sample_weight(t_i, nx_i, b_j, b_{j+1}),
// and (i, j) is a piece iff ov > 0.  Per batch integral = sum x_i * ov,
// covered = sum ov, mean = integral / covered (NaN where covered == 0); per
// row n counts the samples with positive weight in [start, end].
//
// Pieces are listed by a merge.  key_i is the running maximum of the finite
// times up to i, clamped to [start, end]: t_i itself wherever the times are
// non-decreasing, and sorted whatever the row holds.  The merge of key_0 ..
// key_{m-1} with the interior edges b_1 .. b_{K-1}, an edge going first on a
// tie, has m + K - 1 steps.  After each step the last sample and the number
// of edges taken name one candidate (i, j); every piece is among them once,
// in order of j and then i, and a candidate that is no piece has ov <= 0 or
// NaN.  The host walks the merge step by step, the kernel gives each lane an
// equal share of its steps.
#pragma once

#include "timestat.hpp"

#include <cstdint>

namespace cmb {
namespace tbatch {

constexpr uint32_t MAX_BATCHES = 65536;
// Merge steps per lane, longest N + K of the wave tier (one wave per row,
// the whole merge in one chunk) and merge steps per chunk of the block tier
// (one workgroup of 256 per row).
constexpr uint32_t LANE_STEPS = 8;
constexpr uint32_t WAVE_MAX = 64 * LANE_STEPS;
constexpr uint32_t CHUNK = 256 * LANE_STEPS;

CMB_INLINE bool finite(double v) { return v - v == 0.0; }

CMB_INLINE bool row_on(double start, double end) {
    return finite(start) && finite(end) && end > start;
}

CMB_INLINE double width(double start, double end, uint32_t K) {
    return row_on(start, end) ? (end - start) / (double)K : tstat::quiet_nan();
}

// b_j of a row that is on, 0 <= j <= K
CMB_INLINE double edge(double start, double w, double end, uint32_t j,
                       uint32_t K) {
    return j < K ? start + (double)j * w : end;
}

// key of a sample at time ti when the key before it is prev (start for the
// first sample); prev lies in [start, end]
CMB_INLINE double next_key(double prev, double ti, double end) {
    const double k = ti > prev ? ti : prev;  // a NaN keeps prev
    return k > end ? end : k;
}

CMB_INLINE double mean_of(double integral, double covered) {
    return covered > 0.0 ? integral / covered : tstat::quiet_nan();
}

inline bool args_ok(uint64_t T, uint64_t N, uint64_t stride, uint32_t K) {
    return T >= 1 && stride >= N && K >= 1 && K <= MAX_BATCHES;
}

// The GPU path: T * N inputs and T * K outputs within ostat's workspace rule.
inline bool grid_ok(uint64_t T, uint64_t N, uint32_t K) {
    return ostat::grid_ok(T, N, 0) && ostat::grid_ok(T, K, 0);
}

// The merge, one step at a time, pieces summed left to right.  n_out[T],
// width_out[T]; integral_out, covered_out and mean_out are [T][K].  Returns
// 0, or -1 on bad arguments.
inline int time_batches_host(const double* x, const double* t, uint64_t T,
                             uint64_t N, uint64_t stride, const uint32_t* len,
                             const double* start, const double* end,
                             uint32_t K, double* n_out, double* width_out,
                             double* integral_out, double* covered_out,
                             double* mean_out) {
    if (!args_ok(T, N, stride, K)) return -1;
    for (uint64_t r = 0; r < T; ++r) {
        const uint64_t m = corr::effective_n(N, len, r, 0);
        const double* xr = x + r * stride;
        const double* tr = t + r * stride;
        const double s = start[r], e = end[r];
        const double w = width(s, e, K);
        double* ig = integral_out + r * K;
        double* cv = covered_out + r * K;
        double* mn = mean_out + r * K;
        width_out[r] = w;
        uint64_t n = 0;
        if (!row_on(s, e)) {
            for (uint32_t j = 0; j < K; ++j) {
                ig[j] = cv[j] = 0.0;
                mn[j] = tstat::quiet_nan();
            }
            n_out[r] = 0.0;
            continue;
        }
        uint64_t i = 0;  // samples taken
        uint32_t j = 0;  // edges taken: the open batch
        double key = m ? next_key(s, tr[0], e) : e;  // of sample i
        double lo = s, hi = edge(s, w, e, 1, K);
        double ai = 0.0, ac = 0.0;
        const uint64_t steps = m + K - 1;
        for (uint64_t d = 0; d < steps; ++d) {
            if (j + 1 < K && (i >= m || hi <= key)) {
                ig[j] = ai;
                cv[j] = ac;
                mn[j] = mean_of(ai, ac);
                ai = ac = 0.0;
                ++j;
                lo = hi;
                hi = edge(s, w, e, j + 1, K);
            } else {
                ++i;
                const double nx = i < m ? tr[i] : e;
                if (tstat::sample_weight(tr[i - 1], nx, s, e) > 0.0) ++n;
                if (i < m) key = next_key(key, tr[i], e);
            }
            if (i) {
                const double ov = tstat::sample_weight(
                    tr[i - 1], i < m ? tr[i] : e, lo, hi);
                if (ov > 0.0) {
                    ai += xr[i - 1] * ov;
                    ac += ov;
                }
            }
        }
        ig[j] = ai;
        cv[j] = ac;
        mn[j] = mean_of(ai, ac);
        n_out[r] = (double)n;
    }
    return 0;
}

}  // namespace tbatch
}  // namespace cmb
