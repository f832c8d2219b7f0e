// Correlogram pieces shared by the host and the GPU path: the blocking
// constants of hip/correlogram_kernel.hip, the plain host lag sums and the
// Durbin-Levinson core of the partial autocorrelation.
//
// Definition (the one Dataset::acf uses): for a series x_0..x_{n-1} with
// full-series mean mu and d_s = x_s - mu, the centred raw lag sum is
//     c_k = sum_{s=0}^{n-k-1} d_s * d_{s+k},   k = 0..maxlag,
// with no 1/n and c_k = 0 for k >= n.  r_k = c_k / c_0.
#pragma once

#include "config.hpp"

#include <cstdint>
#include <limits>
#include <vector>

namespace cmb {
namespace corr {

constexpr uint32_t MAX_LAG = 255;
constexpr uint32_t SEG = 16;            // one MFMA tile edge
constexpr uint32_t STEP_SEGS = 4;       // segments one 16x16x4 MFMA covers
constexpr uint32_t STEP = SEG * STEP_SEGS;
constexpr uint32_t CHUNK_SEGS = 128;    // segments one wave owns
constexpr uint32_t CHUNK = CHUNK_SEGS * SEG;  // 2048 observations

// Block lags a wave accumulates: lag k = 16m + delta reads tiles m and
// m + 1, so maxlag needs maxlag / 16 + 2 tiles.  The kernel is instantiated
// for a few MB tiers: 2 / 5 / 6 / 9 / 17 tiles cover
// maxlag <= 15 / 63 / 79 / 127 / 255 (64 lags are the common request and
// get a tier of their own instead of paying for 127)
constexpr uint32_t mb_tier(uint32_t maxlag) {
    return maxlag <= 15   ? 2
           : maxlag <= 63  ? 5
           : maxlag <= 79  ? 6
           : maxlag <= 127 ? 9
                           : 17;
}
// doubles of LDS one wave stages: its chunk plus a halo of MB segments
constexpr uint32_t lds_doubles(uint32_t mb) { return (CHUNK_SEGS + mb) * SEG; }

// chunks that cover the longest possible effective series
inline uint64_t chunks_for(uint64_t N, uint32_t skip) {
    const uint64_t n = N > skip ? N - skip : 0;
    const uint64_t c = (n + CHUNK - 1) / CHUNK;
    return c ? c : 1;
}

inline bool args_ok(uint64_t T, uint64_t N, uint64_t stride, uint32_t maxlag) {
    return T >= 1 && stride >= N && maxlag >= 1 && maxlag <= MAX_LAG;
}

// The GPU path launches one block per (row, chunk) and one fold thread per
// (row, lag); both grids must fit a launch.  Call after args_ok.
constexpr uint64_t MAX_GRID = 0x7fffffffull;
constexpr uint64_t FOLD_WG = 256;
inline bool grid_ok(uint64_t T, uint64_t N, uint32_t skip, uint32_t maxlag) {
    return chunks_for(N, skip) <= MAX_GRID / T &&
           T <= (MAX_GRID * FOLD_WG) / ((uint64_t)maxlag + 1);
}

// effective length of a row: x[skip : min(len, N)]
CMB_INLINE uint64_t effective_n(uint64_t N, const uint32_t* len, uint64_t t,
                            uint32_t skip) {
    const uint64_t end = len && len[t] < N ? len[t] : N;
    return end > skip ? end - skip : 0;
}

// Plain f64 loops over x[T][stride].  n_out[T], mean_out[T],
// c_out[T][maxlag + 1].  Returns 0, or -1 on bad arguments.
inline int lag_sums_host(const double* x, uint64_t T, uint64_t N,
                         uint64_t stride, const uint32_t* len, uint32_t skip,
                         uint32_t maxlag, double* n_out, double* mean_out,
                         double* c_out) {
    if (!args_ok(T, N, stride, maxlag)) return -1;
    const uint64_t L1 = (uint64_t)maxlag + 1;
    for (uint64_t t = 0; t < T; ++t) {
        const uint64_t n = effective_n(N, len, t, skip);
        const double* row = x + t * stride + skip;
        double* c = c_out + t * L1;
        n_out[t] = (double)n;
        for (uint64_t k = 0; k < L1; ++k) c[k] = 0.0;
        if (n == 0) {
            mean_out[t] = std::numeric_limits<double>::quiet_NaN();
            continue;
        }
        double mu = 0.0;
        for (uint64_t s = 0; s < n; ++s) mu += row[s];
        mu /= (double)n;
        mean_out[t] = mu;
        for (uint64_t k = 0; k < L1 && k < n; ++k) {
            double ck = 0.0;
            for (uint64_t s = 0; s + k < n; ++s)
                ck += (row[s] - mu) * (row[s + k] - mu);
            c[k] = ck;
        }
    }
    return 0;
}

// Partial autocorrelations p_1..p_L from autocorrelations r_1..r_L by the
// Durbin-Levinson recursion (r[0] is r_1).
inline std::vector<double> pacf_from_acf(const std::vector<double>& r) {
    const int maxlag = (int)r.size();
    std::vector<double> p((size_t)maxlag, 0.0);
    if (r.empty()) return p;
    std::vector<double> phi_prev((size_t)maxlag + 1, 0.0);
    std::vector<double> phi((size_t)maxlag + 1, 0.0);
    double v = 1.0;
    for (int k = 1; k <= maxlag; ++k) {
        double num = r[(size_t)k - 1];
        for (int j = 1; j < k; ++j)
            num -= phi_prev[(size_t)j] * r[(size_t)(k - j) - 1];
        const double a = v > 0.0 ? num / v : 0.0;
        phi[(size_t)k] = a;
        for (int j = 1; j < k; ++j)
            phi[(size_t)j] =
                phi_prev[(size_t)j] - a * phi_prev[(size_t)(k - j)];
        v *= (1.0 - a * a);
        p[(size_t)k - 1] = a;
        phi_prev = phi;
    }
    return p;
}

}  // namespace corr
}  // namespace cmb
