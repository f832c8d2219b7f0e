// Batched order statistics shared by the host and the GPU path: the total
// order on doubles that hip/orderstat_kernel.hip sorts by, the quantile and
// histogram arithmetic of Dataset (dataset.hpp), the tier constants of the
// kernels and the plain host path.
//
// Rows follow corr::effective_n: row t of x[T][stride] is
// x[t*stride + skip : t*stride + min(len[t], N)], len may be null.
#pragma once

#include "config.hpp"
#include "correlogram.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace cmb {
namespace ostat {

// Longest padded row of the wave tier (one wave, eight keys per lane) and of
// the block tier (one workgroup, the row resident in 64 KB of LDS).
constexpr uint32_t WAVE_MAX = 512;
constexpr uint32_t BLOCK_MAX = 8192;
constexpr uint32_t LOG_BLOCK_MAX = 13;
static_assert(1u << LOG_BLOCK_MAX == BLOCK_MAX, "BLOCK_MAX is a power of two");
constexpr uint32_t MAX_Q = 64;
constexpr uint32_t MAX_BINS = 4096;
constexpr uint64_t MAX_KEYS = 1ull << 28;  // padded workspace, T * n_pad
constexpr uint64_t KEY_PAD = ~0ull;        // padding slots and every NaN

// Unsigned compare of keys orders the doubles: negatives have all bits
// flipped, non-negatives the sign bit, so -0.0 sorts just before +0.0.
// Every NaN, of either sign, maps to the all-ones key and sorts last.
CMB_FORCEINLINE uint64_t key_of(double x) {
    if (x != x) return KEY_PAD;
    const uint64_t u = double_as_u64(x);
    return (u >> 63) ? ~u : u | (1ull << 63);
}

// Bit pattern of the double a key stands for.  The all-ones key gives a
// quiet NaN: padding slots and NaNs look the same in the output.
CMB_FORCEINLINE uint64_t key_to_bits(uint64_t k) {
    if (k == KEY_PAD) return 0x7ff8000000000000ull;
    return (k >> 63) ? k ^ (1ull << 63) : ~k;
}
CMB_FORCEINLINE double key_to_double(uint64_t k) {
    return u64_as_double(key_to_bits(k));
}

// Dataset::quantile on an ascending row, term for term.  An empty row gives
// NaN, not Dataset's 0.0: deliberately, as lag_sums gives an empty series a
// NaN mean, so that "no data" cannot pass for a quantile of 0.
CMB_INLINE double quantile_sorted(const double* xs, uint64_t n, double q) {
    if (n == 0) return u64_as_double(0x7ff8000000000000ull);
    const double pos = q * (double)(n - 1);
    const uint64_t lo = (uint64_t)pos;
    const double frac = pos - (double)lo;
    if (lo + 1 >= n) return xs[n - 1];
    return xs[lo] * (1.0 - frac) + xs[lo + 1] * frac;
}

// Dataset::histogram: equal-width bins over [lo, hi] of the row.
CMB_INLINE double hist_width(double lo, double hi, uint32_t nbins) {
    return hi > lo ? (hi - lo) / (double)nbins : 1.0;
}
// The bin of x, clamped to [0, nbins - 1]; monotone in x.  Dataset's
// (int) cast, with the clamps applied before it so that a quotient that is
// huge or not a number (hi - lo overflowed) has a defined bin.
CMB_INLINE uint32_t hist_bin(double x, double lo, double w, uint32_t nbins) {
    const double r = (x - lo) / w;
    if (!(r >= 0.0)) return 0;
    if (r >= (double)nbins) return nbins - 1;
    return (uint32_t)r;
}
// A row is binned only when it has data and both extremes are finite (so a
// row holding a NaN, which sorts last, is not); otherwise its histogram is
// all zero.
CMB_INLINE bool hist_row_ok(const double* xs, uint64_t n) {
    if (n == 0) return false;
    const double big = 1.7976931348623157e308;
    return xs[0] >= -big && xs[0] <= big && xs[n - 1] >= -big &&
           xs[n - 1] <= big;
}

// Padded row length of a call: the longest possible effective row, rounded
// up to a power of two, at least one key per lane of a wave.
inline uint64_t pad_len(uint64_t N, uint32_t skip) {
    const uint64_t n = N > skip ? N - skip : 0;
    uint64_t p = 64;
    while (p < n) p <<= 1;
    return p;
}

inline bool args_ok(uint64_t T, uint64_t N, uint64_t stride, const double* q,
                    uint32_t nq, uint32_t nbins) {
    if (!(T >= 1 && stride >= N && nq <= MAX_Q && nbins <= MAX_BINS))
        return false;
    for (uint32_t i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return false;
    return true;
}

// The GPU path keeps T padded rows of keys in one workspace.  Call after
// args_ok.  (Every grid of the kernels is smaller than that workspace.)
inline bool grid_ok(uint64_t T, uint64_t N, uint32_t skip) {
    return N < MAX_KEYS && T <= MAX_KEYS / pad_len(N, skip);
}

// std::sort on keys per row, then the two functions above.  n_out[T];
// sorted_out[T][N] (NaN at and past n_t), quant_out[T][nq] and
// hist_out[T][nbins] may each be null.  Returns 0, or -1 on bad arguments.
inline int sort_rows_host(const double* x, uint64_t T, uint64_t N,
                          uint64_t stride, const uint32_t* len, uint32_t skip,
                          const double* q, uint32_t nq, uint32_t nbins,
                          double* n_out, double* sorted_out, double* quant_out,
                          int64_t* hist_out) {
    if (!args_ok(T, N, stride, q, nq, nbins)) return -1;
    std::vector<uint64_t> keys;
    std::vector<double> xs;
    for (uint64_t t = 0; t < T; ++t) {
        const uint64_t n = corr::effective_n(N, len, t, skip);
        const double* row = x + t * stride + skip;
        n_out[t] = (double)n;
        keys.resize(n);
        xs.resize(n);
        for (uint64_t i = 0; i < n; ++i) keys[i] = key_of(row[i]);
        std::sort(keys.begin(), keys.end());
        for (uint64_t i = 0; i < n; ++i) xs[i] = key_to_double(keys[i]);
        if (sorted_out)
            for (uint64_t i = 0; i < N; ++i)
                sorted_out[t * N + i] =
                    i < n ? xs[i] : key_to_double(KEY_PAD);
        if (quant_out)
            for (uint32_t i = 0; i < nq; ++i)
                quant_out[t * nq + i] = quantile_sorted(xs.data(), n, q[i]);
        if (hist_out) {
            int64_t* h = hist_out + t * nbins;
            for (uint32_t b = 0; b < nbins; ++b) h[b] = 0;
            if (nbins && hist_row_ok(xs.data(), n)) {
                const double w = hist_width(xs[0], xs[n - 1], nbins);
                for (uint64_t i = 0; i < n; ++i)
                    h[hist_bin(xs[i], xs[0], w, nbins)]++;
            }
        }
    }
    return 0;
}

}  // namespace ostat
}  // namespace cmb
