// Steady-state output analysis shared by the host and the GPU path: the
// MSER-m truncation point and the batch-means doubling ladder of many output
// series at once, the blocking constants of hip/steadystate_kernel.hip and
// the plain host loops.
//
// Row.  Row r of x[T][stride] is x[r][skip_r : min(len_r, N)], n_r values
// (0 when skip_r is at or past the end); len may be null, skip has T entries.
//
// Batch means.  For a batch size m >= 1, k = n_r / m (trailing observations
// are dropped) and
//     y_j = (0.0 + x_{jm} + x_{jm+1} + ... + x_{jm+m-1}) / m,
// summed left to right in double and divided once.  The build has
// -ffp-contract=off, so host and GPU give the same bits for every y_j.
//
// Doubling ladder.  Level 0 is y_j.  Level l + 1 has k_{l+1} = k_l / 2 means
//     y^{l+1}_j = (y^l_{2j} + y^l_{2j+1}) / 2,
// one add and an exact halving: every level is bit-identical on both paths.
// k_l = k >> l, and the batch size of level l is m << l.
//
// MSER-m (White and Spratt).  With dmax = k / 2 and, for d = 0..dmax,
//     stat(d) = sum_{j=d}^{k-1} (y_j - ybar_d)^2 / (k - d)^2,
// ybar_d the mean of y_d..y_{k-1}: d* is the smallest d in [0, dmax] that
// minimises stat(d) among those whose stat(d) is not NaN; without one (k = 0,
// or a NaN at or past dmax) d* = 0, stat = NaN and mean = NaN.  The suffix
// (count, mean, M2) triples come from Moments2::merge (stats.hpp), never from
// raw sums of squares.  The host adds one y_j at a time from the row's end;
// the GPU merges pieces in a tree, so stat and mean agree to rounding only.
//
// Ladder sums.  Per level l, over that level's k_l means: mean (their sum in
// order, divided by k_l), sse = sum (y_j - mean)^2,
// c1 = sum_{j<k_l-1} (y_j - mean)(y_{j+1} - mean) and
// dsq = sum_{j<k_l-1} (y_{j+1} - y_j)^2, the numerator of von Neumann's
// ratio, returned as a sum of its own because taking it from sse, c1 and the
// end terms cancels badly for the strongly correlated series it is meant
// for.  k_l = 0 gives a NaN mean and sums of 0.0, as lag_sums does.  Both
// paths take the mean in a first sweep and the centred sums in a second one
// (two-pass, the definition the tolerances of the correlogram are written
// for); the GPU adds in another order.
#pragma once

#include "config.hpp"
#include "stats.hpp"

#include <cstdint>
#include <limits>
#include <vector>

namespace cmb {
namespace sstat {

constexpr uint32_t WAVE = 64;
constexpr uint32_t REGS = 4;              // batch means a lane holds
constexpr uint32_t CHUNK_LOG = 8;
constexpr uint32_t CHUNK = WAVE * REGS;   // batch means a wave takes at once
static_assert(1u << CHUNK_LOG == CHUNK, "a chunk is a whole ladder subtree");
// Batch sizes up to M_STAGE go through LDS: 64 batches of a row-contiguous,
// coalesced load, batch b at b * stage_stride(m), an odd number of doubles,
// so that the 64 lanes reading element i of their own batch hit 64
// different banks.  Larger batches are summed straight from global memory,
// a lane walking its own cache lines.
constexpr uint32_t M_STAGE = 16;
constexpr uint32_t stage_stride(uint32_t m) { return m | 1; }
// Rows of up to WAVE_MAX observations (N) get one wave each, four rows to a
// workgroup; longer rows get a workgroup of BLOCK_WAVES waves each, which
// take BLOCK_WAVES consecutive chunks per round.
constexpr uint32_t WAVE_MAX = 8192;
constexpr uint32_t BLOCK_WAVES = 4;
constexpr uint32_t WAVE_ROWS = 4;
constexpr uint32_t MAX_LEVELS = 16;
// doubles of LDS one wave owns: the staging tile and the chunk's batch means
// at a stride of REGS + 1 (lane l reads its REGS consecutive means without
// a bank conflict).  11.3 KB a wave, 45 KB for a workgroup of four in either
// tier; the seam, carry and level state on top of it is under 2 KB.
constexpr uint32_t lds_doubles() {
    return WAVE * stage_stride(M_STAGE) + WAVE * (REGS + 1);
}

constexpr uint64_t MAX_GRID = 0x7fffffffull;

inline bool args_ok(uint64_t T, uint64_t N, uint64_t stride, uint64_t m,
                    uint64_t levels) {
    return T >= 1 && stride >= N && m >= 1 && m <= 0xffffffffull &&
           N <= 0xffffffffull && levels >= 1 && levels <= MAX_LEVELS;
}
// one workgroup per WAVE_ROWS rows, or per row.  Call after args_ok.
inline bool grid_ok(uint64_t T, uint64_t N) {
    return N <= WAVE_MAX ? (T + WAVE_ROWS - 1) / WAVE_ROWS <= MAX_GRID
                         : T <= MAX_GRID;
}
// width of a row of the MSER curve: d = 0 .. N / (2 m)
inline uint64_t curve_width(uint64_t N, uint64_t m) { return N / (2 * m) + 1; }

struct Row {
    uint64_t first;  // index in the row's storage of its first observation
    uint64_t n;
};
CMB_INLINE Row row_of(uint64_t N, const uint32_t* len, const uint32_t* skip,
                      uint64_t t) {
    const uint64_t end = len && len[t] < N ? len[t] : N;
    const uint64_t s = skip[t] < end ? skip[t] : end;
    return Row{s, end - s};
}

CMB_INLINE double nan_value() { return u64_as_double(0x7ff8000000000000ull); }

// one level-0 batch mean, the operation order of the definition
CMB_INLINE double batch_mean(const double* x, uint32_t m) {
    double s = 0.0;
    for (uint32_t i = 0; i < m; ++i) s += x[i];
    return s / (double)m;
}

// The running (best stat, its d, its mean): take() is offered candidates in
// any order and keeps the smallest stat that is not NaN, the smaller d on a
// tie.
struct Best {
    double stat, mean;
    uint32_t d;
    CMB_FORCEINLINE void reset() { stat = nan_value(); mean = nan_value(); d = 0; }
    CMB_FORCEINLINE void take(double s, double mu, uint32_t at) {
        if (s != s) return;
        if (stat != stat || s < stat || (s == stat && at < d)) {
            stat = s; mean = mu; d = at;
        }
    }
};

// Sequential host path.  skip[T]; n, k, d, cut: uint32 [T]; stat, mean:
// double [T]; curve: null or double [T][curve_width(N, m)].  Returns 0, or
// -1 on bad arguments.
inline int mser_host(const double* x, uint64_t T, uint64_t N, uint64_t stride,
                     const uint32_t* len, const uint32_t* skip, uint32_t m,
                     uint32_t* n_out, uint32_t* k_out, uint32_t* d_out,
                     uint32_t* cut_out, double* stat_out, double* mean_out,
                     double* curve_out) {
    if (!args_ok(T, N, stride, m, 1)) return -1;
    const uint64_t cw = curve_width(N, m);
    for (uint64_t t = 0; t < T; ++t) {
        const Row r = row_of(N, len, skip, t);
        const double* row = x + t * stride + r.first;
        const uint64_t k = r.n / m, dmax = k / 2;
        double* curve = curve_out ? curve_out + t * cw : nullptr;
        if (curve)
            for (uint64_t d = 0; d < cw; ++d) curve[d] = nan_value();
        Best best;
        best.reset();
        Moments2 acc, one;
        acc.reset();
        for (uint64_t j = k; j-- > 0;) {
            one.set_one(batch_mean(row + j * m, m));
            acc.merge(one);
            if (j > dmax) continue;
            const double s = acc.m2 / (acc.n * acc.n);
            best.take(s, acc.mean, (uint32_t)j);
            if (curve) curve[j] = s;
        }
        n_out[t] = (uint32_t)r.n;
        k_out[t] = (uint32_t)k;
        d_out[t] = best.d;
        cut_out[t] = skip[t] + best.d * m;
        stat_out[t] = best.stat;
        mean_out[t] = best.mean;
    }
    return 0;
}

// Sequential host path of the ladder.  Every output is double [T][levels].
inline int batch_means_host(const double* x, uint64_t T, uint64_t N,
                            uint64_t stride, const uint32_t* len,
                            const uint32_t* skip, uint32_t m, uint32_t levels,
                            double* k_out, double* mean_out, double* sse_out,
                            double* c1_out, double* dsq_out) {
    if (!args_ok(T, N, stride, m, levels)) return -1;
    std::vector<double> y;
    for (uint64_t t = 0; t < T; ++t) {
        const Row r = row_of(N, len, skip, t);
        const double* row = x + t * stride + r.first;
        uint64_t k = r.n / m;
        y.resize(k);
        for (uint64_t j = 0; j < k; ++j) y[j] = batch_mean(row + j * m, m);
        for (uint32_t l = 0; l < levels; ++l) {
            if (l > 0) {
                k /= 2;
                for (uint64_t j = 0; j < k; ++j)
                    y[j] = (y[2 * j] + y[2 * j + 1]) / 2.0;
            }
            const uint64_t o = t * levels + l;
            double mu = 0.0, sse = 0.0, c1 = 0.0, dsq = 0.0;
            for (uint64_t j = 0; j < k; ++j) mu += y[j];
            mu = k ? mu / (double)k : nan_value();
            for (uint64_t j = 0; j < k; ++j) {
                const double a = y[j] - mu;
                sse += a * a;
                if (j + 1 < k) {
                    c1 += a * (y[j + 1] - mu);
                    dsq += (y[j + 1] - y[j]) * (y[j + 1] - y[j]);
                }
            }
            k_out[o] = (double)k;
            mean_out[o] = mu;
            sse_out[o] = sse;
            c1_out[o] = c1;
            dsq_out[o] = dsq;
        }
    }
    return 0;
}

}  // namespace sstat
}  // namespace cmb
