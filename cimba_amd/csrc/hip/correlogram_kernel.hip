// Correlogram kernels (include/cimba/correlogram.hpp): per-trial mean and
// centred raw lag sums c_k = sum_s d_s * d_{s+k}, d = x - mean, k = 0..L,
// of a dense device array x[T][stride].
//
// Three launches, no atomics, every sum in a fixed order, so a result is
// bit-identical from run to run:
//
//   corr_mean_kernel   one wave per trial: lane-strided pass over the row,
//                      then the shuffle butterfly; writes n_t and mean_t.
//                      Rows of 16384 values or more get sixteen waves each,
//                      folded in wave order.
//   corr_lag_kernel    one wave per (trial, chunk of 2048 observations).
//                      The wave stages its chunk plus a halo of MB segments
//                      of 16 into LDS as CENTRED values, 0.0 at and past
//                      n_t, so tails, ragged rows and halos past the end
//                      need no branch in the inner loop.  It then forms the
//                      Hankel blocks
//                          D_m[i][j] = sum_a d[16a + i] * d[16(a + m) + j]
//                      with v_mfma_f64_16x16x4_f64: one step covers four
//                      segments a, lane l feeds A = d[64s + l] and
//                      B = d[64s + 16m + l], both 64 consecutive doubles
//                      (one conflict-free 8-byte LDS read per lane).  A step
//                      is one A read, MB - 1 B reads (B_0 is A) and MB
//                      MFMAs into MB accumulator tiles held in registers.
//                      Lag k = 16m + delta is diag_delta(D_m) +
//                      diag_{delta-16}(D_{m+1}): sixteen tile entries,
//                      summed by one lane in a fixed order from LDS.
//   corr_fold_kernel   sums a trial's chunk partials in chunk order (only
//                      launched when a row spans more than one chunk).
//
// LDS per wave: (128 + MB) * 16 doubles, 16.6 .. 18.1 KB, so LDS allows 8
// waves per CU; the D tiles reuse that buffer in the epilogue.  The
// accumulators are 8 * MB VGPRs; the MB = 17 tier needs 174 VGPRs in all
// and is register-limited to two waves per SIMD
// (profiles/r11_correlogram.md).
#include <hip/hip_runtime.h>

#include "../include/cimba/correlogram.hpp"
#include "hip_host.hpp"

namespace {

namespace corr = cmb::corr;

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr uint32_t WAVE = 64;
constexpr uint32_t MEAN_WG = 256;  // four trials per block
constexpr int MEAN_LONG_WPT = 16;  // waves per trial once rows are long
constexpr uint64_t MEAN_LONG_N = 16384;
constexpr uint32_t FOLD_WG = (uint32_t)corr::FOLD_WG;
constexpr uint32_t TILE = corr::SEG * corr::SEG;

// WPT waves share one trial: wave v of them takes the 64-element groups
// v, v + WPT, ... of the row.  WPT = 1 is the shape for many short rows
// (four trials per block); long rows get a whole block of WPT = 16 waves,
// whose sums lane 0 adds in wave order.
template <int WPT>
__global__ __launch_bounds__(MEAN_WG * (WPT > 1 ? 4 : 1)) void corr_mean_kernel(
    const double* __restrict__ x, uint64_t T, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, uint32_t skip,
    double* __restrict__ n_out, double* __restrict__ mean_out) {
    static_assert(WPT == 1 || WPT == MEAN_LONG_WPT, "one trial per block");
    __shared__ double wave_sum[WPT];
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = threadIdx.x / WAVE;
    const uint64_t t = WPT > 1 ? (uint64_t)blockIdx.x
                               : (uint64_t)blockIdx.x * (MEAN_WG / WAVE) + wave;
    if (t >= T) return;  // wave-uniform; never taken when WPT > 1
    const uint64_t n = corr::effective_n(N, len, t, skip);
    const double* row = x + t * stride + skip;
    // four independent partial sums per lane keep four loads in flight;
    // their order of combination is fixed
    constexpr uint64_t HOP = (uint64_t)WPT * WAVE;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint64_t i = (WPT > 1 ? wave * WAVE : 0) + lane;
    for (; i + 3 * HOP < n; i += 4 * HOP) {
        s0 += row[i];
        s1 += row[i + HOP];
        s2 += row[i + 2 * HOP];
        s3 += row[i + 3 * HOP];
    }
    for (; i < n; i += HOP) s0 += row[i];
    double s = (s0 + s1) + (s2 + s3);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (WPT > 1) {
        if (lane == 0) wave_sum[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            s = 0.0;
            for (int v = 0; v < WPT; ++v) s += wave_sum[v];
        }
    }
    if (lane == 0 && (WPT == 1 || wave == 0)) {
        n_out[t] = (double)n;
        mean_out[t] = n ? s / (double)n : __builtin_nan("");
    }
}

// D-tile layout of v_mfma_f64_16x16x4_f64 (AMD matrix instruction
// calculator): lane l, register r of the four holds D[i][j] with
// j = l % 16 and i = 4 * r + l / 16.  (The f32 16x16x4 form differs:
// i = 4 * (l / 16) + r.)  This helper is the only place that knows; the
// small-shape tests fail if it is permuted or transposed.
__device__ __forceinline__ void store_tile(double* tile, const f64x4& acc,
                                           uint32_t lane) {
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t i = 4 * r + lane / corr::SEG;
        const uint32_t j = lane % corr::SEG;
        tile[i * corr::SEG + j] = acc[r];
    }
}

// At least two waves per SIMD caps the kernel at 256 registers, which makes
// the compiler keep the MFMA accumulators in VGPRs.  With the default
// budget of 512 it puts them in AGPRs and copies every tile to and from
// VGPRs around the MFMAs of each step (8 * MB copies each way per step).
template <int MB>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2)))
void corr_lag_kernel(
    const double* __restrict__ x, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, uint32_t skip, uint32_t maxlag,
    uint64_t nchunks, const double* __restrict__ mean,
    double* __restrict__ partial) {
    __shared__ double d[corr::lds_doubles(MB)];
    static_assert(corr::lds_doubles(MB) >= 5 * TILE, "epilogue reuses d[]");
    const uint32_t lane = threadIdx.x;
    const uint64_t w = blockIdx.x;
    const uint64_t t = w / nchunks;
    const uint64_t base = (w - t * nchunks) * corr::CHUNK;
    const uint64_t n = corr::effective_n(N, len, t, skip);
    double* out = partial + w * ((uint64_t)maxlag + 1);
    if (base >= n) {  // chunk past the end of a short row (or n == 0)
        for (uint32_t k = lane; k <= maxlag; k += WAVE) out[k] = 0.0;
        return;
    }
    const uint64_t rem = n - base;
    const uint32_t own = rem < corr::CHUNK ? (uint32_t)rem : corr::CHUNK;
    const uint32_t steps = (own + corr::STEP - 1) / corr::STEP;
    // the steps read d[0 .. 64 * steps + 16 * (MB - 1)); stage whole
    // segments up to there, centred, zero at and past the row's end
    const uint32_t staged = steps * corr::STEP + MB * corr::SEG;
    const double mu = mean[t];
    const double* row = x + t * stride + skip + base;
    // the load is unconditional (index clamped into the row) so that the
    // unrolled loop keeps four of them in flight
#pragma unroll 4
    for (uint32_t p = lane; p < staged; p += WAVE) {
        const double v = row[p < rem ? p : rem - 1];
        d[p] = p < rem ? v - mu : 0.0;
    }
    __syncthreads();

    f64x4 acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint32_t s = 0; s < steps; ++s) {
        const double* p = d + s * corr::STEP + lane;
        const double a = p[0];
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc[0], 0, 0, 0);
#pragma unroll
        for (int m = 1; m < MB; ++m)
            acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                a, p[m * corr::SEG], acc[m], 0, 0, 0);
    }

    // epilogue: four block lags at a time.  Tiles 4g .. 4g + 4 go to LDS;
    // lane (mm, delta) walks row i of tile mm while i + delta < 16 and of
    // tile mm + 1 after, which is lag 16 * (4g + mm) + delta.
    const uint32_t mm = lane / corr::SEG, delta = lane % corr::SEG;
#pragma unroll
    for (int g = 0; 4 * g < MB - 1; ++g) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 5; ++q)
            if (4 * g + q < MB) store_tile(d + q * TILE, acc[4 * g + q], lane);
        __syncthreads();
        const uint32_t m = 4 * g + mm;
        const uint32_t k = m * corr::SEG + delta;
        if (m + 1 < (uint32_t)MB && k <= maxlag) {
            double sum = 0.0;
#pragma unroll
            for (uint32_t i = 0; i < corr::SEG; ++i) {
                const uint32_t j = i + delta;
                sum += d[(mm + j / corr::SEG) * TILE + i * corr::SEG +
                         j % corr::SEG];
            }
            out[k] = sum;
        }
    }
}

__global__ __launch_bounds__(FOLD_WG) void corr_fold_kernel(
    const double* __restrict__ partial, uint64_t T, uint64_t nchunks,
    uint32_t L1, double* __restrict__ c) {
    const uint64_t idx = (uint64_t)blockIdx.x * FOLD_WG + threadIdx.x;
    if (idx >= T * L1) return;
    const uint64_t t = idx / L1;
    const uint64_t k = idx - t * L1;
    const double* p = partial + t * nchunks * L1 + k;
    double s = 0.0;
    for (uint64_t ch = 0; ch < nchunks; ++ch, p += L1) s += *p;
    c[idx] = s;
}

template <int MB>
void launch_lag(uint64_t blocks, const double* x, uint64_t N, uint64_t stride,
                const uint32_t* len, uint32_t skip, uint32_t maxlag,
                uint64_t nchunks, const double* mean, double* partial) {
    hipLaunchKernelGGL(corr_lag_kernel<MB>, dim3((uint32_t)blocks), dim3(WAVE),
                       0, 0, x, N, stride, len, skip, maxlag, nchunks, mean,
                       partial);
}

}  // namespace

extern "C" {

// Device pointers: x[T][stride] (the last row may end after N values),
// len[T] or null, n[T], mean[T], c[T][maxlag + 1].  elapsed_ms (nullable)
// is the three kernels alone.
int cimba_lag_sums_gpu_dev(const double* x, uint64_t T, uint64_t N,
                           uint64_t stride, const uint32_t* len, uint32_t skip,
                           uint32_t maxlag, double* n_out, double* mean_out,
                           double* c_out, double* elapsed_ms) {
    if (!corr::args_ok(T, N, stride, maxlag) ||
        !corr::grid_ok(T, N, skip, maxlag))
        return (int)hipErrorInvalidValue;
    const uint64_t nchunks = corr::chunks_for(N, skip);
    const uint32_t L1 = maxlag + 1;
    const uint64_t mean_blocks = (T + MEAN_WG / WAVE - 1) / (MEAN_WG / WAVE);
    const uint64_t fold_blocks = (T * L1 + FOLD_WG - 1) / FOLD_WG;
    const uint64_t lag_blocks = T * nchunks;
    // a single-chunk launch writes c directly: nothing to fold
    cmb_hip::DevBuf<double> d_partial;
    if (nchunks > 1) HIP_TRY(d_partial.alloc(lag_blocks * L1));
    double* partial = nchunks > 1 ? d_partial.get() : c_out;

    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    if (N >= MEAN_LONG_N)
        hipLaunchKernelGGL(corr_mean_kernel<MEAN_LONG_WPT>, dim3((uint32_t)T),
                           dim3(MEAN_LONG_WPT * WAVE), 0, 0, x, T, N, stride,
                           len, skip, n_out, mean_out);
    else
        hipLaunchKernelGGL(corr_mean_kernel<1>, dim3((uint32_t)mean_blocks),
                           dim3(MEAN_WG), 0, 0, x, T, N, stride, len, skip,
                           n_out, mean_out);
    HIP_TRY(hipGetLastError());
    switch (corr::mb_tier(maxlag)) {
        case 2:
            launch_lag<2>(lag_blocks, x, N, stride, len, skip, maxlag, nchunks,
                          mean_out, partial);
            break;
        case 5:
            launch_lag<5>(lag_blocks, x, N, stride, len, skip, maxlag, nchunks,
                          mean_out, partial);
            break;
        case 6:
            launch_lag<6>(lag_blocks, x, N, stride, len, skip, maxlag, nchunks,
                          mean_out, partial);
            break;
        case 9:
            launch_lag<9>(lag_blocks, x, N, stride, len, skip, maxlag, nchunks,
                          mean_out, partial);
            break;
        default:
            launch_lag<17>(lag_blocks, x, N, stride, len, skip, maxlag,
                           nchunks, mean_out, partial);
            break;
    }
    HIP_TRY(hipGetLastError());
    if (nchunks > 1) {
        hipLaunchKernelGGL(corr_fold_kernel, dim3((uint32_t)fold_blocks),
                           dim3(FOLD_WG), 0, 0, partial, T, nchunks, L1,
                           c_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;
    return 0;
}

// Host arrays in and out: host_x[T][stride] (T - 1 full rows and N values
// of the last), host_len[T] or null; n_out[T], mean_out[T],
// c_out[T][maxlag + 1].
int cimba_lag_sums_gpu(const double* host_x, uint64_t T, uint64_t N,
                       uint64_t stride, const uint32_t* host_len,
                       uint32_t skip, uint32_t maxlag, int device,
                       double* n_out, double* mean_out, double* c_out,
                       double* elapsed_ms) {
    if (!corr::args_ok(T, N, stride, maxlag)) return (int)hipErrorInvalidValue;
    HIP_TRY(hipSetDevice(device));
    const size_t nx = (size_t)((T - 1) * stride + N);
    const size_t nc = (size_t)T * (maxlag + 1);
    cmb_hip::DevBuf<double> d_x, d_n, d_mean, d_c;
    cmb_hip::DevBuf<uint32_t> d_len;
    HIP_TRY(d_x.alloc(nx ? nx : 1));
    HIP_TRY(d_n.alloc(T));
    HIP_TRY(d_mean.alloc(T));
    HIP_TRY(d_c.alloc(nc));
    if (nx) HIP_TRY(d_x.upload(host_x, nx));
    if (host_len) {
        HIP_TRY(d_len.alloc(T));
        HIP_TRY(d_len.upload(host_len, T));
    }
    HIP_TRY(cimba_lag_sums_gpu_dev(d_x.get(), T, N, stride, d_len.get(), skip,
                                   maxlag, d_n.get(), d_mean.get(), d_c.get(),
                                   elapsed_ms));
    HIP_TRY(d_n.download(n_out, T));
    HIP_TRY(d_mean.download(mean_out, T));
    return d_c.download(c_out, nc);
}

}  // extern "C"
