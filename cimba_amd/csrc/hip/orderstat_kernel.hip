// Batched order statistics (include/cimba/orderstat.hpp): every row of a
// dense device array x[T][stride] sorted by the 64-bit key of its doubles,
// then quantiles and an equal-width histogram read off the sorted rows.
//
// The sort is a bitonic network on keys.  Rows are padded with all-ones keys
// to n_pad, a power of two that fits the longest possible row of the call,
// and all rows of a call take the same tier.  No atomics, every exchange at
// a fixed place in the network: a result is the same from run to run.
//
//   ostat_wave_kernel<K>   n_pad = 64 K <= 512: one wave per row, four rows
//       per block, K keys per lane (element e = lane * K + j).  Strides
//       below K are compare-exchanges between registers of a lane; strides
//       K and up exchange the two key halves with lane ^ m: DPP quad_perm
//       for m = 1, 2, ds_swizzle for 4, 8, 16, ds_bpermute for 32.  No LDS,
//       no barrier.
//   ostat_block_kernel<NPAD>  n_pad = 1024 .. 8192: one workgroup of
//       NPAD / 8 threads per row, keys in LDS.  A thread first sorts its 8
//       adjacent keys in registers (merge sizes 2, 4, 8).  After that every
//       pass is register-blocked: a thread reads the 8 keys closed under
//       three consecutive strides 4s, 2s, s, does those levels (12
//       compare-exchanges) and writes them back, one LDS round trip and one
//       barrier per three levels.  A merge whose level count is no multiple
//       of three starts with a pass of one or two levels, so the last pass
//       is always strides 4, 2, 1 on 8 adjacent keys, and the last of all
//       goes from registers straight to global memory.
//       LDS index: i ^ f(i >> 5), f chosen so that for every pass stride
//       s = 1 .. 16 (and trivially above) 32 consecutive lanes hit 32
//       different 8-byte slots; no padding, so 8192 keys are exactly 64 KB.
//   chunk tier, n_pad > 8192, keys[T][n_pad] in a global workspace:
//     ostat_chunk_sort_kernel    sorts each chunk of 8192 as the block tier
//         does; the direction of element g at merge size k is (g & k) == 0
//         on the index in the whole row, so chunks alternate.
//     ostat_global_merge_kernel<NL>  for merge size k the levels with stride
//         >= 8192, NL <= 3 of them per launch, 2^NL strided keys per
//         thread, consecutive threads on consecutive keys.
//     ostat_chunk_merge_kernel   the strides below 8192 of that merge, one
//         chunk per workgroup in LDS (one level, then four passes of three).
//   ostat_quantile_kernel  one thread per (row, q): quantile_sorted.
//   ostat_hist_kernel      one thread per (row, bin): binary search for the
//       first sorted value whose hist_bin exceeds the bin; counts are
//       differences of neighbouring boundaries.
//
// The last pass of each tier stores doubles, not keys: into the workspace
// row (read by the two epilogue kernels) and into sorted_out[T][N], NaN at
// and past n_t, each only when wanted.
//
// Compiler's resource report (gfx950, -O3; profiles/r13_orderstat.md):
//   ostat_wave_kernel<1/2/4/8>      14 / 23 / 39 / 69 VGPRs, no LDS;
//                                   8 waves per SIMD, 7 at K = 8
//   ostat_block_kernel<1024..8192>  56 VGPRs, LDS 8 / 16 / 32 / 64 KB
//   ostat_chunk_sort_kernel         41 VGPRs, LDS 64 KB
//   ostat_chunk_merge_kernel        34 VGPRs, LDS 64 KB
//   ostat_global_merge_kernel<1/2/3>  11 / 20 / 38 VGPRs, no LDS
//   ostat_quantile_kernel 14, ostat_hist_kernel 30 VGPRs, no LDS
// No kernel uses scratch.  64 KB of LDS allows two workgroups of 1024
// threads per CU, 8 waves per SIMD, which the registers allow too.
#include <hip/hip_runtime.h>

#include "../include/cimba/orderstat.hpp"
#include "hip_host.hpp"

namespace {

namespace ostat = cmb::ostat;
namespace corr = cmb::corr;

constexpr uint32_t WAVE = 64;
constexpr uint32_t WAVE_WG = 256;  // four rows per block
constexpr uint32_t FLAT_WG = 256;
constexpr uint32_t BM = ostat::BLOCK_MAX;
constexpr uint32_t LBM = ostat::LOG_BLOCK_MAX;

struct QList {
    double q[ostat::MAX_Q];
};

// ---- wave tier -------------------------------------------------------------

// v of lane ^ m.  After unrolling m is a constant and one case is left.
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, uint32_t m,
                                             uint32_t lane) {
    switch (m) {
        case 1:  // quad_perm [1, 0, 3, 2]
            return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF,
                                                         0xF, true);
        case 2:  // quad_perm [2, 3, 0, 1]
            return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF,
                                                         0xF, true);
        // bit mode: and_mask 0x1f, or_mask 0, xor_mask m (within 32 lanes)
        case 4:
            return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v,
                                                         (4 << 10) | 0x1F);
        case 8:
            return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v,
                                                         (8 << 10) | 0x1F);
        case 16:
            return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v,
                                                         (16 << 10) | 0x1F);
        default:
            return (uint32_t)__builtin_amdgcn_ds_bpermute(
                (int)((lane ^ m) << 2), (int)v);
    }
}

__device__ __forceinline__ uint64_t lane_xor64(uint64_t v, uint32_t m,
                                               uint32_t lane) {
    const uint32_t lo = lane_xor((uint32_t)v, m, lane);
    const uint32_t hi = lane_xor((uint32_t)(v >> 32), m, lane);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void cmpx(uint64_t& a, uint64_t& b, bool asc) {
    const bool lt = a < b;
    const uint64_t lo = lt ? a : b, hi = lt ? b : a;
    a = asc ? lo : hi;
    b = asc ? hi : lo;
}

// Eight values a thread holds for row t, columns col .. col + 7, to the
// workspace row and to sorted_out (columns below N only).
template <int NV>
__device__ __forceinline__ void store_sorted(const uint64_t (&r)[NV],
                                             uint64_t t, uint32_t col,
                                             uint64_t n_pad, uint64_t N,
                                             uint64_t* __restrict__ ws,
                                             uint64_t* __restrict__ sorted) {
    if (ws) {
#pragma unroll
        for (int m = 0; m < NV; ++m)
            ws[t * n_pad + col + m] = ostat::key_to_bits(r[m]);
    }
    if (sorted) {
#pragma unroll
        for (int m = 0; m < NV; ++m)
            if (col + m < N) sorted[t * N + col + m] = ostat::key_to_bits(r[m]);
    }
}

// columns n_pad .. N - 1 of sorted_out exist when skip > 0: they are NaN
__device__ __forceinline__ void fill_tail(uint64_t t, uint32_t tid,
                                          uint32_t nthreads, uint64_t n_pad,
                                          uint64_t N,
                                          uint64_t* __restrict__ sorted) {
    if (!sorted) return;
    for (uint64_t c = n_pad + tid; c < N; c += nthreads)
        sorted[t * N + c] = ostat::key_to_bits(ostat::KEY_PAD);
}

template <int K>
__global__ __launch_bounds__(WAVE_WG) void ostat_wave_kernel(
    const double* __restrict__ x, uint64_t T, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, uint32_t skip,
    double* __restrict__ n_out, uint64_t* __restrict__ ws,
    uint64_t* __restrict__ sorted) {
    constexpr uint32_t NPAD = WAVE * K;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t t = (uint64_t)blockIdx.x * (WAVE_WG / WAVE) +
                       threadIdx.x / WAVE;
    if (t >= T) return;  // wave-uniform: the shuffles see all 64 lanes
    const uint64_t n = corr::effective_n(N, len, t, skip);
    const double* row = x + t * stride + skip;
    uint64_t r[K];
#pragma unroll
    for (uint32_t j = 0; j < K; ++j) {
        const uint32_t e = lane * K + j;
        r[j] = e < n ? ostat::key_of(row[e]) : ostat::KEY_PAD;
    }
#pragma unroll
    for (uint32_t k = 2; k <= NPAD; k <<= 1) {
#pragma unroll
        for (uint32_t s = k >> 1; s >= 1; s >>= 1) {
            if (s >= K) {
                const uint32_t m = s / K;
                // the lower lane of a pair keeps the smaller key when the
                // pair sorts ascending
                const bool keep_min =
                    ((lane & m) == 0) == (((lane * K) & k) == 0);
#pragma unroll
                for (uint32_t j = 0; j < K; ++j) {
                    const uint64_t o = lane_xor64(r[j], m, lane);
                    const bool take = keep_min ? o < r[j] : o > r[j];
                    r[j] = take ? o : r[j];
                }
            } else {
#pragma unroll
                for (uint32_t j = 0; j < K; ++j)
                    if (!(j & s))
                        cmpx(r[j], r[j | s], ((lane * K + j) & k) == 0);
            }
        }
    }
    if (lane == 0) n_out[t] = (double)n;
    store_sorted<K>(r, t, lane * K, NPAD, N, ws, sorted);
    fill_tail(t, lane, WAVE, NPAD, N, sorted);
}

// ---- block tier ------------------------------------------------------------

// LDS slot of key i.  With h = i >> 5, bits 0..2 of h are folded into the
// low five bits as h0 -> bit 2, h1 -> bits 3 and 0, h2 -> bits 4 and 1.
// A pass with low stride s = 2^a gives the 32 lanes of a half wave indices
// that differ in bits {0..a-1} and {a+3..7}; for every a the fold makes the
// low five slot bits a bijection of those, so no two lanes share a slot.
__device__ __forceinline__ uint32_t slot(uint32_t i) {
    const uint32_t h = i >> 5;
    return i ^ (((h & 1u) << 2) | (((h >> 1) & 3u) * 9u));
}

// the top NL of the three levels (strides 4s, 2s, s) on a thread's 8 keys
template <int NL>
__device__ __forceinline__ void levels8(uint64_t (&r)[8], bool asc) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int bit = 4 >> l;
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (!(m & bit)) cmpx(r[m], r[m | bit], asc);
    }
}

// One register-blocked pass at low stride 2^ls0 of merge size k (k is at
// least 8 strides, so one direction serves the 8 keys).  gbase is the index
// of the chunk's first key in its row.
template <int NL, bool WRITE>
__device__ __forceinline__ void lds_pass(uint64_t* keys, uint32_t tid,
                                         uint32_t ls0, uint32_t gbase,
                                         uint32_t k, uint64_t (&r)[8]) {
    const uint32_t s0 = 1u << ls0;
    const uint32_t base = ((tid >> ls0) << (ls0 + 3)) | (tid & (s0 - 1));
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) r[m] = keys[slot(base + m * s0)];
    levels8<NL>(r, ((gbase + base) & k) == 0);
    if (WRITE) {
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m) keys[slot(base + m * s0)] = r[m];
    }
}

// Strides 2^ltop .. 1 of merge size k on keys in LDS (ltop >= 3).  The last
// pass leaves keys 8 tid .. 8 tid + 7 in r; they go back to LDS only when
// another merge follows.  Every thread of the block calls this.
__device__ __forceinline__ void lds_merge(uint64_t* keys, uint32_t tid,
                                          uint32_t ltop, uint32_t gbase,
                                          uint32_t k, uint64_t (&r)[8],
                                          bool writeback) {
    uint32_t l = ltop;
    const uint32_t rem = (ltop + 1) % 3;
    if (rem == 1) {
        lds_pass<1, true>(keys, tid, l - 2, gbase, k, r);
        l -= 1;
        __syncthreads();
    } else if (rem == 2) {
        lds_pass<2, true>(keys, tid, l - 2, gbase, k, r);
        l -= 2;
        __syncthreads();
    }
    while (l > 2) {
        lds_pass<3, true>(keys, tid, l - 2, gbase, k, r);
        l -= 3;
        __syncthreads();
    }
    lds_pass<3, false>(keys, tid, 0, gbase, k, r);
    if (writeback) {
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m) keys[slot(8 * tid + m)] = r[m];
        __syncthreads();
    }
}

// Keys gbase + 8 tid .. + 7 of a row from x, sorted in registers through
// merge sizes 2, 4 and 8, into LDS; then the merges 16 .. NPAD.  The sorted
// keys 8 tid .. 8 tid + 7 of the chunk are left in r.
template <uint32_t NPAD>
__device__ __forceinline__ void sort_chunk(uint64_t* keys, uint32_t tid,
                                           const double* __restrict__ row,
                                           uint64_t n, uint32_t gbase,
                                           uint64_t (&r)[8]) {
    const uint32_t g0 = gbase + 8 * tid;
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m)
        r[m] = g0 + m < n ? ostat::key_of(row[g0 + m]) : ostat::KEY_PAD;
#pragma unroll
    for (uint32_t k = 2; k <= 8; k <<= 1) {
#pragma unroll
        for (uint32_t s = k >> 1; s >= 1; s >>= 1) {
#pragma unroll
            for (uint32_t m = 0; m < 8; ++m)
                if (!(m & s)) cmpx(r[m], r[m | s], ((g0 + m) & k) == 0);
        }
    }
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) keys[slot(8 * tid + m)] = r[m];
    __syncthreads();
    for (uint32_t lk = 4; (1u << lk) <= NPAD; ++lk)
        lds_merge(keys, tid, lk - 1, gbase, 1u << lk, r, (2u << lk) <= NPAD);
}

template <uint32_t NPAD>
__global__ __launch_bounds__(NPAD / 8) void ostat_block_kernel(
    const double* __restrict__ x, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, uint32_t skip,
    double* __restrict__ n_out, uint64_t* __restrict__ ws,
    uint64_t* __restrict__ sorted) {
    static_assert(NPAD >= 1024 && NPAD <= BM, "64 to 1024 threads");
    __shared__ uint64_t keys[NPAD];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x;
    const uint64_t n = corr::effective_n(N, len, t, skip);
    uint64_t r[8];
    sort_chunk<NPAD>(keys, tid, x + t * stride + skip, n, 0, r);
    if (tid == 0) n_out[t] = (double)n;
    store_sorted<8>(r, t, 8 * tid, NPAD, N, ws, sorted);
    fill_tail(t, tid, NPAD / 8, NPAD, N, sorted);
}

// ---- chunk tier ------------------------------------------------------------

// block = chunk c of row t, keys to the workspace
__global__ __launch_bounds__(BM / 8) void ostat_chunk_sort_kernel(
    const double* __restrict__ x, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, uint32_t skip, uint32_t lnpad,
    double* __restrict__ n_out, uint64_t* __restrict__ ws) {
    __shared__ uint64_t keys[BM];
    const uint32_t tid = threadIdx.x;
    const uint32_t lchunks = lnpad - LBM;
    const uint64_t t = blockIdx.x >> lchunks;
    const uint32_t gbase = (blockIdx.x & ((1u << lchunks) - 1)) << LBM;
    const uint64_t n = corr::effective_n(N, len, t, skip);
    uint64_t r[8];
    sort_chunk<BM>(keys, tid, x + t * stride + skip, n, gbase, r);
    if (tid == 0 && gbase == 0) n_out[t] = (double)n;
    uint64_t* out = ws + (t << lnpad) + gbase + 8 * tid;
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) out[m] = r[m];
}

// NL levels of merge size k whose lowest stride is 2^ls0 >= BM.  Thread w
// of a row takes the 2^NL keys base + m * 2^ls0, base = w with NL zero bits
// inserted at ls0.  total = T * n_pad / 2^NL threads.
template <int NL>
__global__ __launch_bounds__(FLAT_WG) void ostat_global_merge_kernel(
    uint64_t* __restrict__ ws, uint64_t total, uint32_t lnpad, uint32_t ls0,
    uint32_t k) {
    constexpr uint32_t NK = 1u << NL;
    const uint64_t g = (uint64_t)blockIdx.x * FLAT_WG + threadIdx.x;
    if (g >= total) return;
    const uint32_t lper = lnpad - NL;
    const uint64_t t = g >> lper;
    const uint32_t w = (uint32_t)(g & ((1ull << lper) - 1));
    const uint32_t base = ((w >> ls0) << (ls0 + NL)) | (w & ((1u << ls0) - 1));
    uint64_t* p = ws + (t << lnpad) + base;
    uint64_t r[NK];
#pragma unroll
    for (uint32_t m = 0; m < NK; ++m) r[m] = p[(uint64_t)m << ls0];
    const bool asc = (base & k) == 0;
#pragma unroll
    for (uint32_t bit = NK >> 1; bit >= 1; bit >>= 1) {
#pragma unroll
        for (uint32_t m = 0; m < NK; ++m)
            if (!(m & bit)) cmpx(r[m], r[m | bit], asc);
    }
#pragma unroll
    for (uint32_t m = 0; m < NK; ++m) p[(uint64_t)m << ls0] = r[m];
}

// Strides BM / 2 .. 1 of merge size k on chunk c of row t.  The last merge
// of the sort (k == n_pad) stores doubles instead of keys, into the
// workspace only when an epilogue kernel will read it (keep_ws).
__global__ __launch_bounds__(BM / 8) void ostat_chunk_merge_kernel(
    uint64_t* __restrict__ ws, uint32_t lnpad, uint32_t k, uint64_t N,
    bool keep_ws, uint64_t* __restrict__ sorted) {
    __shared__ uint64_t keys[BM];
    const uint32_t tid = threadIdx.x;
    const uint32_t lchunks = lnpad - LBM;
    const uint64_t t = blockIdx.x >> lchunks;
    const uint32_t gbase = (blockIdx.x & ((1u << lchunks) - 1)) << LBM;
    uint64_t* chunk = ws + (t << lnpad) + gbase;
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) {
        const uint32_t i = tid + m * (BM / 8);
        keys[slot(i)] = chunk[i];
    }
    __syncthreads();
    uint64_t r[8];
    lds_merge(keys, tid, LBM - 1, gbase, k, r, false);
    if (k >> lnpad) {  // k == n_pad
        store_sorted<8>(r, t, gbase + 8 * tid, 1ull << lnpad, N,
                        keep_ws ? ws : nullptr, sorted);
        if (gbase == 0) fill_tail(t, tid, BM / 8, 1ull << lnpad, N, sorted);
    } else {
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m) chunk[8 * tid + m] = r[m];
    }
}

// ---- epilogues -------------------------------------------------------------

__global__ __launch_bounds__(FLAT_WG) void ostat_quantile_kernel(
    const double* __restrict__ ws, uint64_t T, uint64_t N, uint64_t n_pad,
    const uint32_t* __restrict__ len, uint32_t skip, QList ql, uint32_t nq,
    double* __restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * FLAT_WG + threadIdx.x;
    if (idx >= T * nq) return;
    const uint64_t t = idx / nq;
    const uint32_t i = (uint32_t)(idx - t * nq);
    out[idx] = ostat::quantile_sorted(ws + t * n_pad,
                                      corr::effective_n(N, len, t, skip),
                                      ql.q[i]);
}

// first index in [0, n) whose bin exceeds b, n if none
__device__ __forceinline__ uint64_t first_above(const double* xs, uint64_t n,
                                                double lo, double w,
                                                uint32_t nbins, uint32_t b) {
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

__global__ __launch_bounds__(FLAT_WG) void ostat_hist_kernel(
    const double* __restrict__ ws, uint64_t T, uint64_t N, uint64_t n_pad,
    const uint32_t* __restrict__ len, uint32_t skip, uint32_t nbins,
    int64_t* __restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * FLAT_WG + threadIdx.x;
    if (idx >= T * nbins) return;
    const uint64_t t = idx / nbins;
    const uint32_t b = (uint32_t)(idx - t * nbins);
    const uint64_t n = corr::effective_n(N, len, t, skip);
    const double* xs = ws + t * n_pad;
    int64_t count = 0;
    if (ostat::hist_row_ok(xs, n)) {
        const double lo = xs[0];
        const double w = ostat::hist_width(lo, xs[n - 1], nbins);
        const uint64_t hi_edge = first_above(xs, n, lo, w, nbins, b);
        const uint64_t lo_edge =
            b ? first_above(xs, n, lo, w, nbins, b - 1) : 0;
        count = (int64_t)(hi_edge - lo_edge);
    }
    out[idx] = count;
}

template <int K>
void launch_wave(uint64_t T, const double* x, uint64_t N, uint64_t stride,
                 const uint32_t* len, uint32_t skip, double* n_out,
                 uint64_t* ws, uint64_t* sorted) {
    const uint64_t blocks = (T + WAVE_WG / WAVE - 1) / (WAVE_WG / WAVE);
    hipLaunchKernelGGL(ostat_wave_kernel<K>, dim3((uint32_t)blocks),
                       dim3(WAVE_WG), 0, 0, x, T, N, stride, len, skip, n_out,
                       ws, sorted);
}

template <uint32_t NPAD>
void launch_block(uint64_t T, const double* x, uint64_t N, uint64_t stride,
                  const uint32_t* len, uint32_t skip, double* n_out,
                  uint64_t* ws, uint64_t* sorted) {
    hipLaunchKernelGGL(ostat_block_kernel<NPAD>, dim3((uint32_t)T),
                       dim3(NPAD / 8), 0, 0, x, N, stride, len, skip, n_out,
                       ws, sorted);
}

int launch_global_merge(int nl, uint64_t* ws, uint64_t T, uint32_t lnpad,
                        uint32_t ls0, uint32_t k) {
    const uint64_t total = T << (lnpad - (uint32_t)nl);
    const dim3 grid((uint32_t)((total + FLAT_WG - 1) / FLAT_WG));
    if (nl == 1)
        hipLaunchKernelGGL(ostat_global_merge_kernel<1>, grid, dim3(FLAT_WG),
                           0, 0, ws, total, lnpad, ls0, k);
    else if (nl == 2)
        hipLaunchKernelGGL(ostat_global_merge_kernel<2>, grid, dim3(FLAT_WG),
                           0, 0, ws, total, lnpad, ls0, k);
    else
        hipLaunchKernelGGL(ostat_global_merge_kernel<3>, grid, dim3(FLAT_WG),
                           0, 0, ws, total, lnpad, ls0, k);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Device pointers: x[T][stride] (the last row may end after N values),
// len[T] or null, n_out[T]; sorted_out[T][N], quant_out[T][nq] and
// hist_out[T][nbins] may each be null and are then neither computed nor
// stored.  q[nq] is a HOST array (it is checked here and travels as a
// kernel argument).  elapsed_ms (nullable) is the kernels alone.
int cimba_order_stats_gpu_dev(const double* x, uint64_t T, uint64_t N,
                              uint64_t stride, const uint32_t* len,
                              uint32_t skip, const double* q, uint32_t nq,
                              uint32_t nbins, double* n_out,
                              double* sorted_out, double* quant_out,
                              int64_t* hist_out, double* elapsed_ms) {
    if (!ostat::args_ok(T, N, stride, q, nq, nbins) ||
        !ostat::grid_ok(T, N, skip))
        return (int)hipErrorInvalidValue;
    const uint64_t n_pad = ostat::pad_len(N, skip);
    uint32_t lnpad = 0;
    while ((1ull << lnpad) < n_pad) ++lnpad;
    const bool want_q = quant_out && nq, want_h = hist_out && nbins;
    const bool chunked = n_pad > BM;
    // the workspace holds keys between the chunk tier's launches and the
    // sorted doubles that the epilogue kernels read
    cmb_hip::DevBuf<uint64_t> d_ws;
    if (chunked || want_q || want_h) HIP_TRY(d_ws.alloc(T * n_pad));
    uint64_t* ws = d_ws.get();
    uint64_t* sorted = reinterpret_cast<uint64_t*>(sorted_out);
    QList ql = {};
    for (uint32_t i = 0; i < nq; ++i) ql.q[i] = q[i];

    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    if (!chunked) {
        switch (n_pad) {
            case 64:
                launch_wave<1>(T, x, N, stride, len, skip, n_out, ws, sorted);
                break;
            case 128:
                launch_wave<2>(T, x, N, stride, len, skip, n_out, ws, sorted);
                break;
            case 256:
                launch_wave<4>(T, x, N, stride, len, skip, n_out, ws, sorted);
                break;
            case 512:
                launch_wave<8>(T, x, N, stride, len, skip, n_out, ws, sorted);
                break;
            case 1024:
                launch_block<1024>(T, x, N, stride, len, skip, n_out, ws,
                                   sorted);
                break;
            case 2048:
                launch_block<2048>(T, x, N, stride, len, skip, n_out, ws,
                                   sorted);
                break;
            case 4096:
                launch_block<4096>(T, x, N, stride, len, skip, n_out, ws,
                                   sorted);
                break;
            default:
                launch_block<8192>(T, x, N, stride, len, skip, n_out, ws,
                                   sorted);
                break;
        }
        HIP_TRY(hipGetLastError());
    } else {
        const dim3 chunks((uint32_t)(T << (lnpad - LBM)));
        hipLaunchKernelGGL(ostat_chunk_sort_kernel, chunks, dim3(BM / 8), 0, 0,
                           x, N, stride, len, skip, lnpad, n_out, ws);
        HIP_TRY(hipGetLastError());
        for (uint32_t lk = LBM + 1; lk <= lnpad; ++lk) {
            // global strides 2^(lk-1) .. 2^LBM: the odd one or two levels
            // first, then three per launch
            uint32_t l = lk - 1;
            const uint32_t rem = (lk - LBM) % 3;
            if (rem) {
                HIP_TRY(launch_global_merge((int)rem, ws, T, lnpad,
                                            l - rem + 1, 1u << lk));
                l -= rem;
            }
            for (; l >= LBM; l -= 3)
                HIP_TRY(launch_global_merge(3, ws, T, lnpad, l - 2, 1u << lk));
            hipLaunchKernelGGL(ostat_chunk_merge_kernel, chunks, dim3(BM / 8),
                               0, 0, ws, lnpad, 1u << lk, N, want_q || want_h,
                               lk == lnpad ? sorted : nullptr);
            HIP_TRY(hipGetLastError());
        }
    }
    if (want_q) {
        const uint64_t blocks = (T * nq + FLAT_WG - 1) / FLAT_WG;
        hipLaunchKernelGGL(ostat_quantile_kernel, dim3((uint32_t)blocks),
                           dim3(FLAT_WG), 0, 0,
                           reinterpret_cast<const double*>(ws), T, N, n_pad,
                           len, skip, ql, nq, quant_out);
        HIP_TRY(hipGetLastError());
    }
    if (want_h) {
        const uint64_t blocks = (T * nbins + FLAT_WG - 1) / FLAT_WG;
        hipLaunchKernelGGL(ostat_hist_kernel, dim3((uint32_t)blocks),
                           dim3(FLAT_WG), 0, 0,
                           reinterpret_cast<const double*>(ws), T, N, n_pad,
                           len, skip, nbins, hist_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;
    return 0;
}

// Host arrays in and out: host_x[T][stride] (T - 1 full rows and N values
// of the last), host_len[T] or null; n_out[T] and the outputs of
// cimba_order_stats_gpu_dev, of which only those asked for are allocated on
// the device and downloaded.
int cimba_order_stats_gpu(const double* host_x, uint64_t T, uint64_t N,
                          uint64_t stride, const uint32_t* host_len,
                          uint32_t skip, const double* q, uint32_t nq,
                          uint32_t nbins, int device, double* n_out,
                          double* sorted_out, double* quant_out,
                          int64_t* hist_out, double* elapsed_ms) {
    if (!ostat::args_ok(T, N, stride, q, nq, nbins) ||
        !ostat::grid_ok(T, N, skip))
        return (int)hipErrorInvalidValue;
    HIP_TRY(hipSetDevice(device));
    const size_t nx = (size_t)((T - 1) * stride + N);
    const bool want_s = sorted_out && N, want_q = quant_out && nq,
               want_h = hist_out && nbins;
    cmb_hip::DevBuf<double> d_x, d_n, d_sorted, d_quant;
    cmb_hip::DevBuf<int64_t> d_hist;
    cmb_hip::DevBuf<uint32_t> d_len;
    HIP_TRY(d_x.alloc(nx ? nx : 1));
    HIP_TRY(d_n.alloc(T));
    if (nx) HIP_TRY(d_x.upload(host_x, nx));
    if (host_len) {
        HIP_TRY(d_len.alloc(T));
        HIP_TRY(d_len.upload(host_len, T));
    }
    if (want_s) HIP_TRY(d_sorted.alloc((size_t)(T * N)));
    if (want_q) HIP_TRY(d_quant.alloc((size_t)T * nq));
    if (want_h) HIP_TRY(d_hist.alloc((size_t)T * nbins));
    HIP_TRY(cimba_order_stats_gpu_dev(
        d_x.get(), T, N, stride, d_len.get(), skip, q, nq, nbins, d_n.get(),
        d_sorted.get(), d_quant.get(), d_hist.get(), elapsed_ms));
    HIP_TRY(d_n.download(n_out, T));
    if (want_s) HIP_TRY(d_sorted.download(sorted_out, (size_t)(T * N)));
    if (want_q) HIP_TRY(d_quant.download(quant_out, (size_t)T * nq));
    if (want_h) HIP_TRY(d_hist.download(hist_out, (size_t)T * nbins));
    return 0;
}

}  // extern "C"
