// Steady-state kernels (include/cimba/steadystate.hpp): the MSER-m cut and
// the batch-means doubling ladder of a dense device array x[T][stride], one
// row per trial, any row length.
//
// Both kernels walk a row in chunks of 256 level-0 batch means and come in
// two tiers, one template: W = 1 gives a row to one wave, four rows to a
// workgroup; W = BLOCK_WAVES gives a row to a workgroup whose waves take W
// consecutive chunks per round.  Only the few doubles named below cross a
// chunk or a wave, so a row of any length runs in the same registers.
//
//   load_chunk    64 batches at a time: a row-contiguous (coalesced) load
//                 into LDS at a stride of m | 1 doubles, then lane l sums its
//                 own m values left to right, conflict-free.  The four means
//                 a lane ends up holding are consecutive (chunk index
//                 4 l + r), which costs one more trip through LDS and buys a
//                 scan of one cross-lane pass per 256 means instead of four.
//   mser_kernel   a suffix scan of (count, mean, M2) under Moments2::merge,
//                 walking from the row's end.  Per chunk: the lane folds its
//                 four means, the lane totals are scanned across the wave
//                 with shuffles, the chunk totals of a round meet in LDS, and
//                 each wave rescans its own registers with everything behind
//                 it as carry-in, keeping a running (best stat, d, mean).
//                 The carry between rounds is one triple.  Chunks that lie
//                 wholly above dmax are only summarised.
//   ladder_kernel two sweeps over the row: per-level sums, then with each
//                 level's own mean the centred sse, c1 and dsq.  (The
//                 alternative, one sweep of merged triples with a cross-
//                 product term, would make the GPU's sums a different formula
//                 from the host's two passes; the second sweep re-reads a row
//                 that the first one has just pulled through the cache.)
//                 Chunks start at multiples of 256 means, so levels 0..8 of
//                 a chunk are a whole subtree: level 0 and 1 in the lane's
//                 registers, each further level the pairwise mean with the
//                 lane 2^(l-3) further on.  Two things cross a seam.  For
//                 c1 and dsq, the last mean of every level of the chunk
//                 before: left in LDS for the lane that holds the first mean
//                 of the next chunk.  For levels 9 and up, the chunk's single
//                 level-8 mean: one thread pairs them like a binary counter,
//                 an odd one waiting in LDS for its partner.
//
// No atomics, every sum in a fixed order: results are bit-identical from
// run to run.  Nothing is read outside [first, first + k * m) of a row.
#include <hip/hip_runtime.h>

#include "../include/cimba/steadystate.hpp"
#include "hip_host.hpp"

namespace {

namespace ss = cmb::sstat;
using cmb::Moments2;

constexpr uint32_t WAVE = ss::WAVE;
constexpr uint32_t REGS = ss::REGS;
constexpr uint32_t CHUNK = ss::CHUNK;
constexpr uint32_t STAGE_DOUBLES = WAVE * ss::stage_stride(ss::M_STAGE);
constexpr uint32_t YM_DOUBLES = WAVE * (REGS + 1);
static_assert(STAGE_DOUBLES + YM_DOUBLES == ss::lds_doubles(), "LDS budget");
constexpr uint32_t NLOW = ss::CHUNK_LOG + 1;         // levels inside a chunk
constexpr uint32_t NHIGH = ss::MAX_LEVELS - NLOW;    // levels across chunks
static_assert(REGS == 4, "the ladder pairs a lane's means by hand");

template <int W>
struct Shape {
    static constexpr int GROUPS = W == 1 ? (int)ss::WAVE_ROWS : 1;  // rows
    static constexpr int WAVES = GROUPS * W;
    static constexpr int THREADS = WAVES * (int)WAVE;
};

// LDS written by some lanes of a wave and read by others of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the waves that share a row
template <int W>
__device__ __forceinline__ void group_sync() {
    if (W == 1) wave_sync();
    else __syncthreads();
}

__device__ __forceinline__ Moments2 shfl_down(const Moments2& a, int off) {
    return Moments2{__shfl_down(a.n, off), __shfl_down(a.mean, off),
                    __shfl_down(a.m2, off)};
}

// Level-0 batch means c * 256 .. c * 256 + 255 of a row of k means: lane l
// gets means 4 l .. 4 l + 3 of the chunk in y, 0.0 at and past k.
__device__ __forceinline__ void load_chunk(const double* __restrict__ row,
                                           uint64_t k, uint32_t m, uint64_t c,
                                           uint32_t lane, double* stage,
                                           double* ym, double (&y)[REGS]) {
    const uint32_t ms = ss::stage_stride(m);
    const uint32_t dq = WAVE / m, dr = WAVE % m;
    wave_sync();  // the chunk before is out of ym
    for (uint32_t s = 0; s < REGS; ++s) {
        const uint64_t jb = c * CHUNK + s * WAVE;
        double mean = 0.0;
        if (jb < k) {  // wave-uniform
            const uint64_t left = k - jb;
            const uint32_t nb = left < WAVE ? (uint32_t)left : WAVE;
            const double* src = row + jb * m;
            if (m <= ss::M_STAGE) {
                const uint32_t cnt = nb * m;
                // p = q * m + r without a division per element
                uint32_t q = lane / m, r = lane % m;
                for (uint32_t p = lane; p < cnt; p += WAVE) {
                    stage[q * ms + r] = src[p];
                    q += dq;
                    r += dr;
                    if (r >= m) {
                        r -= m;
                        ++q;
                    }
                }
                wave_sync();
                if (lane < nb) mean = ss::batch_mean(stage + lane * ms, m);
            } else if (lane < nb) {
                mean = ss::batch_mean(src + (uint64_t)lane * m, m);
            }
        }
        const uint32_t e = s * WAVE + lane;
        ym[(e / REGS) * (REGS + 1) + e % REGS] = mean;
        wave_sync();  // the tile is free again
    }
#pragma unroll
    for (uint32_t r = 0; r < REGS; ++r) y[r] = ym[lane * (REGS + 1) + r];
}

// ---- MSER -----------------------------------------------------------------

template <int W>
__global__ __launch_bounds__(Shape<W>::THREADS) void mser_kernel(
    const double* __restrict__ x, uint64_t T, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, const uint32_t* __restrict__ skip,
    uint32_t m, uint64_t curve_w, uint32_t* __restrict__ n_out,
    uint32_t* __restrict__ k_out, uint32_t* __restrict__ d_out,
    uint32_t* __restrict__ cut_out, double* __restrict__ stat_out,
    double* __restrict__ mean_out, double* __restrict__ curve_out) {
    constexpr int G = Shape<W>::GROUPS;
    __shared__ double stage[Shape<W>::WAVES][STAGE_DOUBLES];
    __shared__ double ym[Shape<W>::WAVES][YM_DOUBLES];
    __shared__ double tot[G][W][3];
    __shared__ double best_sm[G][W][2];
    __shared__ uint32_t best_d[G][W];
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t wave = threadIdx.x / WAVE;
    const uint32_t g = wave / W, w = wave % W;
    const uint64_t t = (uint64_t)blockIdx.x * G + g;
    if (t >= T) return;  // a whole row's waves; the W = 1 tier has no barrier
    const ss::Row rw = ss::row_of(N, len, skip, t);
    const double* row = x + t * stride + rw.first;
    const uint64_t k = rw.n / m, dmax = k / 2;
    const uint64_t nchunks = (k + CHUNK - 1) / CHUNK;
    const uint64_t rounds = (nchunks + W - 1) / W;
    double* curve = curve_out ? curve_out + t * curve_w : nullptr;
    if (curve)  // the scan writes d = 0 .. dmax of a row that has means
        for (uint64_t d = (k ? dmax + 1 : 0) + w * WAVE + lane; d < curve_w;
             d += W * WAVE)
            curve[d] = ss::nan_value();

    Moments2 carry, one;  // carry: everything behind this round
    carry.reset();
    ss::Best best;
    best.reset();
    for (uint64_t rho = 0; rho < rounds; ++rho) {
        // wave 0 takes the round's last chunk: the walk runs from the end
        const uint64_t back = rho * W + w;
        const bool have = back < nchunks;
        const uint64_t c = have ? nchunks - 1 - back : 0;
        const uint64_t j0 = c * CHUNK + (uint64_t)lane * REGS;
        double y[REGS] = {0.0, 0.0, 0.0, 0.0};
        Moments2 incl;  // this lane's means and those of the lanes after it
        incl.reset();
        if (have) {
            load_chunk(row, k, m, c, lane, stage[wave], ym[wave], y);
#pragma unroll
            for (int r = REGS - 1; r >= 0; --r)
                if (j0 + r < k) {
                    one.set_one(y[r]);
                    incl.merge(one);
                }
#pragma unroll
            for (int off = 1; off < (int)WAVE; off <<= 1) {
                const Moments2 o = shfl_down(incl, off);
                if (lane + off < WAVE) incl.merge(o);
            }
        }
        Moments2 excl = shfl_down(incl, 1);
        if (lane == WAVE - 1) excl.reset();
        if (lane == 0) {
            tot[g][w][0] = incl.n;
            tot[g][w][1] = incl.mean;
            tot[g][w][2] = incl.m2;
        }
        group_sync<W>();
        // every wave folds the round's totals in the same order, so all of
        // them carry the same bits into the next round
        Moments2 acc = carry;
#pragma unroll
        for (int v = 0; v < W; ++v) {
            if (v == (int)w) acc = carry;
            carry.merge(Moments2{tot[g][v][0], tot[g][v][1], tot[g][v][2]});
        }
        if (have && c * CHUNK <= dmax) {
            acc.merge(excl);
#pragma unroll
            for (int r = REGS - 1; r >= 0; --r) {
                const uint64_t j = j0 + r;
                if (j < k) {
                    one.set_one(y[r]);
                    acc.merge(one);
                    if (j <= dmax) {
                        const double s = acc.m2 / (acc.n * acc.n);
                        best.take(s, acc.mean, (uint32_t)j);
                        if (curve) curve[j] = s;
                    }
                }
            }
        }
        group_sync<W>();  // tot is read
    }

#pragma unroll
    for (int off = 1; off < (int)WAVE; off <<= 1)
        best.take(__shfl_xor(best.stat, off), __shfl_xor(best.mean, off),
                  __shfl_xor(best.d, off));
    if (W > 1) {
        if (lane == 0) {
            best_sm[g][w][0] = best.stat;
            best_sm[g][w][1] = best.mean;
            best_d[g][w] = best.d;
        }
        __syncthreads();
        for (int v = 0; v < W; ++v)
            best.take(best_sm[g][v][0], best_sm[g][v][1], best_d[g][v]);
    }
    if (w == 0 && lane == 0) {
        n_out[t] = (uint32_t)rw.n;
        k_out[t] = (uint32_t)k;
        d_out[t] = best.d;
        cut_out[t] = skip[t] + best.d * m;
        stat_out[t] = best.stat;
        mean_out[t] = best.mean;
    }
}

// ---- batch-means ladder ---------------------------------------------------

// per-level state of levels 9 and up, one thread's, in LDS
enum { HI_PEND, HI_PREV, HI_MEAN, HI_SSE, HI_C1, HI_DSQ, HI_FIELDS };

// Chunk number cnt (counted from 1) has delivered its level-8 mean z: pair
// it upwards.  Level 8 + h spans 2^h chunks; a mean with an even index waits
// in HI_PEND for the odd one.  Pass 0 sums each level's means into HI_MEAN,
// pass 1 (HI_MEAN then holds the mean) takes the centred sums.
template <int PASS>
__device__ __forceinline__ void cascade(double (*hi)[HI_FIELDS], double z,
                                        uint64_t cnt, uint32_t levels) {
    double v = z;
    for (uint32_t l = NLOW; l < levels; ++l) {
        double* s = hi[l - NLOW];
        const uint32_t h = l - NLOW;
        if ((cnt >> h) & 1) {
            s[HI_PEND] = v;
            return;
        }
        v = (s[HI_PEND] + v) / 2.0;
        if (PASS == 0) {
            s[HI_MEAN] += v;
        } else {
            const double mu = s[HI_MEAN], a = v - mu;
            s[HI_SSE] += a * a;
            if ((cnt >> (h + 1)) > 1) {  // not the level's first mean
                const double p = s[HI_PREV];
                s[HI_C1] += (p - mu) * a;
                s[HI_DSQ] += (v - p) * (v - p);
            }
            s[HI_PREV] = v;
        }
    }
}

// One pass over the row.  PASS 0: a[0][l] += the level-l means.  PASS 1:
// a[0..2][l] += the terms of sse, c1, dsq, centred on mu[l].  Each lane adds
// what it holds; the caller folds the lanes.
template <int W, int PASS>
__device__ __forceinline__ void ladder_sweep(
    const double* __restrict__ row, uint64_t k, uint32_t m, uint32_t levels,
    uint64_t rounds, uint32_t lane, uint32_t w, double* stage,
    double* ym, double (*slot)[NLOW], double (*hi)[HI_FIELDS],
    const double (&mu)[NLOW], double (&a)[3][NLOW]) {
    const uint32_t low = levels < NLOW ? levels : NLOW;
    // one value of level L at global index g, its successor nxt if has_next
    auto term = [&](int L, double cur, double nxt, uint64_t g, bool has_next) {
        const uint64_t kl = k >> L;
        if (g >= kl) return;
        if (PASS == 0) {
            a[0][L] += cur;
            return;
        }
        const double d = cur - mu[L];
        a[0][L] += d * d;
        if (has_next && g + 1 < kl) {
            a[1][L] += d * (nxt - mu[L]);
            a[2][L] += (nxt - cur) * (nxt - cur);
        }
    };
    for (uint64_t rho = 0; rho < rounds; ++rho) {
        const uint64_t c = rho * W + w;
        double first[NLOW] = {};  // this lane's (first) mean of every level
        if (c * CHUNK < k) {  // wave-uniform
            double y[REGS];
            load_chunk(row, k, m, c, lane, stage, ym, y);
            const bool more = lane + 1 < WAVE;
            const uint64_t g0 = c * CHUNK + (uint64_t)lane * REGS;
            const double ny = __shfl_down(y[0], 1);
            term(0, y[0], y[1], g0, true);
            term(0, y[1], y[2], g0 + 1, true);
            term(0, y[2], y[3], g0 + 2, true);
            term(0, y[3], ny, g0 + 3, more);
            first[0] = y[0];
            if (lane == WAVE - 1) slot[w + 1][0] = y[3];
            double v = 0.0;
            if (low > 1) {
                const double u0 = (y[0] + y[1]) / 2.0;
                const double u1 = (y[2] + y[3]) / 2.0;
                const double nu = __shfl_down(u0, 1);
                term(1, u0, u1, g0 / 2, true);
                term(1, u1, nu, g0 / 2 + 1, more);
                first[1] = u0;
                if (lane == WAVE - 1) slot[w + 1][1] = u1;
                v = (u0 + u1) / 2.0;
            }
#pragma unroll
            for (int L = 2; L < (int)NLOW; ++L) {
                if (L < (int)low) {  // uniform
                    // lanes that are multiples of step hold level L
                    const uint32_t step = 1u << (L - 2);
                    const double nv = __shfl_down(v, step);
                    if (lane % step == 0)
                        term(L, v, nv, c * (CHUNK >> L) + lane / step,
                             lane + step < WAVE);
                    first[L] = v;
                    if (lane == WAVE - step) slot[w + 1][L] = v;
                    v = (v + nv) / 2.0;
                }
            }
        }
        group_sync<W>();
        if (lane == 0 && c > 0 && PASS == 1) {
            // the pair across the seam: the chunk before ended every level
            // that has a mean here
#pragma unroll
            for (int L = 0; L < (int)NLOW; ++L)
                if (L < (int)low && c * (CHUNK >> L) < (k >> L)) {
                    const double p = slot[w][L];
                    a[1][L] += (p - mu[L]) * (first[L] - mu[L]);
                    a[2][L] += (first[L] - p) * (first[L] - p);
                }
        }
        if (lane == 0 && w == 0 && levels > NLOW)
            for (int v = 0; v < W; ++v) {
                const uint64_t cv = rho * W + v;
                if (cv < (k >> ss::CHUNK_LOG))
                    cascade<PASS>(hi, slot[v + 1][NLOW - 1], cv + 1, levels);
            }
        group_sync<W>();
        // the round's last chunk is the next round's predecessor
        if (lane == 0 && w == W - 1)
            for (uint32_t L = 0; L < NLOW; ++L) slot[0][L] = slot[W][L];
    }
}

// Sum v over the lanes of a wave, then over the W waves of a row in wave
// order; every thread of the row gets the same bits.
template <int W>
__device__ __forceinline__ double row_sum(double v, uint32_t lane, uint32_t w,
                                          double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (W > 1) {
        __syncthreads();  // red is free
        if (lane == 0) red[w] = v;
        __syncthreads();
        v = 0.0;
        for (int i = 0; i < W; ++i) v += red[i];
    }
    return v;
}

template <int W>
__global__ __launch_bounds__(Shape<W>::THREADS) void ladder_kernel(
    const double* __restrict__ x, uint64_t T, uint64_t N, uint64_t stride,
    const uint32_t* __restrict__ len, const uint32_t* __restrict__ skip,
    uint32_t m, uint32_t levels, double* __restrict__ k_out,
    double* __restrict__ mean_out, double* __restrict__ sse_out,
    double* __restrict__ c1_out, double* __restrict__ dsq_out) {
    constexpr int G = Shape<W>::GROUPS;
    __shared__ double stage[Shape<W>::WAVES][STAGE_DOUBLES];
    __shared__ double ym[Shape<W>::WAVES][YM_DOUBLES];
    __shared__ double slot[G][W + 1][NLOW];
    __shared__ double hi[G][NHIGH][HI_FIELDS];
    __shared__ double red[G][W];
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t wave = threadIdx.x / WAVE;
    const uint32_t g = wave / W, w = wave % W;
    const uint64_t t = (uint64_t)blockIdx.x * G + g;
    if (t >= T) return;  // a whole row's waves; the W = 1 tier has no barrier
    const ss::Row rw = ss::row_of(N, len, skip, t);
    const double* row = x + t * stride + rw.first;
    const uint64_t k = rw.n / m;
    const uint64_t nchunks = (k + CHUNK - 1) / CHUNK;
    const uint64_t rounds = (nchunks + W - 1) / W;
    const uint32_t low = levels < NLOW ? levels : NLOW;
    const bool owner = w == 0 && lane == 0;  // the thread that owns hi[g]
    if (owner)
        for (uint32_t h = 0; h < NHIGH; ++h)
            for (uint32_t f = 0; f < HI_FIELDS; ++f) hi[g][h][f] = 0.0;

    double mu[NLOW], a[3][NLOW];
#pragma unroll
    for (uint32_t L = 0; L < NLOW; ++L) {
        mu[L] = 0.0;
        a[0][L] = a[1][L] = a[2][L] = 0.0;
    }
    ladder_sweep<W, 0>(row, k, m, levels, rounds, lane, w, stage[wave],
                       ym[wave], slot[g], hi[g], mu, a);
#pragma unroll
    for (uint32_t L = 0; L < NLOW; ++L) {
        if (L < low) {
            const double s = row_sum<W>(a[0][L], lane, w, red[g]);
            mu[L] = (k >> L) ? s / (double)(k >> L) : ss::nan_value();
        }
        a[0][L] = 0.0;
    }
    if (owner)
        for (uint32_t l = NLOW; l < levels; ++l) {
            double* s = hi[g][l - NLOW];
            s[HI_MEAN] = (k >> l) ? s[HI_MEAN] / (double)(k >> l)
                                  : ss::nan_value();
        }
    ladder_sweep<W, 1>(row, k, m, levels, rounds, lane, w, stage[wave],
                       ym[wave], slot[g], hi[g], mu, a);
    const uint64_t o = t * levels;
#pragma unroll
    for (uint32_t L = 0; L < NLOW; ++L)
        if (L < low) {
            const double sse = row_sum<W>(a[0][L], lane, w, red[g]);
            const double c1 = row_sum<W>(a[1][L], lane, w, red[g]);
            const double dsq = row_sum<W>(a[2][L], lane, w, red[g]);
            if (owner) {
                k_out[o + L] = (double)(k >> L);
                mean_out[o + L] = mu[L];
                sse_out[o + L] = sse;
                c1_out[o + L] = c1;
                dsq_out[o + L] = dsq;
            }
        }
    if (owner)
        for (uint32_t l = NLOW; l < levels; ++l) {
            const double* s = hi[g][l - NLOW];
            k_out[o + l] = (double)(k >> l);
            mean_out[o + l] = s[HI_MEAN];
            sse_out[o + l] = s[HI_SSE];
            c1_out[o + l] = s[HI_C1];
            dsq_out[o + l] = s[HI_DSQ];
        }
}

template <int W>
uint32_t blocks_for(uint64_t T) {
    return (uint32_t)((T + Shape<W>::GROUPS - 1) / Shape<W>::GROUPS);
}

// the inputs of both entry points on the device
struct DevRows {
    cmb_hip::DevBuf<double> x;
    cmb_hip::DevBuf<uint32_t> len, skip;
    int upload(const double* host_x, uint64_t T, uint64_t N, uint64_t stride,
               const uint32_t* host_len, const uint32_t* host_skip) {
        const size_t nx = (size_t)((T - 1) * stride + N);
        HIP_TRY(x.alloc(nx ? nx : 1));
        if (nx) HIP_TRY(x.upload(host_x, nx));
        if (host_len) {
            HIP_TRY(len.alloc(T));
            HIP_TRY(len.upload(host_len, T));
        }
        HIP_TRY(skip.alloc(T));
        return skip.upload(host_skip, T);
    }
};

}  // namespace

extern "C" {

// Host arrays in and out: host_x[T][stride] (T - 1 full rows and N values of
// the last), host_len[T] or null, host_skip[T]; n, k, d, cut: uint32 [T];
// stat, mean: double [T]; curve: null or double [T][curve_width(N, m)].
// elapsed_ms (nullable) is the kernel alone.
int cimba_mser_gpu(const double* host_x, uint64_t T, uint64_t N,
                   uint64_t stride, const uint32_t* host_len,
                   const uint32_t* host_skip, uint32_t m, int device,
                   uint32_t* n_out, uint32_t* k_out, uint32_t* d_out,
                   uint32_t* cut_out, double* stat_out, double* mean_out,
                   double* curve_out, double* elapsed_ms) {
    if (!ss::args_ok(T, N, stride, m, 1) || !ss::grid_ok(T, N))
        return (int)hipErrorInvalidValue;
    HIP_TRY(hipSetDevice(device));
    DevRows in;
    HIP_TRY(in.upload(host_x, T, N, stride, host_len, host_skip));
    const uint64_t cw = ss::curve_width(N, m);
    cmb_hip::DevBuf<uint32_t> d_u;  // n, k, d, cut
    cmb_hip::DevBuf<double> d_f, d_curve;  // stat, mean
    HIP_TRY(d_u.alloc(4 * T));
    HIP_TRY(d_f.alloc(2 * T));
    if (curve_out) HIP_TRY(d_curve.alloc(T * cw));
    uint32_t* u = d_u.get();
    double* f = d_f.get();

    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    if (N <= ss::WAVE_MAX)
        hipLaunchKernelGGL(mser_kernel<1>, dim3(blocks_for<1>(T)),
                           dim3(Shape<1>::THREADS), 0, 0, in.x.get(), T, N,
                           stride, in.len.get(), in.skip.get(), m, cw, u,
                           u + T, u + 2 * T, u + 3 * T, f, f + T,
                           d_curve.get());
    else
        hipLaunchKernelGGL(mser_kernel<ss::BLOCK_WAVES>,
                           dim3(blocks_for<ss::BLOCK_WAVES>(T)),
                           dim3(Shape<ss::BLOCK_WAVES>::THREADS), 0, 0,
                           in.x.get(), T, N, stride, in.len.get(),
                           in.skip.get(), m, cw, u, u + T, u + 2 * T,
                           u + 3 * T, f, f + T, d_curve.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;

    std::vector<uint32_t> hu(4 * T);
    std::vector<double> hf(2 * T);
    HIP_TRY(d_u.download(hu.data(), 4 * T));
    HIP_TRY(d_f.download(hf.data(), 2 * T));
    for (uint64_t t = 0; t < T; ++t) {
        n_out[t] = hu[t];
        k_out[t] = hu[T + t];
        d_out[t] = hu[2 * T + t];
        cut_out[t] = hu[3 * T + t];
        stat_out[t] = hf[t];
        mean_out[t] = hf[T + t];
    }
    if (curve_out) HIP_TRY(d_curve.download(curve_out, T * cw));
    return 0;
}

// As above; every output is double [T][levels].
int cimba_batch_means_gpu(const double* host_x, uint64_t T, uint64_t N,
                          uint64_t stride, const uint32_t* host_len,
                          const uint32_t* host_skip, uint32_t m,
                          uint32_t levels, int device, double* k_out,
                          double* mean_out, double* sse_out, double* c1_out,
                          double* dsq_out, double* elapsed_ms) {
    if (!ss::args_ok(T, N, stride, m, levels) || !ss::grid_ok(T, N))
        return (int)hipErrorInvalidValue;
    HIP_TRY(hipSetDevice(device));
    DevRows in;
    HIP_TRY(in.upload(host_x, T, N, stride, host_len, host_skip));
    const size_t no = (size_t)T * levels;
    cmb_hip::DevBuf<double> d_o;  // k, mean, sse, c1, dsq
    HIP_TRY(d_o.alloc(5 * no));
    double* p = d_o.get();

    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    if (N <= ss::WAVE_MAX)
        hipLaunchKernelGGL(ladder_kernel<1>, dim3(blocks_for<1>(T)),
                           dim3(Shape<1>::THREADS), 0, 0, in.x.get(), T, N,
                           stride, in.len.get(), in.skip.get(), m, levels, p,
                           p + no, p + 2 * no, p + 3 * no, p + 4 * no);
    else
        hipLaunchKernelGGL(ladder_kernel<ss::BLOCK_WAVES>,
                           dim3(blocks_for<ss::BLOCK_WAVES>(T)),
                           dim3(Shape<ss::BLOCK_WAVES>::THREADS), 0, 0,
                           in.x.get(), T, N, stride, in.len.get(),
                           in.skip.get(), m, levels, p, p + no, p + 2 * no,
                           p + 3 * no, p + 4 * no);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;

    HIP_TRY(d_o.download(k_out, no));
    std::vector<double> h(4 * no);
    HIP_TRY(hipMemcpy(h.data(), p + no, sizeof(double) * 4 * no,
                      hipMemcpyDeviceToHost));
    for (size_t i = 0; i < no; ++i) {
        mean_out[i] = h[i];
        sse_out[i] = h[no + i];
        c1_out[i] = h[2 * no + i];
        dsq_out[i] = h[3 * no + i];
    }
    return 0;
}

}  // extern "C"
