// Time-weighted order statistics (include/cimba/timestat.hpp): every row of
// a state history x[T][stride], t[T][stride] turned into (key, weight)
// pairs, sorted, scanned and searched by cumulative weight in ONE launch;
// the sorted row never goes through HBM between sort and scan.
//
// A pair is the 64-bit key of the value (ostat::key_of) and the bits of the
// sample's duration, a positive double, which order as the durations do.
// Dropped samples and padding are (KEY_PAD, W_PAD): they sort after every
// kept pair and the scan reads them as weight 0.  Rows are padded to n_pad,
// a power of two that fits the longest possible row of the call, and all
// rows of a call take the same tier.  No atomics, every exchange and every
// addition at a fixed place: a result is the same from run to run.
//
//   tstat_wave_kernel<K>   n_pad = 64 K <= 512: one wave per row, four rows
//       per block, K pairs per lane (element e = lane * K + j).  A lane
//       loads t_e for its K elements and takes t of the next lane's first
//       element by ds_bpermute, so every weight is built in registers.  The
//       bitonic network is ostat_wave_kernel's on pairs: both 64-bit halves
//       travel to lane ^ m by DPP quad_perm (m = 1, 2), ds_swizzle (4, 8,
//       16) or ds_bpermute (32).  Then a lane sums its K sorted weights
//       serially; an inclusive scan of the lane sums (DPP row_shr 1, 2, 4, 8
//       inside each row of 16 lanes, the three row totals by readlane) and
//       one shift by a lane give every cum_k in registers.  For each q the
//       lanes test their positions against q * total, a ballot finds the
//       first lane that holds a hit and that lane stores the value.  No
//       LDS, no barrier.
//   tstat_block_kernel<NPAD>  n_pad = 1024 .. 8192: one workgroup of
//       NPAD / 8 threads per row.  Register-blocked passes of three levels
//       per LDS round trip as in ostat_block_kernel; the last pass leaves 8
//       adjacent sorted pairs in registers and the scan goes on from there:
//       serial over the 8, the wave scan above, wave totals through 16 LDS
//       words.  Quantiles: every wave ballots for its first hit and leaves
//       (flag, value) in LDS, thread i picks the first wave for q_i.
//       LDS layout: keys[NPAD] and weights[NPAD] are two arrays, each
//       indexed by ostat's XOR fold i ^ f(i >> 5).  That fold was derived
//       for 8-byte slots read by ds_read_b64; a 16-byte pair slot would be
//       read by ds_read_b128, which the LDS serves in other lane groups, so
//       the fold's proof does not carry over.  Two folded 8-byte arrays keep
//       it as proven: every pass is two conflict-free b64 accesses.
//       8192 pairs are 128 KB: dynamic LDS with the function attribute
//       raised above the 64 KB static limit, one workgroup per CU.
//   tstat_hist_kernel      one thread per (row, bin): tstat::hist_time, two
//       binary searches in the sorted values and a difference of cum.
//
// Sorted values and cumulative weights go to vals[T][N] and cum[T][N] (NaN
// at and past n_r): the caller's outputs when it wants them, else a
// workspace, and only when the histogram needs them or they are wanted.
//
// Compiler's resource report (gfx950, -O3; profiles/r14_timestat.md):
//   tstat_wave_kernel<1/2/4/8>      21 / 32 / 52 / 87 VGPRs, no LDS;
//                                   8 waves per SIMD, 5 at K = 8
//   tstat_block_kernel<1024..4096>  76 VGPRs, 6 waves per SIMD by registers;
//                                   dynamic LDS 16 / 32 / 64 KB
//   tstat_block_kernel<8192>        92 VGPRs, dynamic LDS 128 KB: one
//                                   workgroup of 16 waves per CU, 4 per SIMD
//   tstat_hist_kernel               32 VGPRs, no LDS, 8 waves per SIMD
// No kernel uses scratch.
#include <hip/hip_runtime.h>

#include "../include/cimba/timestat.hpp"
#include "hip_host.hpp"

namespace {

namespace ostat = cmb::ostat;
namespace tstat = cmb::tstat;
namespace corr = cmb::corr;

constexpr uint32_t WAVE = 64;
constexpr uint32_t WAVE_WG = 256;  // four rows per block
constexpr uint32_t FLAT_WG = 256;

struct QList {
    double q[ostat::MAX_Q];
};

// what every sorting kernel reads and writes
struct Rows {
    const double* x;
    const double* t;
    uint64_t T, N, stride;
    const uint32_t* len;
    const double* start;
    const double* end;
    uint32_t nq;
    double* n_out;
    double* total_out;
    double* quant_out;
    double* vals;  // [T][N], with cum, or both null
    double* cum;
};

// ---- lane exchanges ---------------------------------------------------------

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

// v of lane src (any lane, 0 .. 63)
__device__ __forceinline__ uint64_t lane_get64(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(
        (int)(src << 2), (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(
        (int)(src << 2), (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// v of lane - D inside a row of 16 lanes, +0.0 where that lane is outside
template <int D>
__device__ __forceinline__ double row_shr(double v) {
    const uint64_t u = cmb::double_as_u64(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(
        0, (int)(uint32_t)u, 0x110 + D, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(
        0, (int)(uint32_t)(u >> 32), 0x110 + D, 0xF, 0xF, true);
    return cmb::u64_as_double(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double read_lane(double v, int src) {
    const uint64_t u = cmb::double_as_u64(v);
    const uint32_t lo =
        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
    const uint32_t hi =
        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
    return cmb::u64_as_double(((uint64_t)hi << 32) | lo);
}

// Inclusive scan of s over the 64 lanes of a full wave: Hillis-Steele inside
// each row of 16, then the totals of the rows below added in a fixed order.
__device__ __forceinline__ double wave_scan(double s, uint32_t lane) {
    s += row_shr<1>(s);
    s += row_shr<2>(s);
    s += row_shr<4>(s);
    s += row_shr<8>(s);
    const double t0 = read_lane(s, 15), t1 = read_lane(s, 31),
                 t2 = read_lane(s, 47);
    const uint32_t row = lane >> 4;
    const double below =
        row == 0 ? 0.0 : row == 1 ? t0 : row == 2 ? t0 + t1 : (t0 + t1) + t2;
    return s + below;
}

// the scan's value of the lane below, 0.0 for lane 0
__device__ __forceinline__ double lane_below(double inc, uint32_t lane) {
    const double v = cmb::u64_as_double(
        lane_get64(cmb::double_as_u64(inc), (lane + WAVE - 1) & (WAVE - 1)));
    return lane ? v : 0.0;
}

__device__ __forceinline__ double weight_of(uint64_t wbits) {
    return wbits == tstat::W_PAD ? 0.0 : cmb::u64_as_double(wbits);
}

__device__ __forceinline__ void cmpx(uint64_t& ka, uint64_t& wa, uint64_t& kb,
                                     uint64_t& wb, bool asc) {
    // equal pairs may swap: they are indistinguishable
    const bool swap = tstat::pair_less(kb, wb, ka, wa) == asc;
    const uint64_t k0 = swap ? kb : ka, w0 = swap ? wb : wa;
    const uint64_t k1 = swap ? ka : kb, w1 = swap ? wa : wb;
    ka = k0;
    wa = w0;
    kb = k1;
    wb = w1;
}

// pair of element e of a row of m samples; tt is t_e, nx the time at which
// the sample ends (the row's end for the last one)
__device__ __forceinline__ void make_pair(const double* __restrict__ xr,
                                          uint64_t e, uint64_t m, double tt,
                                          double nx, double start, double end,
                                          uint64_t& k, uint64_t& w) {
    k = ostat::KEY_PAD;
    w = tstat::W_PAD;
    if (e < m) {
        const double d = tstat::sample_weight(tt, nx, start, end);
        if (d > 0.0) {
            k = ostat::key_of(xr[e]);
            w = cmb::double_as_u64(d);
        }
    }
}

// ---- wave tier -------------------------------------------------------------

// Level of stride S of merge size KK on the wave's pairs, then the levels
// below it.  Templates, not loops: every stride is a constant, so each
// lane exchange compiles to its one instruction.
template <int K, uint32_t KK, uint32_t S>
__device__ __forceinline__ void wave_levels(uint64_t (&k)[K], uint64_t (&w)[K],
                                            uint32_t lane) {
    if constexpr (S >= K) {
        constexpr uint32_t mm = S / K;
        // the lower lane of a pair of lanes keeps the smaller pair when the
        // two sort ascending
        const bool keep_min = ((lane & mm) == 0) == (((lane * K) & KK) == 0);
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) {
            const uint64_t ok = lane_xor64(k[j], mm, lane);
            const uint64_t ow = lane_xor64(w[j], mm, lane);
            const bool take = keep_min
                                  ? tstat::pair_less(ok, ow, k[j], w[j])
                                  : tstat::pair_less(k[j], w[j], ok, ow);
            k[j] = take ? ok : k[j];
            w[j] = take ? ow : w[j];
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < K; ++j)
            if (!(j & S))
                cmpx(k[j], w[j], k[j | S], w[j | S],
                     ((lane * K + j) & KK) == 0);
    }
    if constexpr (S > 1) wave_levels<K, KK, S / 2>(k, w, lane);
}

// merge sizes KK, 2 KK, .. 64 K
template <int K, uint32_t KK>
__device__ __forceinline__ void wave_merges(uint64_t (&k)[K], uint64_t (&w)[K],
                                            uint32_t lane) {
    wave_levels<K, KK, KK / 2>(k, w, lane);
    if constexpr (KK < WAVE * K) wave_merges<K, 2 * KK>(k, w, lane);
}

template <int K>
__global__ __launch_bounds__(WAVE_WG) void tstat_wave_kernel(Rows a,
                                                             QList ql) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t r = (uint64_t)blockIdx.x * (WAVE_WG / WAVE) +
                       threadIdx.x / WAVE;
    if (r >= a.T) return;  // wave-uniform: the shuffles see all 64 lanes
    const uint64_t m = corr::effective_n(a.N, a.len, r, 0);
    const double* xr = a.x + r * a.stride;
    const double* tr = a.t + r * a.stride;
    const double start = a.start[r], end = a.end[r];

    // times past the row read as its end, so the last sample ends there
    double tt[K];
#pragma unroll
    for (uint32_t j = 0; j < K; ++j) {
        const uint32_t e = lane * K + j;
        tt[j] = e < m ? tr[e] : end;
    }
    double nxt = cmb::u64_as_double(
        lane_get64(cmb::double_as_u64(tt[0]), (lane + 1) & (WAVE - 1)));
    if (lane == WAVE - 1) nxt = end;
    uint64_t k[K], w[K];
#pragma unroll
    for (uint32_t j = 0; j < K; ++j)
        make_pair(xr, lane * K + j, m, tt[j], j + 1 < K ? tt[j + 1] : nxt,
                  start, end, k[j], w[j]);

    wave_merges<K, 2>(k, w, lane);

    // kept pairs come first: count them, then scan the weights
    uint32_t n = 0;
    double c[K], acc = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < K; ++j) {
        n += (uint32_t)__builtin_popcountll(
            __builtin_amdgcn_ballot_w64(w[j] != tstat::W_PAD));
        acc += weight_of(w[j]);
        c[j] = acc;
    }
    const double below = lane_below(wave_scan(acc, lane), lane);
    double last = 0.0;  // cum of position n - 1, in the lane that holds it
#pragma unroll
    for (uint32_t j = 0; j < K; ++j) {
        c[j] = below + c[j];
        if (lane * K + j + 1 == n) last = c[j];
    }
    const double total =
        n ? cmb::u64_as_double(
                lane_get64(cmb::double_as_u64(last), (n - 1) / K))
          : 0.0;
    if (lane == 0) {
        a.n_out[r] = (double)n;
        a.total_out[r] = total;
    }

    for (uint32_t i = 0; i < a.nq; ++i) {
        const double target = ql.q[i] * total;
        bool hit = false;
        uint64_t v = ostat::KEY_PAD;
#pragma unroll
        for (int j = K - 1; j >= 0; --j)
            if (lane * K + j < n && c[j] >= target) {
                hit = true;
                v = k[j];
            }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(hit);
        // no hit (an empty row): the all-ones key of lane 0 gives NaN
        const uint32_t first = mask ? (uint32_t)__builtin_ctzll(mask) : 0;
        if (lane == first) a.quant_out[r * a.nq + i] = ostat::key_to_double(v);
    }

    if (a.vals) {
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) {
            const uint32_t col = lane * K + j;
            if (col < a.N) {
                a.vals[r * a.N + col] = ostat::key_to_double(k[j]);
                a.cum[r * a.N + col] = col < n ? c[j] : tstat::quiet_nan();
            }
        }
    }
}

// ---- block tier ------------------------------------------------------------

// LDS slot of element i in either array (ostat_block_kernel's fold).  With
// h = i >> 5, bits 0..2 of h are folded into the low five bits as h0 -> bit
// 2, h1 -> bits 3 and 0, h2 -> bits 4 and 1, so that for every pass stride
// 1 .. 16 the 32 lanes of a half wave hit 32 different 8-byte slots.
__device__ __forceinline__ uint32_t slot(uint32_t i) {
    const uint32_t h = i >> 5;
    return i ^ (((h & 1u) << 2) | (((h >> 1) & 3u) * 9u));
}

// the top NL of the three levels (strides 4s, 2s, s) on a thread's 8 pairs
template <int NL>
__device__ __forceinline__ void levels8(uint64_t (&k)[8], uint64_t (&w)[8],
                                        bool asc) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int bit = 4 >> l;
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (!(m & bit)) cmpx(k[m], w[m], k[m | bit], w[m | bit], asc);
    }
}

// One register-blocked pass at low stride 2^ls0 of merge size kk (at least
// 8 strides, so one direction serves the 8 pairs).
template <int NL, bool WRITE>
__device__ __forceinline__ void lds_pass(uint64_t* keys, uint64_t* wts,
                                         uint32_t tid, uint32_t ls0,
                                         uint32_t kk, uint64_t (&k)[8],
                                         uint64_t (&w)[8]) {
    const uint32_t s0 = 1u << ls0;
    const uint32_t base = ((tid >> ls0) << (ls0 + 3)) | (tid & (s0 - 1));
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) {
        const uint32_t s = slot(base + m * s0);
        k[m] = keys[s];
        w[m] = wts[s];
    }
    levels8<NL>(k, w, (base & kk) == 0);
    if (WRITE) {
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m) {
            const uint32_t s = slot(base + m * s0);
            keys[s] = k[m];
            wts[s] = w[m];
        }
    }
}

// Strides 2^ltop .. 1 of merge size kk on pairs in LDS (ltop >= 3).  The
// last pass leaves pairs 8 tid .. 8 tid + 7 in registers; they go back to
// LDS only when another merge follows.  Every thread of the block calls it.
__device__ __forceinline__ void lds_merge(uint64_t* keys, uint64_t* wts,
                                          uint32_t tid, uint32_t ltop,
                                          uint32_t kk, uint64_t (&k)[8],
                                          uint64_t (&w)[8], bool writeback) {
    uint32_t l = ltop;
    const uint32_t rem = (ltop + 1) % 3;
    if (rem == 1) {
        lds_pass<1, true>(keys, wts, tid, l - 2, kk, k, w);
        l -= 1;
        __syncthreads();
    } else if (rem == 2) {
        lds_pass<2, true>(keys, wts, tid, l - 2, kk, k, w);
        l -= 2;
        __syncthreads();
    }
    while (l > 2) {
        lds_pass<3, true>(keys, wts, tid, l - 2, kk, k, w);
        l -= 3;
        __syncthreads();
    }
    lds_pass<3, false>(keys, wts, tid, 0, kk, k, w);
    if (writeback) {
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m) {
            const uint32_t s = slot(8 * tid + m);
            keys[s] = k[m];
            wts[s] = w[m];
        }
        __syncthreads();
    }
}

template <uint32_t NPAD>
__global__ __launch_bounds__(NPAD / 8) void tstat_block_kernel(Rows a,
                                                               QList ql) {
    static_assert(NPAD >= 1024 && NPAD <= tstat::BLOCK_MAX,
                  "128 to 1024 threads");
    constexpr uint32_t NW = NPAD / 8 / WAVE;  // waves of the block
    // words of the LDS reused after the sort
    constexpr uint32_t L_WTOT = 0, L_WCNT = 16, L_TOTAL = 32, L_FLAG = 64,
                       L_HIT = L_FLAG + ostat::MAX_Q * NW;
    static_assert(L_HIT + ostat::MAX_Q * NW <= 2 * NPAD, "fits the pairs");
    extern __shared__ uint64_t lds[];
    uint64_t* keys = lds;
    uint64_t* wts = lds + NPAD;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1), wv = tid / WAVE;
    const uint64_t r = blockIdx.x;
    const uint64_t m = corr::effective_n(a.N, a.len, r, 0);
    const double* xr = a.x + r * a.stride;
    const double* tr = a.t + r * a.stride;
    const double start = a.start[r], end = a.end[r];

    // 8 adjacent pairs; times past the row read as its end
    const uint32_t g0 = 8 * tid;
    double tt[9];
#pragma unroll
    for (uint32_t j = 0; j < 9; ++j) tt[j] = g0 + j < m ? tr[g0 + j] : end;
    uint64_t k[8], w[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j)
        make_pair(xr, g0 + j, m, tt[j], tt[j + 1], start, end, k[j], w[j]);

    // merge sizes 2, 4, 8 in registers, then 16 .. NPAD through LDS
#pragma unroll
    for (uint32_t kk = 2; kk <= 8; kk <<= 1) {
#pragma unroll
        for (uint32_t s = kk >> 1; s >= 1; s >>= 1) {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                if (!(j & s))
                    cmpx(k[j], w[j], k[j | s], w[j | s],
                         ((g0 + j) & kk) == 0);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t s = slot(g0 + j);
        keys[s] = k[j];
        wts[s] = w[j];
    }
    __syncthreads();
    for (uint32_t lk = 4; (1u << lk) <= NPAD; ++lk)
        lds_merge(keys, wts, tid, lk - 1, 1u << lk, k, w, (2u << lk) <= NPAD);
    __syncthreads();  // the last pass is read: the LDS is free

    // serial over the 8, scan over the wave, wave totals through LDS
    uint32_t wcount = 0;
    double c[8], acc = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        wcount += (uint32_t)__builtin_popcountll(
            __builtin_amdgcn_ballot_w64(w[j] != tstat::W_PAD));
        acc += weight_of(w[j]);
        c[j] = acc;
    }
    const double inc = wave_scan(acc, lane);
    double below = lane_below(inc, lane);
    if (lane == WAVE - 1) lds[L_WTOT + wv] = cmb::double_as_u64(inc);
    if (lane == 0) lds[L_WCNT + wv] = wcount;
    __syncthreads();
    uint32_t n = 0;
    double wbelow = 0.0;
    for (uint32_t v = 0; v < NW; ++v) {
        n += (uint32_t)lds[L_WCNT + v];
        if (v < wv) wbelow += cmb::u64_as_double(lds[L_WTOT + v]);
    }
    below = wbelow + below;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        c[j] = below + c[j];
        if (g0 + j + 1 == n) lds[L_TOTAL] = cmb::double_as_u64(c[j]);
    }
    if (n == 0 && tid == 0) lds[L_TOTAL] = 0;  // +0.0
    if (a.vals) {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t col = g0 + j;
            if (col < a.N) {
                a.vals[r * a.N + col] = ostat::key_to_double(k[j]);
                a.cum[r * a.N + col] = col < n ? c[j] : tstat::quiet_nan();
            }
        }
    }
    __syncthreads();
    const double total = cmb::u64_as_double(lds[L_TOTAL]);
    if (tid == 0) {
        a.n_out[r] = (double)n;
        a.total_out[r] = total;
    }

    // every wave leaves its first hit for q_i, thread i takes the first wave
    for (uint32_t i = 0; i < a.nq; ++i) {
        const double target = ql.q[i] * total;
        bool hit = false;
        uint64_t v = ostat::KEY_PAD;
#pragma unroll
        for (int j = 7; j >= 0; --j)
            if (g0 + j < n && c[j] >= target) {
                hit = true;
                v = k[j];
            }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(hit);
        const uint32_t first = mask ? (uint32_t)__builtin_ctzll(mask) : 0;
        if (lane == first) {
            lds[L_FLAG + i * NW + wv] = mask != 0;
            lds[L_HIT + i * NW + wv] = v;
        }
    }
    __syncthreads();
    if (tid < a.nq) {
        uint64_t v = ostat::KEY_PAD;  // no hit (an empty row): NaN
        for (uint32_t u = NW; u-- > 0;)
            if (lds[L_FLAG + tid * NW + u]) v = lds[L_HIT + tid * NW + u];
        a.quant_out[r * a.nq + tid] = ostat::key_to_double(v);
    }
}

// ---- histogram epilogue ----------------------------------------------------

__global__ __launch_bounds__(FLAT_WG) void tstat_hist_kernel(
    const double* __restrict__ vals, const double* __restrict__ cum,
    const double* __restrict__ n_out, uint64_t T, uint64_t N, uint32_t nbins,
    double* __restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * FLAT_WG + threadIdx.x;
    if (idx >= T * nbins) return;
    const uint64_t r = idx / nbins;
    const uint32_t b = (uint32_t)(idx - r * nbins);
    out[idx] = tstat::hist_time(vals + r * N, cum + r * N, (uint64_t)n_out[r],
                                nbins, b);
}

template <int K>
void launch_wave(const Rows& a, const QList& ql) {
    const uint64_t blocks = (a.T + WAVE_WG / WAVE - 1) / (WAVE_WG / WAVE);
    hipLaunchKernelGGL(tstat_wave_kernel<K>, dim3((uint32_t)blocks),
                       dim3(WAVE_WG), 0, 0, a, ql);
}

// 16 bytes of dynamic LDS per pair; above 64 KB the limit is raised first
template <uint32_t NPAD>
int launch_block(const Rows& a, const QList& ql) {
    constexpr size_t bytes = (size_t)NPAD * 16;
    if (bytes > 65536)
        HIP_TRY(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&tstat_block_kernel<NPAD>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(tstat_block_kernel<NPAD>, dim3((uint32_t)a.T),
                       dim3(NPAD / 8), bytes, 0, a, ql);
    return 0;
}

}  // namespace

extern "C" {

// Device pointers: x[T][stride] and t[T][stride] (the last row may end after
// N values), len[T] or null, start[T], end[T], n_out[T], total_out[T];
// quant_out[T][nq], hist_out[T][nbins], vals_out[T][N] and cum_out[T][N]
// (both or neither) may be null and are then neither computed nor stored.
// q[nq] is a HOST array (it is checked here and travels as a kernel
// argument).  elapsed_ms (nullable) is the kernels alone.  Returns 0, -1 on
// bad arguments, or the HIP error.
int cimba_time_stats_gpu_dev(const double* x, const double* t, uint64_t T,
                             uint64_t N, uint64_t stride, const uint32_t* len,
                             const double* start, const double* end,
                             const double* q, uint32_t nq, uint32_t nbins,
                             double* n_out, double* total_out,
                             double* quant_out, double* hist_out,
                             double* vals_out, double* cum_out,
                             double* elapsed_ms) {
    if (!tstat::args_ok(T, N, stride, q, nq, nbins) || !tstat::grid_ok(T, N) ||
        !vals_out != !cum_out)
        return -1;
    const uint64_t n_pad = ostat::pad_len(N, 0);
    const bool want_q = quant_out && nq, want_h = hist_out && nbins;
    // the histogram reads the sorted rows: from the outputs when the caller
    // wants those, else from a workspace of the same shape
    cmb_hip::DevBuf<double> d_ws;
    if (want_h && !vals_out && N) {
        HIP_TRY(d_ws.alloc((size_t)(2 * T * N)));
        vals_out = d_ws.get();
        cum_out = d_ws.get() + T * N;
    }
    QList ql = {};
    for (uint32_t i = 0; i < nq; ++i) ql.q[i] = q[i];
    const Rows a = {x,     t,         T,         N,
                    stride, len,      start,     end,
                    want_q ? nq : 0,  n_out,     total_out,
                    quant_out,        vals_out,  cum_out};

    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    switch (n_pad) {
        case 64: launch_wave<1>(a, ql); break;
        case 128: launch_wave<2>(a, ql); break;
        case 256: launch_wave<4>(a, ql); break;
        case 512: launch_wave<8>(a, ql); break;
        case 1024: HIP_TRY(launch_block<1024>(a, ql)); break;
        case 2048: HIP_TRY(launch_block<2048>(a, ql)); break;
        case 4096: HIP_TRY(launch_block<4096>(a, ql)); break;
        default: HIP_TRY(launch_block<8192>(a, ql)); break;
    }
    HIP_TRY(hipGetLastError());
    if (want_h) {
        const uint64_t blocks = (T * nbins + FLAT_WG - 1) / FLAT_WG;
        hipLaunchKernelGGL(tstat_hist_kernel, dim3((uint32_t)blocks),
                           dim3(FLAT_WG), 0, 0, vals_out, cum_out, n_out, T, N,
                           nbins, hist_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;
    return 0;
}

// Host arrays in and out: host_x and host_t [T][stride] (T - 1 full rows
// and N values of the last), host_len[T] or null, host_start[T],
// host_end[T]; n_out[T], total_out[T] and the outputs of
// cimba_time_stats_gpu_dev, of which only those asked for are allocated on
// the device and downloaded.
int cimba_time_stats_gpu(const double* host_x, const double* host_t,
                         uint64_t T, uint64_t N, uint64_t stride,
                         const uint32_t* host_len, const double* host_start,
                         const double* host_end, const double* q, uint32_t nq,
                         uint32_t nbins, int device, double* n_out,
                         double* total_out, double* quant_out,
                         double* hist_out, double* vals_out, double* cum_out,
                         double* elapsed_ms) {
    if (!tstat::args_ok(T, N, stride, q, nq, nbins) || !tstat::grid_ok(T, N) ||
        !vals_out != !cum_out)
        return -1;
    HIP_TRY(hipSetDevice(device));
    const size_t nx = (size_t)((T - 1) * stride + N);
    const bool want_s = vals_out && N, want_q = quant_out && nq,
               want_h = hist_out && nbins;
    cmb_hip::DevBuf<double> d_x, d_t, d_start, d_end, d_n, d_total, d_quant,
        d_hist, d_vals, d_cum;
    cmb_hip::DevBuf<uint32_t> d_len;
    HIP_TRY(d_x.alloc(nx ? nx : 1));
    HIP_TRY(d_t.alloc(nx ? nx : 1));
    HIP_TRY(d_start.alloc(T));
    HIP_TRY(d_end.alloc(T));
    HIP_TRY(d_n.alloc(T));
    HIP_TRY(d_total.alloc(T));
    if (nx) {
        HIP_TRY(d_x.upload(host_x, nx));
        HIP_TRY(d_t.upload(host_t, nx));
    }
    HIP_TRY(d_start.upload(host_start, T));
    HIP_TRY(d_end.upload(host_end, T));
    if (host_len) {
        HIP_TRY(d_len.alloc(T));
        HIP_TRY(d_len.upload(host_len, T));
    }
    if (want_s) {
        HIP_TRY(d_vals.alloc((size_t)(T * N)));
        HIP_TRY(d_cum.alloc((size_t)(T * N)));
    }
    if (want_q) HIP_TRY(d_quant.alloc((size_t)T * nq));
    if (want_h) HIP_TRY(d_hist.alloc((size_t)T * nbins));
    HIP_TRY(cimba_time_stats_gpu_dev(
        d_x.get(), d_t.get(), T, N, stride, d_len.get(), d_start.get(),
        d_end.get(), q, nq, nbins, d_n.get(), d_total.get(), d_quant.get(),
        d_hist.get(), d_vals.get(), d_cum.get(), elapsed_ms));
    HIP_TRY(d_n.download(n_out, T));
    HIP_TRY(d_total.download(total_out, T));
    if (want_s) {
        HIP_TRY(d_vals.download(vals_out, (size_t)(T * N)));
        HIP_TRY(d_cum.download(cum_out, (size_t)(T * N)));
    }
    if (want_q) HIP_TRY(d_quant.download(quant_out, (size_t)T * nq));
    if (want_h) HIP_TRY(d_hist.download(hist_out, (size_t)T * nbins));
    return 0;
}

}  // extern "C"
