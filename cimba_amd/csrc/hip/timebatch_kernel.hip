// Regular-grid time averages (include/cimba/timebatch.hpp): every row of a
// state history x[T][stride], t[T][stride] averaged over K equal intervals
// of its window in ONE launch, by a merge-path segmented reduction.
//
// The pieces of a row are the steps of the merge of its sample keys with the
// interior grid edges (timebatch.hpp).  The steps, not the samples and not
// the batches, are dealt out: every lane takes LANE_STEPS = 8 consecutive
// steps, so a lane is as busy where thousands of samples share a batch as
// where one sample spans hundreds of batches.  Edges are one multiply and
// one add of tbatch::edge, never stored or loaded.
//
//   tbatch_kernel<64>    N + K <= TBATCH_WAVE_MAX = 512: one wave per row,
//       four rows per workgroup, the whole merge (at most 511 steps) in one
//       chunk.
//   tbatch_kernel<256>   one workgroup per row, chunks of TBATCH_CHUNK =
//       2048 steps walked left to right, so a row has no longest length.
//
// A chunk that starts after i0 samples and j0 edges:
//   stage      the next S <= chunk samples, with the one before them and the
//              time after them, go coalesced into LDS: t (raw, so that nx_i
//              is the staged neighbour) and x.
//   keys       a running maximum of the finite staged times (8 serial per
//              thread, __shfl_up over the wave, wave totals through LDS,
//              the chunk before through a register), clamped to the window.
//              Sorted by construction: a NaN time, or a row outside the
//              contract, cannot mislead the searches below.
//   partition  a lane finds where step 8 * lane of the chunk starts by a
//              binary search along its diagonal, staged keys against
//              computed edges; both indices are clamped to the chunk.
//   walk       8 steps in registers.  A step takes the next edge if it is
//              not above the next key, else the next sample, then adds the
//              overlap of the current (sample, batch).  Taking an edge
//              closes a batch: the lane's first closed batch is kept (its
//              head), later ones lie wholly inside the lane and are stored
//              at once.  What is open after the last step is its tail.
//   combine    a segmented inclusive scan of (closed any, tail) over the
//              wave with __shfl_up, wave totals and the open batch of the
//              chunk before folded in through LDS.  Its exclusive value is
//              what the lanes below left open: a lane that closed a batch
//              stores head plus that.  One lane writes each batch once; no
//              atomics, and a fixed order of additions.
//   carry      the scan's total is the batch still open; it and the key of
//              the last sample taken stay in registers for the next chunk.
//              The end of the chunk's path is searched like a lane's start.
//
// How the numbers were chosen.  8 steps per lane amortise one binary search
// (at most 11 probes of LDS) over 8 pieces while the walk's state (two
// sums, head, two edges, three staged values, the next key) stays below
// the 128 VGPRs that 4 waves per SIMD allow (the compiler reports 110, no
// scratch).  The chunk is 8 steps for each of 256 threads; three staged
// arrays of 2048 doubles, padded by one slot in nine so that lanes 8
// samples apart fall into different banks, are 54 KB: two workgroups, 8
// waves, per CU, which is what limits the kernel today.  The wave tier ends
// where one wave's 8 steps per lane end.  None of the three numbers has
// been tuned by measurement yet.  Resource report and measurements:
// profiles/r18_time_batches.md.
#include <hip/hip_runtime.h>

#include "../include/cimba/timebatch.hpp"
#include "hip_host.hpp"

namespace {

namespace tstat = cmb::tstat;
namespace tbatch = cmb::tbatch;
namespace corr = cmb::corr;

constexpr uint32_t WAVE = 64;
constexpr uint32_t WG = 256;
constexpr uint32_t R = tbatch::LANE_STEPS;

struct Args {
    const double* x;
    const double* t;
    uint64_t T, N, stride;
    const uint32_t* len;
    const double* start;
    const double* end;
    uint32_t K;
    double* n_out;
    double* width_out;
    double* integral;
    double* covered;
    double* mean;
};

// LDS slot of staged element i: one slot in nine is left empty
__device__ __forceinline__ uint32_t slot(uint32_t i) { return i + (i >> 3); }

// Samples taken before step d of a chunk with S staged keys and E edges
// left after j0: the smallest i with key[i] >= edge j0 + d - i.
__device__ __forceinline__ uint32_t partition(const double* key, uint32_t S,
                                              uint32_t E, uint32_t j0,
                                              uint32_t d, double start,
                                              double w) {
    uint32_t lo = d > E ? d - E : 0, hi = d < S ? d : S;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        // lo <= mid < hi: 1 <= d - mid <= E, an interior edge, and mid < S
        if (key[slot(mid)] < start + (double)(j0 + (d - mid)) * w)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

template <uint32_t G>
__global__ __launch_bounds__(WG) void tbatch_kernel(Args a) {
    constexpr uint32_t CH = G * R;       // steps of a chunk
    constexpr uint32_t ROWS = WG / G;    // rows of a workgroup
    constexpr uint32_t NW = G / WAVE;    // waves of a row
    constexpr uint32_t SLOTS = CH + CH / 8 + 3;
    static_assert(G == WAVE || G == WG, "a wave or the workgroup per row");
    __shared__ double s_t[ROWS][SLOTS];  // [q]: time of sample i0 + q - 1
    __shared__ double s_x[ROWS][SLOTS];  // [q]: its value
    __shared__ double s_key[ROWS][SLOTS];  // [i]: key of sample i0 + i
    __shared__ double s_wv[NW][3];       // wave totals: max, or (i, c)
    __shared__ uint32_t s_wf[NW];        // wave totals: closed any, or n

    const uint32_t tid = threadIdx.x;
    const uint32_t g = tid % G, lane = tid & (WAVE - 1), wv = g / WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * ROWS + tid / G;
    double* ts = s_t[tid / G];
    double* xs = s_x[tid / G];
    double* key = s_key[tid / G];

    const uint32_t K = a.K;
    const bool live = r < a.T;
    const double start = live ? a.start[r] : 0.0, end = live ? a.end[r] : 0.0;
    const bool run = live && tbatch::row_on(start, end);
    const double w = tbatch::width(start, end, K);
    const double* xr = a.x + (live ? r : 0) * a.stride;
    const double* tr = a.t + (live ? r : 0) * a.stride;
    double* ig = a.integral + (live ? r : 0) * K;
    double* cv = a.covered + (live ? r : 0) * K;
    double* mn = a.mean + (live ? r : 0) * K;
    if (live && !run)
        for (uint32_t j = g; j < K; j += G) {
            ig[j] = 0.0;
            cv[j] = 0.0;
            mn[j] = tstat::quiet_nan();
        }
    // a row that does not run has no samples and no edges: no step, no store
    const uint64_t m = run ? corr::effective_n(a.N, a.len, r, 0) : 0;
    const uint32_t edges = run ? K - 1 : 0;

    uint64_t i0 = 0;        // samples taken before the chunk
    uint32_t j0 = 0;        // edges taken before the chunk
    double kprev = start;   // key of sample i0 - 1
    double ci = 0.0, cc = 0.0;  // the batch open at the start of the chunk
    uint32_t cnt = 0;       // samples this thread took that have weight
    uint64_t left;
    uint32_t dcount;
    do {
        const uint32_t E = edges - j0;
        const uint32_t S = m - i0 < CH ? (uint32_t)(m - i0) : CH;
        left = (m - i0) + E;
        dcount = left < CH ? (uint32_t)left : CH;

        // ---- stage --------------------------------------------------------
        for (uint32_t q = g; q < S + 2; q += G) {
            const uint64_t gi = i0 + q;  // sample gi - 1
            const bool has = gi >= 1 && gi - 1 < m;
            // no sample before the first; the row's end after the last
            ts[slot(q)] = has ? tr[gi - 1] : gi ? end : tstat::quiet_nan();
            xs[slot(q)] = has ? xr[gi - 1] : 0.0;
        }
        __syncthreads();

        // ---- keys ---------------------------------------------------------
        {
            double pm[R], mx = -__builtin_inf();
#pragma unroll
            for (uint32_t k = 0; k < R; ++k) {
                const uint32_t i = g * R + k;
                const double v = i < S ? ts[slot(i + 1)] : mx;
                mx = v > mx ? v : mx;  // a NaN keeps mx
                pm[k] = mx;
            }
            double inc = mx;
#pragma unroll
            for (uint32_t off = 1; off < WAVE; off <<= 1) {
                const double p = __shfl_up(inc, off, WAVE);
                if (lane >= off) inc = p > inc ? p : inc;
            }
            double below = __shfl_up(inc, 1, WAVE);
            if (lane == 0) below = kprev;
            if (NW > 1) {
                if (lane == WAVE - 1) s_wv[wv][0] = inc;
                __syncthreads();
                for (uint32_t v = 0; v < wv; ++v)
                    below = s_wv[v][0] > below ? s_wv[v][0] : below;
            }
            below = kprev > below ? kprev : below;
#pragma unroll
            for (uint32_t k = 0; k < R; ++k) {
                const uint32_t i = g * R + k;
                if (i < S) key[slot(i)] = tbatch::next_key(below, pm[k], end);
            }
        }
        __syncthreads();

        // ---- partition and walk ------------------------------------------
        bool closed = false;
        uint32_t first = 0;
        double hi_ = 0.0, hc_ = 0.0;  // head
        double ai = 0.0, ac = 0.0;    // the open batch: at the end, the tail
        const uint32_t d = g * R;
        if (d < dcount) {
            uint32_t ii = partition(key, S, E, j0, d, start, w);
            uint32_t jj = d - ii;
            uint32_t jb = j0 + jj;
            first = jb;
            double lo = tbatch::edge(start, w, end, jb, K);
            double hi = tbatch::edge(start, w, end, jb + 1, K);
            double ct = ts[slot(ii)], cn = ts[slot(ii + 1)];
            double cx = xs[slot(ii)];
            double kn = ii < S ? key[slot(ii)] : end;
#pragma unroll
            for (uint32_t k = 0; k < R; ++k) {
                if (d + k >= dcount) break;
                // ii + jj = d + k < S + E: an edge or a sample is left
                if (jj < E && (ii >= S || hi <= kn)) {
                    if (closed) {
                        ig[jb] = ai;
                        cv[jb] = ac;
                        mn[jb] = tbatch::mean_of(ai, ac);
                    } else {
                        hi_ = ai;
                        hc_ = ac;
                        closed = true;
                    }
                    ai = ac = 0.0;
                    ++jj;
                    ++jb;
                    lo = hi;
                    hi = tbatch::edge(start, w, end, jb + 1, K);
                } else {  // ii < S
                    ++ii;
                    ct = cn;
                    cn = ts[slot(ii + 1)];
                    cx = xs[slot(ii)];
                    kn = ii < S ? key[slot(ii)] : end;
                    cnt += tstat::sample_weight(ct, cn, start, end) > 0.0;
                }
                const double ov = tstat::sample_weight(ct, cn, lo, hi);
                if (ov > 0.0) {
                    ai += cx * ov;
                    ac += ov;
                }
            }
        }

        // ---- combine ------------------------------------------------------
        uint32_t f = closed;
        double vi = ai, vc = ac;
#pragma unroll
        for (uint32_t off = 1; off < WAVE; off <<= 1) {
            const uint32_t pf = __shfl_up(f, off, WAVE);
            const double pvi = __shfl_up(vi, off, WAVE);
            const double pvc = __shfl_up(vc, off, WAVE);
            if (lane >= off) {
                if (!f) {
                    vi = pvi + vi;
                    vc = pvc + vc;
                }
                f |= pf;
            }
        }
        uint32_t ef = __shfl_up(f, 1, WAVE);
        double ei = __shfl_up(vi, 1, WAVE), ec = __shfl_up(vc, 1, WAVE);
        if (lane == 0) {
            ef = 0;
            ei = ec = 0.0;
        }
        // what the waves below, and the chunk before, left open
        double pi = ci, pc = cc;
        if (NW > 1) {
            if (lane == WAVE - 1) {
                s_wf[wv] = f;
                s_wv[wv][1] = vi;
                s_wv[wv][2] = vc;
            }
            __syncthreads();
            for (uint32_t v = 0; v < NW; ++v) {
                if (v == wv && !ef) {
                    ei = pi + ei;
                    ec = pc + ec;
                }
                pi = s_wf[v] ? s_wv[v][1] : pi + s_wv[v][1];
                pc = s_wf[v] ? s_wv[v][2] : pc + s_wv[v][2];
            }
        } else {
            if (!ef) {
                ei = pi + ei;
                ec = pc + ec;
            }
            const uint32_t tf = __shfl(f, WAVE - 1, WAVE);
            const double ti = __shfl(vi, WAVE - 1, WAVE);
            const double tc = __shfl(vc, WAVE - 1, WAVE);
            pi = tf ? ti : pi + ti;
            pc = tf ? tc : pc + tc;
        }
        if (closed) {
            const double si = ei + hi_, sc = ec + hc_;
            ig[first] = si;
            cv[first] = sc;
            mn[first] = tbatch::mean_of(si, sc);
        }

        // ---- carry --------------------------------------------------------
        ci = pi;
        cc = pc;
        const uint32_t ie = partition(key, S, E, j0, dcount, start, w);
        if (ie) kprev = key[slot(ie - 1)];
        i0 += ie;
        j0 += dcount - ie;
        __syncthreads();  // the staged chunk and the wave totals are read
    } while (left > dcount);

    // the last batch is open at the end of the row; n; width
#pragma unroll
    for (uint32_t off = WAVE / 2; off >= 1; off >>= 1)
        cnt += __shfl_xor(cnt, off, WAVE);
    if (NW > 1) {
        if (lane == 0) s_wf[wv] = cnt;
        __syncthreads();
        cnt = 0;
        for (uint32_t v = 0; v < NW; ++v) cnt += s_wf[v];
    }
    if (live && g == 0) {
        if (run) {
            ig[K - 1] = ci;
            cv[K - 1] = cc;
            mn[K - 1] = tbatch::mean_of(ci, cc);
        }
        a.n_out[r] = (double)cnt;
        a.width_out[r] = w;
    }
}

}  // namespace

extern "C" {

// Host arrays in and out: host_x and host_t [T][stride] (T - 1 full rows and
// N values of the last), host_len[T] or null, host_start[T], host_end[T];
// n_out[T], width_out[T], integral_out, covered_out and mean_out [T][K].
// elapsed_ms (nullable) is the kernel alone.  Returns 0, -1 on bad
// arguments, or the HIP error.
int cimba_time_batches_gpu(const double* host_x, const double* host_t,
                           uint64_t T, uint64_t N, uint64_t stride,
                           const uint32_t* host_len, const double* host_start,
                           const double* host_end, uint32_t K, int device,
                           double* n_out, double* width_out,
                           double* integral_out, double* covered_out,
                           double* mean_out, double* elapsed_ms) {
    if (!tbatch::args_ok(T, N, stride, K) || !tbatch::grid_ok(T, N, K))
        return -1;
    HIP_TRY(hipSetDevice(device));
    const size_t nx = (size_t)((T - 1) * stride + N);
    const size_t no = (size_t)T * K;
    cmb_hip::DevBuf<double> d_x, d_t, d_win, d_row, d_out;
    cmb_hip::DevBuf<uint32_t> d_len;
    HIP_TRY(d_x.alloc(nx ? nx : 1));
    HIP_TRY(d_t.alloc(nx ? nx : 1));
    HIP_TRY(d_win.alloc(2 * T));  // start, end
    HIP_TRY(d_row.alloc(2 * T));  // n, width
    HIP_TRY(d_out.alloc(3 * no));  // integral, covered, mean
    if (nx) {
        HIP_TRY(d_x.upload(host_x, nx));
        HIP_TRY(d_t.upload(host_t, nx));
    }
    HIP_TRY(hipMemcpy(d_win.get(), host_start, sizeof(double) * T,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_win.get() + T, host_end, sizeof(double) * T,
                      hipMemcpyHostToDevice));
    if (host_len) {
        HIP_TRY(d_len.alloc(T));
        HIP_TRY(d_len.upload(host_len, T));
    }
    const Args a = {d_x.get(),   d_t.get(),         T,
                    N,           stride,            d_len.get(),
                    d_win.get(), d_win.get() + T,   K,
                    d_row.get(), d_row.get() + T,   d_out.get(),
                    d_out.get() + no, d_out.get() + 2 * no};

    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    if (N + K <= tbatch::WAVE_MAX) {
        const uint64_t rows = WG / WAVE;
        hipLaunchKernelGGL(tbatch_kernel<WAVE>,
                           dim3((uint32_t)((T + rows - 1) / rows)), dim3(WG),
                           0, 0, a);
    } else {
        hipLaunchKernelGGL(tbatch_kernel<WG>, dim3((uint32_t)T), dim3(WG), 0,
                           0, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;

    HIP_TRY(d_row.download(n_out, T));
    HIP_TRY(hipMemcpy(width_out, d_row.get() + T, sizeof(double) * T,
                      hipMemcpyDeviceToHost));
    HIP_TRY(d_out.download(integral_out, no));
    HIP_TRY(hipMemcpy(covered_out, d_out.get() + no, sizeof(double) * no,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mean_out, d_out.get() + 2 * no, sizeof(double) * no,
                      hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
