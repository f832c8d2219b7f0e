// gfx950 bulk-sampling kernels: the device-wide batched counterpart of the
// reference's ziggurat samplers (reference src/cmb_random.c:148-175 +
// codegen tables; BASELINE.json north star: "ziggurat normal/exponential
// sampling as a hand-written CDNA4 kernel ... shown with rocprof
// counters").
//
// Unlike the in-trial RNG (one sequential stream per trial wavefront),
// these kernels run all 64 lanes of every wave: lane-parallel independent
// sfc64 streams (fmix64-derived per-lane seeds), grid-stride over the
// output, coalesced 8B stores.  The ziggurat common path is ~15 ALU ops +
// one 8B constant-cache table read per sample; rejection handling is
// per-lane (divergence cost ~2-3% at the published acceptance rates).
// A fused moment-reduction variant accumulates raw sums (n, Sx, Sx2, Sx3,
// Sx4, min, max) through wave shuffles + one atomic per wave, so 1e9+
// sample statistical tests never materialize the samples.
#include <hip/hip_runtime.h>

#include "../include/cimba/bulk_rng.hpp"
#include "hip_host.hpp"

namespace {

using cmb::Rng;
using cmb::bulk::sample_one;

__global__ __launch_bounds__(cmb::bulk::BLOCK) void sample_kernel(
    int dist, double p0, uint64_t n, uint64_t seed, double* __restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    Rng r;
    r.seed(cmb::bulk::lane_seed(seed, gid));
    for (uint64_t i = gid; i < n; i += stride) {
        out[i] = sample_one(r, dist, p0);
    }
}

struct MomentAcc {
    double n, s1, s2, s3, s4, mn, mx;
};

__global__ __launch_bounds__(cmb::bulk::BLOCK) void sample_moments_kernel(
    int dist, double p0, uint64_t n, uint64_t seed,
    MomentAcc* __restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    Rng r;
    r.seed(cmb::bulk::lane_seed(seed, gid));
    double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    double mn = 1e308, mx = -1e308;
    uint64_t cnt = 0;
    for (uint64_t i = gid; i < n; i += stride) {
        const double x = sample_one(r, dist, p0);
        const double x2 = x * x;
        s1 += x;
        s2 += x2;
        s3 += x2 * x;
        s4 += x2 * x2;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        ++cnt;
    }
    // wave-level butterfly reduction over the 64 lanes
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off);
        s2 += __shfl_down(s2, off);
        s3 += __shfl_down(s3, off);
        s4 += __shfl_down(s4, off);
        cnt += (uint64_t)__shfl_down((unsigned long long)cnt, off);
        const double omn = __shfl_down(mn, off);
        const double omx = __shfl_down(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out->n, (double)cnt);
        atomicAdd(&out->s1, s1);
        atomicAdd(&out->s2, s2);
        atomicAdd(&out->s3, s3);
        atomicAdd(&out->s4, s4);
        // f64 atomic min/max via CAS loop (rare after wave reduce)
        unsigned long long* pmn = (unsigned long long*)&out->mn;
        unsigned long long old = *pmn, assumed;
        do {
            assumed = old;
            if (__longlong_as_double(assumed) <= mn) break;
            old = atomicCAS(pmn, assumed, __double_as_longlong(mn));
        } while (old != assumed);
        unsigned long long* pmx = (unsigned long long*)&out->mx;
        old = *pmx;
        do {
            assumed = old;
            if (__longlong_as_double(assumed) >= mx) break;
            old = atomicCAS(pmx, assumed, __double_as_longlong(mx));
        } while (old != assumed);
    }
}


// MFMA-assisted variant (the north star asked for "MFMA for the batched
// table lookups/rejection math"; the A/B and the analysis live in
// profiles/r02_mfma_ziggurat.md).  The rejection/table math itself has
// no GEMM shape — per-sample work is independent elementwise int64/f64
// ops — so the only productive MFMA mapping is the MOMENT ACCUMULATION:
// v_mfma_f64_16x16x4_f64 with B = ones folds each lane's power value
// into the accumulator tile, offloading the 4 f64 adds per sample from
// the VALU onto the (otherwise idle) matrix pipe.
typedef __attribute__((ext_vector_type(4))) double f64x4;

__global__ __launch_bounds__(cmb::bulk::BLOCK) void sample_moments_mfma_kernel(
    int dist, double p0, uint64_t n, uint64_t seed,
    MomentAcc* __restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    Rng r;
    r.seed(cmb::bulk::lane_seed(seed, gid));
    // D[i][j] += sum_k A[i][k] * B[k][j]; with B = ones every lane's A
    // value lands in its row's running sums — 4 power accumulators
    f64x4 d1 = {0, 0, 0, 0}, d2 = {0, 0, 0, 0};
    f64x4 d3 = {0, 0, 0, 0}, d4 = {0, 0, 0, 0};
    double mn = 1e308, mx = -1e308;
    uint64_t cnt = 0;
    // MFMA does not honour the EXEC mask: it reads the A operand of all 64
    // lanes, whether or not they are still in the loop.  So the trip count
    // is wave-uniform (driven by the wave's first lane) and a lane past n
    // contributes 0.0 instead of whatever its register last held.
    const uint64_t lane = threadIdx.x & 63;
    for (uint64_t i = gid; i - lane < n; i += stride) {
        double x = 0.0;
        if (i < n) {
            x = sample_one(r, dist, p0);
            mn = x < mn ? x : mn;
            mx = x > mx ? x : mx;
            ++cnt;
        }
        const double x2 = x * x;
        d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, 1.0, d1, 0, 0, 0);
        d2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, 1.0, d2, 0, 0, 0);
        d3 = __builtin_amdgcn_mfma_f64_16x16x4f64(x2 * x, 1.0, d3, 0, 0, 0);
        d4 = __builtin_amdgcn_mfma_f64_16x16x4f64(x2 * x2, 1.0, d4, 0, 0, 0);
    }
    // every D column holds the same row sums (B = ones): col 0 lanes own
    // rows (lane>>4)*4+r; fold rows via the same wave butterfly
    double s1 = d1[0] + d1[1] + d1[2] + d1[3];
    double s2 = d2[0] + d2[1] + d2[2] + d2[3];
    double s3 = d3[0] + d3[1] + d3[2] + d3[3];
    double s4 = d4[0] + d4[1] + d4[2] + d4[3];
    if ((threadIdx.x & 15) != 0) {  // only col-0 lanes carry real sums
        s1 = s2 = s3 = s4 = 0.0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off);
        s2 += __shfl_down(s2, off);
        s3 += __shfl_down(s3, off);
        s4 += __shfl_down(s4, off);
        cnt += (uint64_t)__shfl_down((unsigned long long)cnt, off);
        const double omn = __shfl_down(mn, off);
        const double omx = __shfl_down(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out->n, (double)cnt);
        atomicAdd(&out->s1, s1);
        atomicAdd(&out->s2, s2);
        atomicAdd(&out->s3, s3);
        atomicAdd(&out->s4, s4);
        unsigned long long* pmn = (unsigned long long*)&out->mn;
        unsigned long long old = *pmn, assumed;
        do {
            assumed = old;
            if (__longlong_as_double(assumed) <= mn) break;
            old = atomicCAS(pmn, assumed, __double_as_longlong(mn));
        } while (old != assumed);
        unsigned long long* pmx = (unsigned long long*)&out->mx;
        old = *pmx;
        do {
            assumed = old;
            if (__longlong_as_double(assumed) >= mx) break;
            old = atomicCAS(pmx, assumed, __double_as_longlong(mx));
        } while (old != assumed);
    }
}

}  // namespace

extern "C" {

// `blocks` is the grid size (cmb::bulk::DEFAULT_BLOCKS unless a test wants
// few lanes with deep per-lane streams); lanes = blocks * cmb::bulk::BLOCK.
int cimba_sample_gpu(int dist, double p0, uint64_t n, uint64_t seed,
                     int device, double* host_out, double* elapsed_ms,
                     uint32_t blocks) {
    if (!cmb::bulk::blocks_ok(blocks)) return (int)hipErrorInvalidValue;
    HIP_TRY(hipSetDevice(device));
    cmb_hip::DevBuf<double> d_out;
    HIP_TRY(d_out.alloc(n));
    cmb_hip::EventTimer timer;
    HIP_TRY(timer.start());
    hipLaunchKernelGGL(sample_kernel, dim3(blocks), dim3(cmb::bulk::BLOCK), 0,
                       0, dist, p0, n, seed, d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.stop(elapsed_ms));
    return d_out.download(host_out, n);
}

int cimba_sample_moments_gpu2(int dist, double p0, uint64_t n,
                              uint64_t seed, int device, int use_mfma,
                              double* out7, double* elapsed_ms,
                              uint32_t blocks);

int cimba_sample_moments_gpu(int dist, double p0, uint64_t n, uint64_t seed,
                             int device, double* out7, double* elapsed_ms) {
    return cimba_sample_moments_gpu2(dist, p0, n, seed, device, 0, out7,
                                     elapsed_ms, cmb::bulk::DEFAULT_BLOCKS);
}

int cimba_sample_moments_gpu2(int dist, double p0, uint64_t n,
                              uint64_t seed, int device, int use_mfma,
                              double* out7, double* elapsed_ms,
                              uint32_t blocks) {
    if (!cmb::bulk::blocks_ok(blocks)) return (int)hipErrorInvalidValue;
    HIP_TRY(hipSetDevice(device));
    MomentAcc h{0, 0, 0, 0, 0, 1e308, -1e308};
    cmb_hip::DevBuf<MomentAcc> d;
    HIP_TRY(d.alloc(1));
    HIP_TRY(d.upload(&h));
    cmb_hip::EventTimer timer;
    HIP_TRY(timer.start());
    if (use_mfma)
        hipLaunchKernelGGL(sample_moments_mfma_kernel, dim3(blocks),
                           dim3(cmb::bulk::BLOCK), 0, 0, dist, p0, n, seed,
                           d.get());
    else
        hipLaunchKernelGGL(sample_moments_kernel, dim3(blocks),
                           dim3(cmb::bulk::BLOCK), 0, 0, dist, p0, n, seed,
                           d.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.stop(elapsed_ms));
    HIP_TRY(d.download(&h));
    out7[0] = h.n;
    out7[1] = h.s1;
    out7[2] = h.s2;
    out7[3] = h.s3;
    out7[4] = h.s4;
    out7[5] = h.mn;
    out7[6] = h.mx;
    return 0;
}

}  // extern "C"
