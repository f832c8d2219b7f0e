// Pooling kernel of the device tally stream (include/cimba/tally.hpp):
// column sums of the per-trial 32-bit histograms into one 64-bit
// histogram per tally.
//
// Threads along x own adjacent bins, so a wave reads 256 contiguous bytes
// of one trial's row; grid.y splits the trials into slabs.  Each thread
// sums its column over its slab in a 64-bit register and then issues one
// vector atomicAdd on unsigned long long into the zeroed output.  The
// sums are integers: the result does not depend on the order of the adds
// and equals the host sum exactly.  The rows are read in place inside the
// TallyRec arena (row_stride = sizeof(TallyRec) / 4) or from a dense
// [count][K][NBINS] array (row_stride = NBINS).
//
// Memory-bound: every bin word is read once.  A slab of 256 trials keeps
// the atomics at 1/256 of the loads and still gives a 65536-trial window
// 256 slabs x 7 column blocks to fill the chip.
#include <hip/hip_runtime.h>

#include "../include/cimba/tally.hpp"
#include "hip_host.hpp"

namespace {

constexpr uint32_t REDUCE_WG = 256;
constexpr uint64_t REDUCE_SLAB = 256;  // trials per grid.y slab, at least
constexpr uint64_t REDUCE_MAX_SLABS = 65535;

__global__ __launch_bounds__(REDUCE_WG) void tally_reduce_kernel(
    const uint32_t* __restrict__ rows, uint64_t count, uint32_t K,
    uint64_t row_stride, uint64_t slab,
    unsigned long long* __restrict__ pooled) {
    const uint32_t col = blockIdx.x * REDUCE_WG + threadIdx.x;
    if (col >= K * cmb::TALLY_NBINS) return;
    const uint32_t k = col / cmb::TALLY_NBINS;
    const uint32_t b = col - k * cmb::TALLY_NBINS;
    const uint64_t t0 = (uint64_t)blockIdx.y * slab;
    const uint64_t t1 = t0 + slab < count ? t0 + slab : count;
    const uint64_t step = (uint64_t)K * row_stride;  // trial to trial
    const uint32_t* p = rows + (t0 * K + k) * row_stride + b;
    unsigned long long acc = 0;
#pragma unroll 8
    for (uint64_t t = t0; t < t1; ++t, p += step) acc += *p;
    if (acc) atomicAdd(&pooled[col], acc);
}

}  // namespace

extern "C" {

// device pointers; see deskernel_impl.hpp for the contract
int cimba_tally_reduce_gpu(const uint32_t* per_trial, uint64_t count,
                           uint32_t K, uint64_t row_stride, uint64_t* pooled) {
    if (K < 1 || K > (uint32_t)cmb::TALLY_MAX_K ||
        row_stride < cmb::TALLY_NBINS)
        return cmb::TALLY_ERR_BAD_SINK;
    const uint32_t cols = K * cmb::TALLY_NBINS;
    HIP_TRY(hipMemsetAsync(pooled, 0, sizeof(uint64_t) * cols, 0));
    if (count == 0) return 0;
    uint64_t slab = REDUCE_SLAB;
    if ((count + slab - 1) / slab > REDUCE_MAX_SLABS)
        slab = (count + REDUCE_MAX_SLABS - 1) / REDUCE_MAX_SLABS;
    const dim3 grid((cols + REDUCE_WG - 1) / REDUCE_WG,
                    (uint32_t)((count + slab - 1) / slab));
    hipLaunchKernelGGL(tally_reduce_kernel, grid, dim3(REDUCE_WG), 0, 0,
                       per_trial, count, K, row_stride, slab,
                       (unsigned long long*)pooled);
    return (int)hipGetLastError();
}

// test hook: a dense HOST array [count][K][NBINS] in, pooled[K][NBINS]
// out; elapsed_ms (nullable) is the kernel with its memset alone
int cimba_tally_reduce_host(const uint32_t* host_rows, uint64_t count,
                            uint32_t K, int device, uint64_t* host_pooled,
                            double* elapsed_ms) {
    if (K < 1 || K > (uint32_t)cmb::TALLY_MAX_K)
        return cmb::TALLY_ERR_BAD_SINK;
    HIP_TRY(hipSetDevice(device));
    const size_t cols = (size_t)K * cmb::TALLY_NBINS;
    cmb_hip::DevBuf<uint32_t> d_rows;
    cmb_hip::DevBuf<uint64_t> d_pooled;
    HIP_TRY(d_rows.alloc(count ? count * cols : 1));
    HIP_TRY(d_pooled.alloc(cols));
    if (count) HIP_TRY(d_rows.upload(host_rows, count * cols));
    cmb_hip::EventTimer timer;
    double ms = 0.0;
    HIP_TRY(timer.start());
    HIP_TRY(cimba_tally_reduce_gpu(d_rows.get(), count, K, cmb::TALLY_NBINS,
                                   d_pooled.get()));
    HIP_TRY(timer.stop(&ms));
    if (elapsed_ms) *elapsed_ms = ms;
    return d_pooled.download(host_pooled, cols);
}

}  // extern "C"
