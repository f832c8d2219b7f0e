// Bulk-sampling layout shared by the gfx950 kernels (hip/rng_kernel.hip)
// and the host lane reference (bindings.cpp rng_sample_lanes): launch
// geometry, distribution ids, the per-lane seed and the per-sample
// dispatch.  One definition, so the two sides cannot drift apart.
//
// Layout: `lanes` independent sfc64 streams; lane g is seeded with
// lane_seed(seed, g) and sample i is draw i / lanes of lane i % lanes.
#pragma once

#include "rng.hpp"

namespace cmb {
namespace bulk {

constexpr uint32_t BLOCK = 256;            // threads per block
constexpr uint32_t DEFAULT_BLOCKS = 2048;  // 524288 lanes
constexpr uint32_t MAX_BLOCKS = 2048;

CMB_FORCEINLINE bool blocks_ok(uint32_t blocks) {
    return blocks >= 1 && blocks <= MAX_BLOCKS;
}

enum DistId : int {
    DIST_U01 = 0,
    DIST_STD_NORMAL = 1,
    DIST_STD_EXPONENTIAL = 2,
    DIST_GAMMA = 3,    // p0 = shape
    DIST_POISSON = 4,  // p0 = mean
};

CMB_FORCEINLINE uint64_t lane_seed(uint64_t seed, uint64_t gid) {
    return fmix64(seed ^ (gid * UINT64_C(0x9E3779B97F4A7C15) + 1));
}

CMB_FORCEINLINE double sample_one(Rng& r, int dist, double p0) {
    switch (dist) {
        case DIST_STD_NORMAL: return r.std_normal();
        case DIST_STD_EXPONENTIAL: return r.std_exponential();
        case DIST_GAMMA: return r.std_gamma(p0);
        case DIST_POISSON: return (double)r.poisson(p0);
        default: return r.u01();
    }
}

}  // namespace bulk
}  // namespace cmb
