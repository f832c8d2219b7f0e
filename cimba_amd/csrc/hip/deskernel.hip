// gfx950 DES kernel entry points for the M/M/1 flagship model, plus the
// device utility calls.  The kernel/launcher templates live in
// deskernel_impl.hpp; MG1 / JobShop / Scenario entries compile in their
// own TUs (deskernel_mg1/jobshop/scenario.hip) so hipcc builds the
// models in parallel (the combined TU took ~8 min at -O3).
#include "deskernel_impl.hpp"

#include "../models/mm1.hpp"
#include "mm1_gpu_out.hpp"

using cmb::Engine;
using cmb_models::MM1;
using namespace cmb_dk;

// LDS budget check: 4 engine stores per workgroup, several workgroups/CU
static_assert(sizeof(Engine<MM1>::Storage) * 4 < 60 * 1024, "MM1 LDS plan");
// conv_lds_kernel residency is bought with hot bytes per lane: a field
// added to a hot header fails here instead of silently costing a wave
static_assert(LdsHotPlan<MM1>::HS == 312, "MM1 hot lane stride");
static_assert(LdsHotPlan<MM1>::WAVES_PER_CU == 8, "MM1: 2 waves on every SIMD");

extern "C" {

// per_trial_avg_out (nullable): per-trial average system times, for the
// host-vs-device divergence-count test (tests/test_gpu.py)
int cimba_mm1_gpu_run_pt(uint64_t ntrials, double arr_mean, double srv_mean,
                         uint64_t num_objects, uint64_t seed,
                         uint64_t trial_base, int device, double until,
                         uint64_t max_events, Mm1GpuOut* out,
                         double* per_trial_avg_out);

int cimba_mm1_gpu_run(uint64_t ntrials, double arr_mean, double srv_mean,
                      uint64_t num_objects, uint64_t seed,
                      uint64_t trial_base, int device, double until,
                      uint64_t max_events, Mm1GpuOut* out) {
    return cimba_mm1_gpu_run_pt(ntrials, arr_mean, srv_mean, num_objects,
                                seed, trial_base, device, until, max_events,
                                out, nullptr);
}

int cimba_mm1_gpu_run_pt(uint64_t ntrials, double arr_mean, double srv_mean,
                         uint64_t num_objects, uint64_t seed,
                         uint64_t trial_base, int device, double until,
                         uint64_t max_events, Mm1GpuOut* out,
                         double* per_trial_avg_out) {
    HIP_TRY(hipSetDevice(device));
    std::vector<MM1::Result> res(ntrials);
    const TrialBatch<MM1> b{{arr_mean, srv_mean, num_objects}, ntrials, seed,
                            trial_base, until, max_events, &out->elapsed_ms,
                            res.data()};
    // lane-parallel auto policy: 64 trials/wave needs a large batch to
    // fill the chip; below the threshold the wave-per-trial kernel wins.
    // CIMBA_MM1_LANE: 0 = wave kernel, 1 = HBM lanes, 2 = scratch lanes,
    // 3 = vote-gated conv, 4 = conv with the hot engine state in LDS.
    // Measured (profiles/r02_conv_divergence.md): after the heap-top
    // register cache the vote-gated conv kernel wins for M/M/1 too
    // (4.69 vs 4.55 G ev/s at the bench batch); with the hot engine
    // state in LDS the same loop runs about twice as fast again
    // (profiles/r04_lds_hot_tier.md), so mode 4 is the default
    const int lane_mode =
        env_int("CIMBA_MM1_LANE").value_or(ntrials >= 32768 ? 4 : 0);
    const uint32_t blocks =
        (uint32_t)env_int("CIMBA_MM1_LANE_BLOCKS").value_or(2048);
    // wave kernel's MINW: 5 measured best (profiles/)
    const int minw = env_int("CIMBA_MM1_MINW").value_or(5);
    int rc;
    if (lane_mode == 1)  // explicit HBM-lane variant
        rc = run_trials_gpu_lane<MM1, 1>(b, blocks);
    else if (lane_mode == 2)  // scratch (HW lane-interleaved)
        rc = run_scratch_auto<MM1>(b, blocks);
    else if (lane_mode == 4)  // default: conv loop, hot state in LDS
        rc = run_lds_auto<MM1>(b);
    else if (lane_mode != 0)  // 3: path-converged lanes, all in scratch
        rc = run_conv_auto<MM1>(b);
    else  // wave kernel
        rc = minw == 5   ? run_trials_gpu<MM1, 4, 5>(b)
             : minw == 6 ? run_trials_gpu<MM1, 4, 6>(b)
                         : run_trials_gpu<MM1, 4, 4>(b);
    if (rc) return rc;
    mm1_aggregate(res.data(), ntrials, out, per_trial_avg_out);
    return 0;
}

// conv_lds_kernel's plan for M/M/1: {sizeof(Hot), lane stride, waves/CU}
void cimba_mm1_lds_layout(uint32_t out3[3]) {
    out3[0] = (uint32_t)sizeof(LdsHotPlan<MM1>::Hot);
    out3[1] = LdsHotPlan<MM1>::HS;
    out3[2] = LdsHotPlan<MM1>::WAVES_PER_CU;
}

int cimba_gpu_device_count(int* n) {
    hipError_t err = hipGetDeviceCount(n);
    if (err != hipSuccess) {
        *n = 0;
        return (int)err;
    }
    return 0;
}

int cimba_gpu_sync(void) { return (int)hipDeviceSynchronize(); }

}  // extern "C"
