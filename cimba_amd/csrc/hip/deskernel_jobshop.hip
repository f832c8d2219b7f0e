// Job-shop DES kernel entry point (templates in deskernel_impl.hpp).
#include "deskernel_impl.hpp"

#include "../models/jobshop.hpp"

using cmb::Engine;
using cmb_models::JobShop;
using namespace cmb_dk;

static_assert(sizeof(Engine<JobShop>::Storage) * 4 < 64 * 1024,
              "JobShop LDS plan");

extern "C" {

int cimba_jobshop_gpu_run(uint64_t ntrials, const void* params,
                          uint64_t seed, uint64_t trial_base, int device,
                          double* elapsed_ms, void* results_out) {
    HIP_TRY(hipSetDevice(device));
    const auto b = unbounded_batch<JobShop>(*(const JobShop::Params*)params,
                                            ntrials, seed, trial_base,
                                            elapsed_ms, results_out);
    // CIMBA_JS_LANE: 0 = wave kernel, 3 = vote-gated conv, any other
    // value = HBM lanes.
    // measured: with the heap-top cache the vote-gated conv kernel
    // edges HBM-lane for JobShop too (1.41 vs 1.40 G ev/s)
    const int lane_mode =
        env_int("CIMBA_JS_LANE").value_or(ntrials >= 32768 ? 3 : 0);
    if (lane_mode == 3) return run_conv_auto<JobShop>(b);
    if (lane_mode != 0) {
        // HBM-lane variant: measured faster than scratch for JobShop's
        // larger store; MINW knob as elsewhere
        const int lminw = env_int("CIMBA_JS_LANE_MINW").value_or(1);
        if (lminw >= 3) return run_trials_gpu_lane<JobShop, 3>(b, 2048u);
        if (lminw == 2) return run_trials_gpu_lane<JobShop, 2>(b, 2048u);
        return run_trials_gpu_lane<JobShop, 1>(b, 2048u);
    }
    const int minw = env_int("CIMBA_JS_MINW").value_or(4);
    if (minw >= 4) return run_trials_gpu<JobShop, 4, 4>(b);
    return run_trials_gpu<JobShop, 4>(b);
}

}  // extern "C"
