// M/G/1 DES kernel entry point (templates in deskernel_impl.hpp).
#include "deskernel_impl.hpp"

#include "../models/mg1.hpp"

using cmb::Engine;
using cmb_models::MG1;
using namespace cmb_dk;

static_assert(sizeof(Engine<MG1>::Storage) * 4 < 64 * 1024, "MG1 LDS plan");
// conv_lds_kernel residency is bought with hot bytes per lane: a field
// added to a hot header fails here instead of silently costing a wave
static_assert(LdsHotPlan<MG1>::HS == 376, "MG1 hot lane stride");
static_assert(LdsHotPlan<MG1>::WAVES_PER_CU == 6, "MG1 LDS plan: 6 waves/CU");

extern "C" {

// conv_lds_kernel's plan for M/G/1: {sizeof(Hot), lane stride, waves/CU}
void cimba_mg1_lds_layout(uint32_t out3[3]) {
    out3[0] = (uint32_t)sizeof(LdsHotPlan<MG1>::Hot);
    out3[1] = LdsHotPlan<MG1>::HS;
    out3[2] = LdsHotPlan<MG1>::WAVES_PER_CU;
}

// MG1: results array provided by caller (per-trial)
int cimba_mg1_gpu_run(uint64_t ntrials, const void* params, uint64_t seed,
                      uint64_t trial_base, int device, double* elapsed_ms,
                      void* results_out) {
    HIP_TRY(hipSetDevice(device));
    const auto b = unbounded_batch<MG1>(*(const MG1::Params*)params, ntrials,
                                        seed, trial_base, elapsed_ms,
                                        results_out);
    // CIMBA_MG1_LANE: 0 = wave kernel, 2 = scratch lanes, 3 = vote-gated
    // conv, 4 = conv with the hot engine state in LDS.
    // measured: vote-gated conv at MINW=4 = 4.19 G ev/s vs 3.69 G
    // scratch — MG1 has a wider path mix (service-distribution
    // branches), so path convergence pays where it did not for M/M/1
    // and with the hot engine state in LDS (mode 4) the conv loop
    // measured 7.60 G against 4.84 G (profiles/r04_lds_hot_tier.md), and
    // 9.7 G at 6 waves per CU (profiles/r09_hot_shrink.md)
    const int lane_mode =
        env_int("CIMBA_MG1_LANE").value_or(ntrials >= 32768 ? 4 : 0);
    if (lane_mode == 4)  // default: conv loop, hot state in LDS
        return run_lds_auto<MG1>(b);
    if (lane_mode == 3) return run_conv_auto<MG1>(b);
    if (lane_mode != 0) return run_scratch_auto<MG1>(b, 2048u);
    const int minw = env_int("CIMBA_MG1_MINW").value_or(4);
    if (minw >= 4) return run_trials_gpu<MG1, 4, 4>(b);
    if (minw == 3) return run_trials_gpu<MG1, 4, 3>(b);
    return run_trials_gpu<MG1, 4>(b);
}

}  // extern "C"
