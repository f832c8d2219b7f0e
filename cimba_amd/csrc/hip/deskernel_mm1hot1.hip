// MM1Hot1 DES kernel entry point (templates in deskernel_impl.hpp): M/M/1
// with a one-entry hot heap tier, always on the LDS kernel.  Its second
// pending event lives in the cold (scratch) tier, so every sift crosses
// the hot/cold boundary that MM1 itself never reaches.  A test model, not
// a tuned one: results must equal cimba_mm1_gpu_run_pt's bit for bit.
// CIMBA_MM1_LANE=5 picks the fused loop, as it does for MM1, and 6 the
// register-heap kernel: its one hot entry then lives in a register and the
// second event in scratch, so every push and pop crosses that boundary.
#include "deskernel_impl.hpp"

#include "../models/mm1.hpp"
#include "mm1_gpu_out.hpp"

using cmb::Engine;
using cmb_models::MM1Hot1;
using namespace cmb_dk;

static_assert(Engine<MM1Hot1>::HOT_EV == 1, "one hot heap entry");
static_assert(sizeof(Engine<MM1Hot1>::Storage) ==
                  sizeof(Engine<cmb_models::MM1>::Storage),
              "the tiers only split the same storage differently");
static_assert(LdsHotPlan<MM1Hot1>::WAVES_PER_CU >= 8, "MM1Hot1 LDS plan");

extern "C" {

int cimba_mm1hot1_gpu_run_pt(uint64_t ntrials, double arr_mean,
                             double srv_mean, uint64_t num_objects,
                             uint64_t seed, uint64_t trial_base, int device,
                             double until, uint64_t max_events, Mm1GpuOut* out,
                             double* per_trial_avg_out) {
    HIP_TRY(hipSetDevice(device));
    std::vector<MM1Hot1::Result> res(ntrials);
    const TrialBatch<MM1Hot1> b{{arr_mean, srv_mean, num_objects}, ntrials,
                                seed, trial_base, until, max_events,
                                &out->elapsed_ms, res.data()};
    const int lane_mode = env_int("CIMBA_MM1_LANE").value_or(4);
    if (lane_mode == 6)
        HIP_TRY(run_lds_regheap<MM1Hot1>(b));
    else if (lane_mode == 5)
        HIP_TRY(run_lds_fused<MM1Hot1>(b));
    else
        HIP_TRY(run_lds_auto<MM1Hot1>(b));
    mm1_aggregate(res.data(), ntrials, out, per_trial_avg_out);
    return 0;
}

}  // extern "C"
