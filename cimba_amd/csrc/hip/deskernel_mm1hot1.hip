// MM1Hot1 DES kernel entry point (templates in deskernel_impl.hpp): M/M/1
// with a one-entry hot heap tier, always on the LDS kernel.  Its second
// pending event lives in the cold (scratch) tier, so every sift crosses
// the hot/cold boundary that MM1 itself never reaches.  A test model, not
// a tuned one: results must equal cimba_mm1_gpu_run_pt's bit for bit.
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
    HIP_TRY(run_lds_auto<MM1Hot1>({{arr_mean, srv_mean, num_objects}, ntrials,
                                   seed, trial_base, until, max_events,
                                   &out->elapsed_ms, res.data()}));
    mm1_aggregate(res.data(), ntrials, out, per_trial_avg_out);
    return 0;
}

}  // extern "C"
