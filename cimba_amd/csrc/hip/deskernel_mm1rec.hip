// MM1Rec DES kernel entry point (templates in deskernel_impl.hpp): M/M/1
// with the queue's length history on, so every put and get updates the
// time-weighted statistics record in the cold half of the storage.  A
// test model, not a tuned one: lane_mode 4 runs the LDS kernel, anything
// else the all-scratch conv kernel, and the two must agree bit for bit.
#include "deskernel_impl.hpp"

#include "../models/mm1.hpp"
#include "mm1_gpu_out.hpp"

using cmb::Engine;
using cmb_models::MM1Rec;
using namespace cmb_dk;

static_assert(sizeof(Engine<MM1Rec>::Storage) ==
                  sizeof(Engine<cmb_models::MM1>::Storage),
              "recording changes no layout");

extern "C" {

// out->total_wait sums the per-trial mean queue lengths and
// out->total_objs counts the trials; per_trial_avg_out gets each mean
int cimba_mm1rec_gpu_run_pt(uint64_t ntrials, double arr_mean,
                            double srv_mean, uint64_t num_objects,
                            uint64_t seed, uint64_t trial_base, int device,
                            int lane_mode, Mm1GpuOut* out,
                            double* per_trial_avg_out) {
    HIP_TRY(hipSetDevice(device));
    std::vector<MM1Rec::Result> res(ntrials);
    const auto b = unbounded_batch<MM1Rec>({arr_mean, srv_mean, num_objects},
                                           ntrials, seed, trial_base,
                                           &out->elapsed_ms, res.data());
    if (lane_mode == 4) {
        HIP_TRY(run_lds_auto<MM1Rec>(b));
    } else {
        const uint32_t blocks =
            (uint32_t)env_int("CIMBA_CONV_BLOCKS").value_or(0);
        HIP_TRY((run_trials_gpu_conv<MM1Rec, 4>(b, blocks)));
    }
    mm1_aggregate(res.data(), ntrials, out, per_trial_avg_out);
    return 0;
}

}  // extern "C"
