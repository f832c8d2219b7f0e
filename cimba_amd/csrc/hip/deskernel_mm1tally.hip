// Tallied M/M/1 DES kernel entry point (templates in deskernel_impl.hpp):
// the worked model for the device tally stream (include/cimba/tally.hpp).
// One MINW per kernel kind stays instantiated — this model exists to show
// and test tallies through every kernel shape, not to be tuned.
#include "deskernel_impl.hpp"

#include "../models/mm1_tally.hpp"

using cmb::Engine;
using cmb_models::MM1Tally;
using namespace cmb_dk;

static_assert(sizeof(Engine<MM1Tally>::Storage) * 4 < 60 * 1024,
              "MM1Tally LDS plan");
static_assert(sizeof(Engine<MM1Tally>::Storage) ==
                  sizeof(Engine<cmb_models::MM1>::Storage),
              "tallies add no per-trial storage");

extern "C" {

// kernel: 0 = wave (trial per wavefront), 1 = lane (HBM stores),
// 2 = scratch, 3 = conv (vote-gated), 4 = lds (conv, hot state in LDS).
// blocks: grid cap, 0 = default.  tally_sink (nullable): HOST buffers sized
// for the clipped window (cmb::tally_clip_window).  Returns 0, a
// hipError_t, or a negative cmb::TALLY_ERR_* code — the latter before any
// device call.
int cimba_mm1tally_gpu_run(uint64_t ntrials, double arr_mean, double srv_mean,
                           uint64_t num_objects, uint64_t seed,
                           uint64_t trial_base, int device, int kernel,
                           uint32_t blocks, cmb::TallyRequest* tally_sink,
                           double* elapsed_ms, void* results_out) {
    if (kernel < 0 || kernel > 4) return cmb::TALLY_ERR_BAD_SINK;
    if (tally_sink)
        if (const int trc = cmb::tally_sink_check(
                &tally_sink->window, Engine<MM1Tally>::TALLY_K, trial_base,
                ntrials))
            return trc;
    HIP_TRY(hipSetDevice(device));
    const auto b = unbounded_batch<MM1Tally>(
        {arr_mean, srv_mean, num_objects}, ntrials, seed, trial_base,
        elapsed_ms, results_out, nullptr, tally_sink);
    const uint32_t lane_blocks = blocks ? blocks : 2048u;
    switch (kernel) {
        case 0: return run_trials_gpu<MM1Tally, 4, 4>(b, blocks);
        case 1: return run_trials_gpu_lane<MM1Tally, 1>(b, lane_blocks);
        case 2: return run_trials_gpu_lane_scratch<MM1Tally, 1>(b, lane_blocks);
        case 3: return run_trials_gpu_conv<MM1Tally, 4>(b, blocks);
        default: return run_trials_gpu_conv<MM1Tally, 1, true>(b, blocks);
    }
}

}  // extern "C"
