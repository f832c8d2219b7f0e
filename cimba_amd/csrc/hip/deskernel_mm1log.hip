// Logged M/M/1 DES kernel entry point (templates in deskernel_impl.hpp):
// the worked model for the device log stream (include/cimba/devlog.hpp).
// One MINW per kernel kind stays instantiated — this model exists to show
// and test logging through every kernel shape, not to be tuned.
#include "deskernel_impl.hpp"

#include "../models/mm1_logged.hpp"

using cmb::Engine;
using cmb_models::MM1Log;
using namespace cmb_dk;

static_assert(sizeof(Engine<MM1Log>::Storage) * 4 < 60 * 1024,
              "MM1Log LDS plan");
static_assert(sizeof(Engine<MM1Log>::Storage) ==
                  sizeof(Engine<cmb_models::MM1>::Storage),
              "logging adds no per-trial storage");

extern "C" {

// kernel: 0 = wave (trial per wavefront), 1 = lane (HBM stores),
// 2 = scratch, 3 = conv (vote-gated).  blocks: grid cap, 0 = default.
// log_sink (nullable): HOST buffers sized for the clipped window
// (cmb::log_clip_window).  Returns 0, a hipError_t, or a negative
// cmb::LOG_ERR_* code — the latter before any device call.
int cimba_mm1log_gpu_run(uint64_t ntrials, double arr_mean, double srv_mean,
                         uint64_t num_objects, uint64_t seed,
                         uint64_t trial_base, int device, int kernel,
                         uint32_t blocks, const cmb::LogSink* log_sink,
                         double* elapsed_ms, void* results_out) {
    if (kernel < 0 || kernel > 3) return cmb::LOG_ERR_BAD_SINK;
    if (const int lrc = cmb::log_sink_check(log_sink, trial_base, ntrials))
        return lrc;
    HIP_TRY(hipSetDevice(device));
    const auto b = unbounded_batch<MM1Log>(
        {arr_mean, srv_mean, num_objects}, ntrials, seed, trial_base,
        elapsed_ms, results_out, log_sink);
    const uint32_t lane_blocks = blocks ? blocks : 2048u;
    switch (kernel) {
        case 0: return run_trials_gpu<MM1Log, 4, 4>(b, blocks);
        case 1: return run_trials_gpu_lane<MM1Log, 1>(b, lane_blocks);
        case 2: return run_trials_gpu_lane_scratch<MM1Log, 1>(b, lane_blocks);
        default: return run_trials_gpu_conv<MM1Log, 4>(b, blocks);
    }
}

}  // extern "C"
