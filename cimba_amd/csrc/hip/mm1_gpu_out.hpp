// Batch totals of an M/M/1-shaped device run, shared by the entry points
// that return them (deskernel.hip, deskernel_mm1hot1.hip).
#pragma once

#include <cstdint>

extern "C" {
struct Mm1GpuOut {
    double elapsed_ms;
    uint64_t total_events;
    uint64_t total_objs;
    double total_wait;
    uint64_t trials_ok;
    int32_t first_bad_status;
    int32_t pad_;
};
}

// fold per-trial results (in trial order) into the totals;
// per_trial_avg_out (nullable): per-trial average system times
template <class Result>
inline void mm1_aggregate(const Result* res, uint64_t ntrials, Mm1GpuOut* out,
                          double* per_trial_avg_out) {
    out->total_events = 0;
    out->total_objs = 0;
    out->total_wait = 0.0;
    out->trials_ok = 0;
    out->first_bad_status = 0;
    for (uint64_t i = 0; i < ntrials; ++i) {
        out->total_events += res[i].events;
        out->total_objs += res[i].obj_cnt;
        out->total_wait += res[i].sum_wait;
        if (per_trial_avg_out)
            per_trial_avg_out[i] =
                res[i].obj_cnt ? res[i].sum_wait / (double)res[i].obj_cnt
                               : 0.0;
        if (res[i].status == 0)
            ++out->trials_ok;
        else if (out->first_bad_status == 0)
            out->first_bad_status = res[i].status;
    }
}
