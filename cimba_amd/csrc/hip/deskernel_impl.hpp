// Shared template implementation for the per-model DES kernel TUs
// (deskernel.hip = M/M/1 + device utils, deskernel_mg1.hip,
// deskernel_jobshop.hip, deskernel_scenario.hip, deskernel_mm1log.hip,
// deskernel_mm1tally.hip, deskernel_mm1hot1.hip).  Split so hipcc compiles
// the models in PARALLEL: each instantiation inlines the whole engine at
// -O3, and one combined TU took ~8 min.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/cimba/runner.hpp"
#include "hip_host.hpp"

// hip/tally_kernel.hip: column sums of per-trial histograms, on the null
// stream.  Row (t, k) starts at per_trial + (t*K + k) * row_stride (in
// 32-bit words) and holds TALLY_NBINS counts; pooled[K][TALLY_NBINS] is
// zeroed here.  All pointers are DEVICE pointers.
extern "C" int cimba_tally_reduce_gpu(const uint32_t* per_trial,
                                      uint64_t count, uint32_t K,
                                      uint64_t row_stride, uint64_t* pooled);

namespace cmb_dk {

using cmb::Engine;
using cmb_hip::DevBuf;
using cmb_hip::env_int;

// generic trial-per-wavefront kernel; WPB = waves (= trials) per workgroup;
// MINW = requested waves/SIMD (caps the register allocator; occupancy knob)
template <class Model, int WPB, int MINW = 1>
__global__ __launch_bounds__(WPB * 64, MINW) __attribute__((flatten)) void trial_kernel(
    typename Model::Params P, uint64_t master_seed, uint64_t trial_base,
    uint32_t ntrials, double until, uint64_t max_events,
    typename Model::Result* __restrict__ out,
    typename Engine<Model>::Spill* __restrict__ sp_arena,
    int32_t* __restrict__ sp_cur, int32_t sp_cap, cmb::LogSink lsink,
    cmb::TallySink tsink) {
    // arrays in LDS; the Engine context (clock, seq, handles, status, RNG
    // state, heap size) is a per-lane local -> register-resident
    __shared__ typename Engine<Model>::Storage st[WPB];
    const int w = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) != 0) return;  // lane 0 of each wave drives
    Engine<Model> E(st[w]);
    E.set_spill_pool(sp_arena, sp_cur, sp_cap);
    if constexpr (Engine<Model>::DEVICE_LOG) E.log_attach(lsink);
    if constexpr (Engine<Model>::TALLY_K > 0) E.tally_attach(tsink);
    const uint32_t stride = gridDim.x * WPB;
    for (uint32_t trial = blockIdx.x * WPB + (uint32_t)w; trial < ntrials;
         trial += stride) {
        E.init(&P, cmb::trial_seed(master_seed, trial_base + trial),
               (uint32_t)(trial_base + trial));
        Model::setup(E);
        E.run(until, max_events);
        Model::finish(E, out[trial]);
        E.log_finish();
    }
}

// Device spill pool: slabs claimed lazily by trials that overflow their
// fast tier (Engine::claim_spill).  Sized far above the measured overflow
// rate (~1 trial per 5e5 at MG1 lognormal SCV=4, rho=0.8) and slabs stay
// claimed by a lane across its later trials, so 4096 covers any batch.
template <class Model>
struct DevSpillPool {
    using Spill = typename cmb::Engine<Model>::Spill;
    DevBuf<Spill> arena;
    DevBuf<int32_t> cursor;
    int32_t cap = 0;
    int alloc(uint64_t ntrials) {
        if constexpr (!cmb::Engine<Model>::NEEDS_SPILL) {
            (void)ntrials;
            return 0;
        } else {
            const char* e = getenv("CIMBA_SPILL_SLABS");
            uint64_t want = e ? (uint64_t)atoll(e) : 4096;
            if (want > ntrials) want = ntrials;
            if (want == 0) want = 1;
            cap = (int32_t)want;
            HIP_TRY(arena.alloc(want));
            HIP_TRY(cursor.alloc(1));
            return cursor.zero();
        }
    }
};

// Device half of a log sink request (include/cimba/devlog.hpp).  The
// caller's LogSink carries HOST buffers sized for the clipped window
// (cmb::log_clip_window); this allocates the device arena + counters,
// hands the kernel a device-pointer sink and copies both back after the
// launch.  The DevBuf members free on every exit path; a
// sink-less launch (or a model without Cfg::DEVICE_LOG) allocates nothing.
template <class Model>
struct DevLog {
    cmb::LogSink sink = {nullptr, nullptr, 0, 0, 0, 0};  // device pointers
    const cmb::LogSink* req = nullptr;
    DevBuf<cmb::LogRec> recs;
    DevBuf<uint32_t> emitted;

    // validate + clip; no device call.  0 or a cmb::LOG_ERR_* code
    int prepare(const cmb::LogSink* r, uint64_t trial_base, uint64_t ntrials) {
        if constexpr (!Engine<Model>::DEVICE_LOG) {
            (void)r; (void)trial_base; (void)ntrials;
            return 0;
        } else {
            const int rc = cmb::log_sink_check(r, trial_base, ntrials);
            if (rc) return rc;
            if (!r || !r->recs || !r->emitted) return 0;
            uint64_t f, c;
            cmb::log_clip_window(r->first, r->count, trial_base, ntrials, &f,
                                 &c);
            if (c == 0) return 0;
            req = r;
            sink.first = f;
            sink.count = c;
            sink.cap = r->cap;
            sink.mask = r->mask;
            return 0;
        }
    }
    int alloc() {
        if (!req) return 0;
        HIP_TRY(recs.alloc(sink.count * sink.cap));
        HIP_TRY(emitted.alloc(sink.count));
        sink.recs = recs.get();
        sink.emitted = emitted.get();
        return emitted.zero();
    }
    int fetch() {
        if (!req) return 0;
        HIP_TRY(recs.download(req->recs, sink.count * sink.cap));
        return emitted.download(req->emitted, sink.count);
    }
};

// Device half of a tally request (include/cimba/tally.hpp).  The caller's
// TallyRequest carries HOST buffers sized for the clipped window
// (cmb::tally_clip_window); this allocates and zeroes the device arena,
// hands the kernel a device-pointer sink, pools the bins on the device
// after the launch (tally_kernel.hip) and copies back the pooled
// histogram and the 64-byte headers — the per-trial bins only when the
// caller gave a buffer for them.  A launch without a request (or a model
// without Cfg::DEVICE_TALLY) allocates nothing.
template <class Model>
struct DevTally {
    static constexpr int K = Engine<Model>::TALLY_K;
    cmb::TallySink sink = {nullptr, 0, 0};  // device pointer
    cmb::TallyRequest* req = nullptr;
    DevBuf<cmb::TallyRec> recs;
    DevBuf<uint64_t> pooled;

    // validate + clip; no device call.  0 or a cmb::TALLY_ERR_* code
    int prepare(cmb::TallyRequest* r, uint64_t trial_base, uint64_t ntrials) {
        if constexpr (K == 0) {
            (void)r; (void)trial_base; (void)ntrials;
            return 0;
        } else {
            if (!r) return 0;
            const int rc =
                cmb::tally_sink_check(&r->window, K, trial_base, ntrials);
            if (rc) return rc;
            if (!r->headers || !r->pooled) return 0;
            uint64_t f, c;
            cmb::tally_clip_window(r->window.first, r->window.count,
                                   trial_base, ntrials, &f, &c);
            if (c == 0) return 0;
            req = r;
            sink.first = f;
            sink.count = c;
            return 0;
        }
    }
    int alloc() {
        if (!req) return 0;
        HIP_TRY(recs.alloc(sink.count * K));
        HIP_TRY(pooled.alloc((size_t)K * cmb::TALLY_NBINS));
        sink.recs = recs.get();
        return recs.zero();  // the bins, once per launch
    }
    // after the trial kernel, on its stream
    int reduce() {
        if constexpr (K == 0) {
            return 0;
        } else {
            if (!req) return 0;
            cmb_hip::EventTimer timer;
            HIP_TRY(timer.start());
            HIP_TRY(cimba_tally_reduce_gpu(
                recs.get()->bins, sink.count, (uint32_t)K,
                sizeof(cmb::TallyRec) / sizeof(uint32_t), pooled.get()));
            return timer.stop(&req->reduce_ms);
        }
    }
    int fetch() {
        if (!req) return 0;
        const size_t rows = sink.count * K;
        HIP_TRY(pooled.download(req->pooled, (size_t)K * cmb::TALLY_NBINS));
        HIP_TRY(hipMemcpy2D(req->headers, sizeof(cmb::TallyHeader), recs.get(),
                            sizeof(cmb::TallyRec), sizeof(cmb::TallyHeader),
                            rows, hipMemcpyDeviceToHost));
        if (!req->trial_bins) return 0;
        constexpr size_t ROW = sizeof(uint32_t) * cmb::TALLY_NBINS;
        return (int)hipMemcpy2D(req->trial_bins, ROW, recs.get()->bins,
                                sizeof(cmb::TallyRec), ROW, rows,
                                hipMemcpyDeviceToHost);
    }
};

// what every launcher takes: one batch of trials of one model.  log_sink
// (nullable) is the caller's HOST sink, see DevLog
template <class Model>
struct TrialBatch {
    typename Model::Params P;
    uint64_t ntrials, seed, trial_base;
    double until;
    uint64_t max_events;
    double* elapsed_ms;
    typename Model::Result* host_out;
    const cmb::LogSink* log_sink = nullptr;
    cmb::TallyRequest* tally_sink = nullptr;  // nullable, see DevTally
};

// a batch that runs every trial to completion (no time or event limit)
template <class Model>
TrialBatch<Model> unbounded_batch(const typename Model::Params& P,
                                  uint64_t ntrials, uint64_t seed,
                                  uint64_t trial_base, double* elapsed_ms,
                                  void* results_out,
                                  const cmb::LogSink* log_sink = nullptr,
                                  cmb::TallyRequest* tally_sink = nullptr) {
    return {P, ntrials, seed, trial_base, 1.0e308,
            UINT64_C(0xFFFFFFFFFFFFFFFF), elapsed_ms,
            (typename Model::Result*)results_out, log_sink, tally_sink};
}

// The one host-side launcher: validate the log and tally requests (no
// device call before that), allocate the result buffer, whatever `extra`
// allocates (returns 0 or an error code), the log and tally arenas and the
// spill pool, time the launch alone, pool the tally histograms on the same
// stream, copy the per-trial results back and then the log and the
// tallies.  `launch(d_out, pool, d_sink, d_tsink)` issues the
// hipLaunchKernelGGL.  Every
// device resource is owned by an object on this frame, so each early
// return releases them all.
template <class Model, class Launch, class Extra>
int launch_trials(const TrialBatch<Model>& b, Launch&& launch, Extra&& extra) {
    DevLog<Model> dlog;
    if (const int lrc = dlog.prepare(b.log_sink, b.trial_base, b.ntrials))
        return lrc;
    DevTally<Model> dtally;
    if (const int trc = dtally.prepare(b.tally_sink, b.trial_base, b.ntrials))
        return trc;
    DevBuf<typename Model::Result> d_out;
    HIP_TRY(d_out.alloc(b.ntrials));
    HIP_TRY(extra());
    DevSpillPool<Model> pool;
    HIP_TRY(dlog.alloc());
    HIP_TRY(dtally.alloc());
    HIP_TRY(pool.alloc(b.ntrials));
    cmb_hip::EventTimer timer;
    HIP_TRY(timer.start());
    launch(d_out.get(), pool, dlog.sink, dtally.sink);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.stop(b.elapsed_ms));
    HIP_TRY(dtally.reduce());
    HIP_TRY(d_out.download(b.host_out, b.ntrials));
    HIP_TRY(dlog.fetch());
    return dtally.fetch();
}

template <class Model, class Launch>
int launch_trials(const TrialBatch<Model>& b, Launch&& launch) {
    return launch_trials(b, launch, [] { return 0; });
}

// trial-per-wavefront launcher; `blocks` (0 = no cap) bounds the grid so a
// small launch can exercise the stride loop, like the lane launchers
template <class Model, int WPB, int MINW = 1>
int run_trials_gpu(const TrialBatch<Model>& b, uint32_t blocks = 0) {
    const uint32_t want_blocks = (uint32_t)((b.ntrials + WPB - 1) / WPB);
    const uint32_t max_blocks = (blocks && blocks < 16384u) ? blocks : 16384u;
    const uint32_t grid = want_blocks < max_blocks ? want_blocks : max_blocks;
    return launch_trials(b, [&](auto* d_out, const auto& pool,
                                const auto& d_sink, const auto& d_tsink) {
        hipLaunchKernelGGL((trial_kernel<Model, WPB, MINW>), dim3(grid),
                           dim3(WPB * 64), 0, 0, b.P, b.seed, b.trial_base,
                           (uint32_t)b.ntrials, b.until, b.max_events, d_out,
                           pool.arena.get(), pool.cursor.get(), pool.cap,
                           d_sink, d_tsink);
    });
}

// lane-parallel variant: one trial per LANE (64 per wave), per-lane
// Storage in HBM (L2/L3-cached — an MM1 store is ~5 KB, so a full
// launch's working set sits in the 256 MiB L3).  The engine context is
// per-lane registers either way; the SIMT cost is divergence across the
// (event-kind, resume-pc) dispatch, the win is 64 trials per instruction
// stream.  Measured A/B against the wave-per-trial kernel in profiles/.
template <class Model, int MINW = 1>
__global__ __launch_bounds__(256, MINW) __attribute__((flatten)) void lane_trial_kernel(
    typename Model::Params P, uint64_t master_seed, uint64_t trial_base,
    uint32_t ntrials, double until, uint64_t max_events,
    typename Model::Result* __restrict__ out,
    typename Engine<Model>::Storage* __restrict__ stores,
    typename Engine<Model>::Spill* __restrict__ sp_arena,
    int32_t* __restrict__ sp_cur, int32_t sp_cap, cmb::LogSink lsink,
    cmb::TallySink tsink) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    Engine<Model> E(stores[gid]);
    E.set_spill_pool(sp_arena, sp_cur, sp_cap);
    if constexpr (Engine<Model>::DEVICE_LOG) E.log_attach(lsink);
    if constexpr (Engine<Model>::TALLY_K > 0) E.tally_attach(tsink);
    for (uint32_t trial = gid; trial < ntrials; trial += stride) {
        E.init(&P, cmb::trial_seed(master_seed, trial_base + trial),
               (uint32_t)(trial_base + trial));
        Model::setup(E);
        E.run(until, max_events);
        Model::finish(E, out[trial]);
        E.log_finish();
    }
}

// scratch variant: the per-trial Storage is a kernel LOCAL, so it lives
// in private (scratch) memory — which the hardware interleaves per lane.
// Same-field accesses across the 64 lanes of a wave therefore COALESCE
// into wide transactions: the AoS->SoA transposition for free.
template <class Model, int MINW = 1>
__global__ __launch_bounds__(256, MINW) void lane_scratch_kernel(
    typename Model::Params P, uint64_t master_seed, uint64_t trial_base,
    uint32_t ntrials, double until, uint64_t max_events,
    typename Model::Result* __restrict__ out,
    typename Engine<Model>::Spill* __restrict__ sp_arena,
    int32_t* __restrict__ sp_cur, int32_t sp_cap, cmb::LogSink lsink,
    cmb::TallySink tsink) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    typename Engine<Model>::Storage st;  // per-lane scratch (HW-swizzled)
    Engine<Model> E(st);
    E.set_spill_pool(sp_arena, sp_cur, sp_cap);
    if constexpr (Engine<Model>::DEVICE_LOG) E.log_attach(lsink);
    if constexpr (Engine<Model>::TALLY_K > 0) E.tally_attach(tsink);
    for (uint32_t trial = gid; trial < ntrials; trial += stride) {
        E.init(&P, cmb::trial_seed(master_seed, trial_base + trial),
               (uint32_t)(trial_base + trial));
        Model::setup(E);
        E.run(until, max_events);
        Model::finish(E, out[trial]);
        E.log_finish();
    }
}

// ---------------------------------------------------------------------------
// Path-converged lane kernel: the divergence fix for the lane regime.
//
// The plain lane kernels run 64 independent trials per wave; at each
// dispatch step the 64 lanes sit at random (event-kind, process-func,
// resume-pc) points, so the wave serializes over every distinct path
// present and VALUUtilization measured 20-28%
// (profiles/r01_lane_divergence.md).  Here each lane still owns ONE trial
// in scratch, but dispatch is gated by a wave vote: every iteration the
// lanes peek their next dispatch path (Engine::peek_path), poll up to 4
// distinct candidates (__shfl from the first lane of each unseen group),
// and ONLY the lanes on the most-popular path dispatch.  Idle minority
// lanes cost less than serializing all paths.  Measurement history and
// the shipped-default matrix: profiles/r02_conv_divergence.md (first
// A/B: 3.93 vs 3.33 G ev/s, profiles/logs/r2_ab1.log; final with the
// heap-top cache: 4.69 G and conv wins for every lane model).
//
// Trial refill is wave-synchronous via the stride loop — all lanes of a
// wave start their next trial together, so the low-utilization tail is
// one trial-length VARIANCE, not a full trial.  (The earlier design —
// K parked trials per lane with per-lane atomic refill — measured 21%
// WORSE at any batch that needs refill: staggered per-lane trial ages
// leave each wave grinding out stragglers at ~50% liveness after the
// pool empties.  profiles/logs (r2 sweep data); kept here as the measured
// justification for the no-refill shape.)
//
// conv_lds_kernel is the same loop with the engine's HOT half in LDS
// (profiles/r04_lds_hot_tier.md).  In conv_lane_kernel every distinct
// dword a wave touches is its own 256-B scratch row, a dispatch walks
// about 120 of them through load-feeds-address chains, and the rows of
// all resident waves together are far larger than L1 and L2.  Models that
// declare Cfg::LDS_HOT keep Engine::Hot — process records, frames,
// guards, toolkit headers, the first HOT_EV heap entries — in a per-lane
// LDS slice instead; Engine::Cold (queue rings, the heap's tail) stays a
// kernel local in scratch.  One wave per workgroup: the loop needs no
// workgroup cooperation, and wave-sized LDS grains lose no residency to
// rounding.  Lane l owns bytes [l*HS, l*HS + sizeof(Hot)) where the
// stride HS is sizeof(Hot) rounded up to 8 x odd: a 64-bit access at one
// field offset then hits distinct banks across each 32-lane service
// group (conflict-free).  Narrower accesses are not: the stride is an odd
// number of 8-byte units, i.e. 2 x odd dwords, so a 32-bit (or 16-bit)
// access puts lanes l and l+16 of one service group on the same bank, a
// 2-way conflict that costs one extra LDS cycle.  Measured on M/M/1:
// SQ_LDS_BANK_CONFLICT is 28 % of SQ_LDS_IDX_ACTIVE, with LDS at about a
// fifth of its cycles (profiles/r04_lds_hot_tier.md).
//
// The kernel is latency-bound on short dependent chains and only resident
// waves hide them; LDS bytes per lane, not registers, decide how many fit
// (LdsHotPlan::WAVES_PER_CU).  So Hot carries nothing a dispatch does not
// touch: the time-weighted statistics records of the toolkit objects and
// the spill cursors of a spill-less queue live elsewhere (engine.hpp).
// M/M/1: 312 B per lane, 19968 B per wave, 8 waves per CU = 2 on every
// SIMD, 12.8 G ev/s against 9.8 G at 392 B / 6 waves; M/G/1: 376 B, 6
// waves.  The model TUs pin these with static_asserts
// (profiles/r09_hot_shrink.md).
// ---------------------------------------------------------------------------

// the vote-gated trial loop, shared by conv_lane_kernel and
// conv_lds_kernel; lane `gid` of `stride` runs trials gid, gid+stride, ...
template <class Model, class Eng>
__device__ __forceinline__ void conv_trial_loop(
    Eng& E, const typename Model::Params& P, uint64_t master_seed,
    uint64_t trial_base, uint32_t ntrials, double until, uint64_t max_events,
    typename Model::Result* __restrict__ out, uint32_t gid, uint32_t stride) {
    constexpr uint32_t DONE = Eng::PATH_DONE;
    for (uint32_t trial = gid;; trial += stride) {
        const bool have = trial < ntrials;
        if (__ballot(have) == 0) break;
        if (have) {
            E.init(&P, cmb::trial_seed(master_seed, trial_base + trial),
                   (uint32_t)(trial_base + trial));
            Model::setup(E);
        }
        uint32_t mypath = have ? E.peek_path(until, max_events) : DONE;
        for (;;) {
            const uint64_t live = __ballot(mypath != DONE);
            if (live == 0) break;
            // poll up to 4 distinct paths; serve the most popular
            uint64_t rem = live;
            uint32_t best = 0;
            int bestv = -1;
            for (int it = 0; it < 4 && rem; ++it) {
                const int src = __ffsll((unsigned long long)rem) - 1;
                const uint32_t cand = __shfl(mypath, src);
                const uint64_t m = __ballot(mypath == cand);
                const int v = __popcll(m);
                if (v > bestv) {
                    bestv = v;
                    best = cand;
                }
                rem &= ~m;
            }
            if (mypath == best) {
                E.dispatch_one();
                if (E.ev_dispatched >= max_events)
                    E.fail(cmb::ST_EVENT_LIMIT);
                mypath = E.peek_path(until, max_events);
            }
        }
        if (have) {
            if (!E.evq.empty() && E.evq.top().t > until) E.now = until;
            Model::finish(E, out[trial]);
            E.log_finish();
        }
    }
}

template <class Model, int MINW = 1>
__global__ __launch_bounds__(256, MINW) void conv_lane_kernel(
    typename Model::Params P, uint64_t master_seed, uint64_t trial_base,
    uint32_t ntrials, double until, uint64_t max_events,
    typename Model::Result* __restrict__ out,
    typename Engine<Model>::Spill* __restrict__ sp_arena,
    int32_t* __restrict__ sp_cur, int32_t sp_cap, cmb::LogSink lsink,
    cmb::TallySink tsink) {
    using Eng = Engine<Model>;
    typename Eng::Storage st;  // per-lane scratch (HW-swizzled)
    Eng E(st);
    E.set_spill_pool(sp_arena, sp_cur, sp_cap);
    if constexpr (Engine<Model>::DEVICE_LOG) E.log_attach(lsink);
    if constexpr (Engine<Model>::TALLY_K > 0) E.tally_attach(tsink);
    conv_trial_loop<Model>(E, P, master_seed, trial_base, ntrials, until,
                           max_events, out,
                           blockIdx.x * blockDim.x + threadIdx.x,
                           gridDim.x * blockDim.x);
}

// per-lane LDS layout of conv_lds_kernel for one model
template <class Model>
struct LdsHotPlan {
    using Hot = typename Engine<Model>::Hot;
    // lane stride: sizeof(Hot) rounded up to 8 x odd bytes
    static constexpr uint32_t HS = 8u * ((((uint32_t)sizeof(Hot) + 7u) / 8u) | 1u);
    static constexpr uint32_t WAVE_BYTES = 64u * HS;
    static constexpr uint32_t LDS_PER_CU = 160u * 1024u;
    // planned residency: at least one wave on each of the CU's 4 SIMDs
    static constexpr uint32_t PLAN_WAVES = 4;
    static constexpr uint32_t WAVES_PER_CU = LDS_PER_CU / WAVE_BYTES;
    static_assert(Engine<Model>::LDS_HOT, "model did not opt into the LDS kernel");
    static_assert(HS >= sizeof(Hot) && HS % 8 == 0 && (HS / 8) % 2 == 1,
                  "lane stride must be 8 x odd bytes");
    static_assert(alignof(Hot) <= 8, "lane slices are 8-byte aligned");
    static_assert(WAVE_BYTES * PLAN_WAVES <= LDS_PER_CU, "LDS plan");
};

template <class Model, int MINW = 1>
__global__ __launch_bounds__(64, MINW) void conv_lds_kernel(
    typename Model::Params P, uint64_t master_seed, uint64_t trial_base,
    uint32_t ntrials, double until, uint64_t max_events,
    typename Model::Result* __restrict__ out,
    typename Engine<Model>::Spill* __restrict__ sp_arena,
    int32_t* __restrict__ sp_cur, int32_t sp_cap, cmb::LogSink lsink,
    cmb::TallySink tsink) {
    using Eng = Engine<Model, cmb::LdsTier>;  // hot heap tier: ds_* by type
    using Plan = LdsHotPlan<Model>;
    __shared__ uint64_t lds[Plan::WAVE_BYTES / 8];
    typename Eng::Hot& hot = *reinterpret_cast<typename Eng::Hot*>(
        reinterpret_cast<unsigned char*>(lds) + threadIdx.x * Plan::HS);
    typename Eng::Cold cold;  // per-lane scratch (HW-swizzled)
    Eng E(hot, cold);
    E.set_spill_pool(sp_arena, sp_cur, sp_cap);
    if constexpr (Engine<Model>::DEVICE_LOG) E.log_attach(lsink);
    if constexpr (Engine<Model>::TALLY_K > 0) E.tally_attach(tsink);
    conv_trial_loop<Model>(E, P, master_seed, trial_base, ntrials, until,
                           max_events, out, blockIdx.x * 64u + threadIdx.x,
                           gridDim.x * 64u);
}

// LDS = false: conv_lane_kernel, 256-lane workgroups; LDS = true:
// conv_lds_kernel, 64-lane workgroups.  `blocks` caps the grid in
// workgroups of that kernel (0 = one lane per trial, capped at 4M lanes)
template <class Model, int MINW, bool LDS = false>
int run_trials_gpu_conv(const TrialBatch<Model>& b, uint32_t blocks) {
    constexpr uint32_t WG = LDS ? 64u : 256u;
    if (blocks == 0) blocks = 16384u * (256u / WG);
    const uint32_t want = (uint32_t)((b.ntrials + WG - 1) / WG);
    const uint32_t grid = want < blocks ? want : blocks;
    if (getenv("CIMBA_CONV_DEBUG"))
        fprintf(stderr, "[conv%s] minw=%d grid=%u lanes=%u ntrials=%llu\n",
                LDS ? "-lds" : "", MINW, grid, grid * WG,
                (unsigned long long)b.ntrials);
    return launch_trials(b, [&](auto* d_out, const auto& pool,
                                const auto& d_sink, const auto& d_tsink) {
        if constexpr (LDS)
            hipLaunchKernelGGL((conv_lds_kernel<Model, MINW>), dim3(grid),
                               dim3(WG), 0, 0, b.P, b.seed, b.trial_base,
                               (uint32_t)b.ntrials, b.until, b.max_events,
                               d_out, pool.arena.get(), pool.cursor.get(),
                               pool.cap, d_sink, d_tsink);
        else
            hipLaunchKernelGGL((conv_lane_kernel<Model, MINW>), dim3(grid),
                               dim3(WG), 0, 0, b.P, b.seed, b.trial_base,
                               (uint32_t)b.ntrials, b.until, b.max_events,
                               d_out, pool.arena.get(), pool.cursor.get(),
                               pool.cap, d_sink, d_tsink);
    });
}

template <class Model, int MINW>
int run_trials_gpu_lane_scratch(const TrialBatch<Model>& b, uint32_t blocks) {
    const uint32_t want = (uint32_t)((b.ntrials + 255) / 256);
    const uint32_t grid = want < blocks ? want : blocks;
    return launch_trials(b, [&](auto* d_out, const auto& pool,
                                const auto& d_sink, const auto& d_tsink) {
        hipLaunchKernelGGL((lane_scratch_kernel<Model, MINW>), dim3(grid),
                           dim3(256), 0, 0, b.P, b.seed, b.trial_base,
                           (uint32_t)b.ntrials, b.until, b.max_events, d_out,
                           pool.arena.get(), pool.cursor.get(), pool.cap,
                           d_sink, d_tsink);
    });
}

template <class Model, int MINW>
int run_trials_gpu_lane(const TrialBatch<Model>& b, uint32_t blocks) {
    const uint32_t want = (uint32_t)((b.ntrials + 255) / 256);
    const uint32_t grid = want < blocks ? want : blocks;
    DevBuf<typename Engine<Model>::Storage> stores;  // one per lane
    return launch_trials(
        b,
        [&](auto* d_out, const auto& pool, const auto& d_sink,
            const auto& d_tsink) {
            hipLaunchKernelGGL((lane_trial_kernel<Model, MINW>), dim3(grid),
                               dim3(256), 0, 0, b.P, b.seed, b.trial_base,
                               (uint32_t)b.ntrials, b.until, b.max_events,
                               d_out, stores.get(), pool.arena.get(),
                               pool.cursor.get(), pool.cap, d_sink,
                               d_tsink);
        },
        [&] { return stores.alloc((size_t)grid * 256); });
}

// scratch-kernel front end: MINW occupancy knob (CIMBA_SCRATCH_MINW)
template <class Model>
int run_scratch_auto(const TrialBatch<Model>& b, uint32_t blocks) {
    if (env_int("CIMBA_SCRATCH_MINW").value_or(1) >= 4)
        return run_trials_gpu_lane_scratch<Model, 4>(b, blocks);
    return run_trials_gpu_lane_scratch<Model, 1>(b, blocks);
}

// converged-kernel front end: grid (CIMBA_CONV_BLOCKS, 0 = one lane per
// trial capped at 16384 blocks) and register budget (CIMBA_CONV_MINW)
template <class Model>
int run_conv_auto(const TrialBatch<Model>& b) {
    const uint32_t blocks = (uint32_t)env_int("CIMBA_CONV_BLOCKS").value_or(0);
    // MINW (waves/SIMD floor) trades registers for occupancy: the engine
    // context spills into hardware-swizzled scratch (L1-friendly) and the
    // extra resident waves hide the dispatch chain's memory latency — the
    // dominant term at 131 VGPRs / 3 waves (r2 sweeps).
    // measured (profiles/r02_conv_divergence.md): MINW=4 is the sweet
    // spot, 6/8 overspill everywhere — only 1 and 4 stay instantiated
    if (env_int("CIMBA_CONV_MINW").value_or(4) >= 4)
        return run_trials_gpu_conv<Model, 4>(b, blocks);
    return run_trials_gpu_conv<Model, 1>(b, blocks);
}

// LDS-kernel front end (lane mode 4).  CIMBA_CONV_BLOCKS counts 64-lane
// workgroups here.  LDS, not registers, bounds residency (LdsHotPlan), so
// MINW only picks the register budget: 1 or 2 waves/SIMD both leave the
// full 256 VGPRs (CIMBA_LDS_MINW, default 1; A/B in
// profiles/r04_lds_hot_tier.md, and again at 8 waves per CU, where the
// kernel really runs 2 waves/SIMD, in profiles/r09_hot_shrink.md: MINW 2
// is 1.5 % slower).  A grid of exactly the resident waves
// (CIMBA_CONV_BLOCKS=2048) measured the same as the default grid
template <class Model>
int run_lds_auto(const TrialBatch<Model>& b) {
    const uint32_t blocks = (uint32_t)env_int("CIMBA_CONV_BLOCKS").value_or(0);
    // 2 waves/SIMD only where LDS has room for a fifth wave on the CU
    if constexpr (LdsHotPlan<Model>::WAVES_PER_CU > 4) {
        if (env_int("CIMBA_LDS_MINW").value_or(1) >= 2)
            return run_trials_gpu_conv<Model, 2, true>(b, blocks);
    }
    return run_trials_gpu_conv<Model, 1, true>(b, blocks);
}

}  // namespace cmb_dk
