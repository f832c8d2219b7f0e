// Device tally stream: in-trial moments and quantile histograms from GPU
// (and host) trials.
//
// A trial hands back sums; a queueing study wants the tail.  A model that
// opts in (Cfg::DEVICE_TALLY = K, 1 <= K <= 8) gets K per-trial tallies in
// HBM: CMB_TALLY(id, x) feeds a DataSummary (four moments, min, max) and a
// fixed log-binned histogram, from which the host reads quantiles
// (cimba_amd/tally.py).  A device kernel (hip/tally_kernel.hip) pools the
// histograms across trials; the host merges the moment headers in trial
// order with DataSummary::merge.
//
// Ownership: trial g inside the window [first, first + count) owns records
// [(g-first)*K, (g-first+1)*K).  The slot is indexed by GLOBAL trial index,
// never by lane/wave/block, and exactly one lane runs a trial, so a tally
// needs no atomics.  A slot is never shared between trials.
//
// Moments and bins live in the slot and are updated by read-modify-write:
// the engine context carries only the sink and the bound slot pointer, so
// the lane kernels keep their register budget.
//
// The same code runs on the host (run_host with a caller-provided, zeroed
// arena) and produces byte-identical records.
#pragma once

#include "config.hpp"
#include "stats.hpp"

#include <type_traits>

namespace cmb {

// ---------------------------------------------------------------------------
// Bin geometry: 48 octaves [2^-24, 2^24) of 16 sub-bins each (the top four
// mantissa bits), so a bin is at most 1/16 wide relative to its lower edge.
//   bin 0    every x for which x >= 2^-24 is false: zero, negatives,
//            denormals
//   bin b    1 <= b <= 768: [tally_edge(b), tally_edge(b + 1))
//   bin 769  x >= 2^24, +inf included
// A pure integer function of the bits (no log, no floating-point
// arithmetic beyond the two comparisons): host and device agree by
// construction.  NaN is the caller's business — tally_add counts it in
// nan_cnt and puts it in no bin and no moment.
// ---------------------------------------------------------------------------
constexpr uint32_t TALLY_NBINS = 770;
constexpr int TALLY_MAX_K = 8;
constexpr uint32_t TALLY_BIN_BIAS = (1023u - 24u) << 4;

CMB_FORCEINLINE uint32_t tally_bin(double x) {
    if (!(x >= 0x1p-24)) return 0;
    if (x >= 0x1p24) return TALLY_NBINS - 1;
    return 1u + (uint32_t)(double_as_u64(x) >> 48) - TALLY_BIN_BIAS;
}

// lower edge of bin b (host-side use); bin 0 reports 0.0 although it also
// holds the negatives, and tally_edge(TALLY_NBINS) is +inf, the upper edge
// of the last bin
inline double tally_edge(uint32_t b) {
    if (b == 0) return 0.0;
    if (b >= TALLY_NBINS) return HUGE_VAL;
    return u64_as_double((uint64_t)(b - 1u + TALLY_BIN_BIAS) << 48);
}

// One tally of one trial.  Per-bin counts are 32 bits PER TRIAL: a trial
// that puts more than 2^32 - 1 observations into one bin wraps that bin
// (the pooled histogram is 64 bits).
struct TallyRec {
    DataSummary s;
    uint64_t nan_cnt;
    uint32_t bins[TALLY_NBINS];
};
// the 64 bytes in front of the bins: what a launcher copies back per tally
struct TallyHeader {
    DataSummary s;
    uint64_t nan_cnt;
};
static_assert(sizeof(DataSummary) == 56, "DataSummary is seven doubles");
static_assert(sizeof(TallyHeader) == 64, "header is one 64-byte line");
static_assert(sizeof(TallyRec) == 3144, "TallyRec layout");
static_assert(std::is_trivially_copyable<TallyRec>::value, "TallyRec is POD");
static_assert(offsetof(TallyRec, s) == 0 && offsetof(TallyRec, nan_cnt) == 56 &&
                  offsetof(TallyRec, bins) == 64 &&
                  offsetof(TallyHeader, nan_cnt) == 56,
              "TallyRec layout");
static_assert(sizeof(TallyRec) % sizeof(uint32_t) == 0,
              "the pooling kernel strides over records in 32-bit words");

// launch descriptor, passed by value to kernels
struct TallySink {
    TallyRec* recs;  // arena base
    uint64_t first;  // window of GLOBAL trial indices: [first, first+count)
    uint64_t count;
};
static_assert(std::is_trivially_copyable<TallySink>::value, "TallySink is POD");

// What a GPU launcher delivers for a window.  `window.recs` is unused (the
// arena stays on the device); the buffers are HOST memory sized for the
// clipped window (tally_clip_window) of a model with K tallies.
struct TallyRequest {
    TallySink window;
    TallyHeader* headers;  // [count * K]
    uint64_t* pooled;      // [K * TALLY_NBINS], summed over the window
    uint32_t* trial_bins;  // nullable: [count * K * TALLY_NBINS]
    double reduce_ms;      // out: time of the pooling kernel alone
};

// launcher error codes (negative, and apart from the LOG_ERR_* values)
constexpr int TALLY_ERR_ARENA_TOO_BIG = -111;  // count*K*3144 B > 1 GiB
constexpr int TALLY_ERR_BAD_SINK = -112;       // bad K, or index > 32 bits

constexpr uint64_t TALLY_ARENA_MAX_BYTES = UINT64_C(1) << 30;

// clip a requested window to the launch's trials
// [trial_base, trial_base + ntrials); an empty intersection gives count 0
inline void tally_clip_window(uint64_t first, uint64_t count,
                              uint64_t trial_base, uint64_t ntrials,
                              uint64_t* first_out, uint64_t* count_out) {
    const uint64_t lo = first > trial_base ? first : trial_base;
    const uint64_t req_end = count > ~first ? ~UINT64_C(0) : first + count;
    const uint64_t run_end = trial_base + ntrials;
    const uint64_t hi = req_end < run_end ? req_end : run_end;
    *first_out = lo;
    *count_out = hi > lo ? hi - lo : 0;
}

// Validate a window request for a model with K tallies BEFORE any
// allocation or device call.  The size guard applies to the window as
// requested, so a refused launch touches nothing.  Returns 0 or a
// TALLY_ERR_* code.
inline int tally_sink_check(const TallySink* req, int K, uint64_t trial_base,
                            uint64_t ntrials) {
    if (!req || req->count == 0) return 0;
    if (K < 1 || K > TALLY_MAX_K) return TALLY_ERR_BAD_SINK;
    if (req->count > TALLY_ARENA_MAX_BYTES / sizeof(TallyRec) / (uint64_t)K)
        return TALLY_ERR_ARENA_TOO_BIG;
    // Engine::init carries the global trial index in 32 bits
    if (trial_base + ntrials > (UINT64_C(1) << 32)) return TALLY_ERR_BAD_SINK;
    return 0;
}

// optional Cfg::DEVICE_TALLY (same detection idiom as DevLogOf)
template <class C, class = void>
struct TallyOf {
    static constexpr int K = 0;
};
template <class C>
struct TallyOf<C, std::void_t<decltype(C::DEVICE_TALLY)>> {
    static constexpr int K = C::DEVICE_TALLY;
    static_assert(K >= 1 && K <= TALLY_MAX_K,
                  "Cfg::DEVICE_TALLY is the number of tallies, 1..8");
};

// Engine base: EMPTY for models that do not opt in, so Engine<Model> keeps
// its layout and code; the sink and the slot pointer exist only for K > 0.
template <int K>
struct TallyState {
    TallySink tally_sink = {nullptr, 0, 0};
    TallyRec* tally_slot = nullptr;  // this trial's K records; null = outside

    CMB_FORCEINLINE void tally_attach(const TallySink& s) {
        tally_sink = s;
        tally_slot = nullptr;
    }

    // bind the records of global trial `g` (Engine::init), or nothing when
    // g is outside the window.  Resets the K headers; the bins were zeroed
    // once for the whole arena (launcher, or the host caller) and no other
    // trial ever touches this slot.
    CMB_FORCEINLINE void tally_bind(uint64_t g) {
        tally_slot = nullptr;
        const uint64_t slot = g - tally_sink.first;  // wraps huge when g < first
        if (tally_sink.recs && slot < tally_sink.count) {
            tally_slot = tally_sink.recs + slot * (uint64_t)K;
            for (int k = 0; k < K; ++k) {
                tally_slot[k].s.reset();
                tally_slot[k].nan_cnt = 0;
            }
        }
    }

    // one observation; never blocks, draws or schedules
    CMB_FORCEINLINE void tally_add(int id, double x) {
        if (!tally_slot) return;
        TallyRec& r = tally_slot[id];
        if (x != x) {
            r.nan_cnt += 1u;
            return;
        }
        r.s.add(x);
        r.bins[tally_bin(x)] += 1u;
    }
};

template <>
struct TallyState<0> {};
static_assert(std::is_empty<TallyState<0>>::value,
              "no tally state in models that do not opt in");

}  // namespace cmb
