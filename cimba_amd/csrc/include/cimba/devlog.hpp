// Device log stream: in-trial log records from GPU (and host) trials.
//
// The reference logger prints "[trial] [seed] time who tag: msg" from
// inside a running trial (reference src/cmb_logger.c:154-156).  A GPU
// trial cannot print, so a model that opts in (Cfg::DEVICE_LOG = true)
// gets a bounded per-trial RING of fixed-size records in HBM; the host
// formats them through the logger after the launch (log_format /
// log_replay below).  The ring keeps the LAST `cap` records of a trial —
// the events just before an abort are the ones worth keeping.
//
// Ownership: trial g inside the window [first, first + count) owns records
// [(g-first)*cap, (g-first+1)*cap) and emitted[g-first].  The slot is
// indexed by GLOBAL trial index, never by lane/wave/block, and exactly one
// lane runs a trial, so emission needs no atomics.
//
// The same code runs on the host (run_host with a caller-provided arena)
// and produces byte-identical records.
#pragma once

#include "config.hpp"
#include "logger.hpp"

#include <type_traits>

namespace cmb {

enum LogValueType : uint8_t { LOGV_U64 = 0, LOGV_I64 = 1, LOGV_F64 = 2 };

struct alignas(32) LogRec {
    double t;        // E.now at emission
    uint64_t value;  // payload bits (see vtype)
    uint32_t flags;  // one LogFlag bit
    uint32_t seq;    // per-trial emission ordinal, from 0
    uint16_t code;   // model-defined
    int16_t proc;    // emitting process index, -1 = engine context
    uint8_t vtype;   // LogValueType
    uint8_t pad_[3];  // zero, so records compare bytewise
};
static_assert(sizeof(LogRec) == 32, "LogRec is two 16-byte stores");
static_assert(std::is_trivially_copyable<LogRec>::value, "LogRec is POD");
// log_emit packs the record as eight little-endian 32-bit words
static_assert(offsetof(LogRec, value) == 8 && offsetof(LogRec, flags) == 16 &&
                  offsetof(LogRec, seq) == 20 && offsetof(LogRec, code) == 24 &&
                  offsetof(LogRec, proc) == 26 && offsetof(LogRec, vtype) == 28,
              "LogRec word layout");

// launch descriptor, passed by value to kernels
struct LogSink {
    LogRec* recs;       // arena base
    uint32_t* emitted;  // one counter per windowed trial
    uint64_t first;     // window of GLOBAL trial indices: [first, first+count)
    uint64_t count;
    uint32_t cap;   // ring capacity per trial, in records
    uint32_t mask;  // LogFlag mask
};
static_assert(std::is_trivially_copyable<LogSink>::value, "LogSink is POD");

// launcher error codes (negative: hipError_t values are positive)
constexpr int LOG_ERR_ARENA_TOO_BIG = -101;  // count*cap*32 B > 1 GiB
constexpr int LOG_ERR_BAD_SINK = -102;       // cap == 0, or index > 32 bits

constexpr uint64_t LOG_ARENA_MAX_BYTES = UINT64_C(1) << 30;

// clip a requested window to the launch's trials
// [trial_base, trial_base + ntrials); an empty intersection gives count 0
inline void log_clip_window(uint64_t first, uint64_t count,
                            uint64_t trial_base, uint64_t ntrials,
                            uint64_t* first_out, uint64_t* count_out) {
    const uint64_t lo = first > trial_base ? first : trial_base;
    const uint64_t req_end = count > ~first ? ~UINT64_C(0) : first + count;
    const uint64_t run_end = trial_base + ntrials;
    const uint64_t hi = req_end < run_end ? req_end : run_end;
    *first_out = lo;
    *count_out = hi > lo ? hi - lo : 0;
}

// Validate a sink request BEFORE any allocation or device call.  The
// size guard applies to the window as requested, so a refused launch
// touches nothing.  Returns 0 or a LOG_ERR_* code.
inline int log_sink_check(const LogSink* req, uint64_t trial_base,
                          uint64_t ntrials) {
    if (!req || req->count == 0) return 0;
    if (req->cap == 0) return LOG_ERR_BAD_SINK;
    if (req->count > LOG_ARENA_MAX_BYTES / sizeof(LogRec) / req->cap)
        return LOG_ERR_ARENA_TOO_BIG;
    // Engine::init carries the global trial index in 32 bits
    if (trial_base + ntrials > (UINT64_C(1) << 32)) return LOG_ERR_BAD_SINK;
    return 0;
}

// 16-byte store unit (may_alias: the arena is read back as LogRec)
typedef uint32_t log_v4u_
    __attribute__((vector_size(16), may_alias, aligned(16)));

// optional Cfg::DEVICE_LOG (same detection idiom as SPILL_EV)
template <class C, class = void>
struct DevLogOf {
    static constexpr bool v = false;
};
template <class C>
struct DevLogOf<C, std::void_t<decltype(C::DEVICE_LOG)>> {
    static constexpr bool v = C::DEVICE_LOG;
};

// Engine base: EMPTY for models that do not opt in, so Engine<Model> keeps
// its layout and code; the ring cursor and sink exist only when ON.
template <bool ON>
struct LogState {};
static_assert(std::is_empty<LogState<false>>::value,
              "no log state in models that do not opt in");

template <>
struct LogState<true> {
    LogSink log_sink = {nullptr, nullptr, 0, 0, 0, 0};
    LogRec* log_ring = nullptr;  // this trial's ring; null = outside window
    uint32_t log_slot = 0;
    uint32_t log_seq = 0;

    CMB_FORCEINLINE void log_attach(const LogSink& s) {
        log_sink = s;
        log_ring = nullptr;
        log_seq = 0;
    }

    // bind the ring of global trial `g` (Engine::init), or nothing when g
    // is outside the window; the cursor restarts for every trial
    CMB_FORCEINLINE void log_bind(uint64_t g) {
        log_seq = 0;
        log_ring = nullptr;
        const uint64_t slot = g - log_sink.first;  // wraps huge when g < first
        if (log_sink.recs && log_sink.cap && slot < log_sink.count) {
            log_slot = (uint32_t)slot;
            log_ring = log_sink.recs + slot * log_sink.cap;
        }
    }

    CMB_FORCEINLINE void log_emit(double t, uint32_t flags, uint16_t code,
                                  int16_t proc, uint8_t vtype,
                                  uint64_t bits) {
        if (!log_ring || !(flags & log_sink.mask)) return;
        const uint64_t tb = double_as_u64(t);
        const log_v4u_ lo = {(uint32_t)tb, (uint32_t)(tb >> 32),
                             (uint32_t)bits, (uint32_t)(bits >> 32)};
        const log_v4u_ hi = {flags, log_seq,
                             (uint32_t)code | ((uint32_t)(uint16_t)proc << 16),
                             (uint32_t)vtype};
        log_v4u_* dst =
            reinterpret_cast<log_v4u_*>(log_ring + (log_seq % log_sink.cap));
        dst[0] = lo;
        dst[1] = hi;
        ++log_seq;
    }

    // end of trial: publish the emission count, once
    CMB_FORCEINLINE void log_flush() {
        if (log_ring) log_sink.emitted[log_slot] = log_seq;
    }
};

// ---------------------------------------------------------------------------
// Host side: one formatter, one replay walk
// ---------------------------------------------------------------------------

inline const char* log_tag(uint32_t flags) {
    if (flags & LOG_FATAL) return "fatal";
    if (flags & LOG_ERROR) return "error";
    if (flags & LOG_WARNING) return "warning";
    if (flags & LOG_INFO) return "info";
    return "user";
}

inline int log_format_who(char* buf, size_t n, const LogRec& r) {
    if (r.proc < 0) return snprintf(buf, n, "engine");
    return snprintf(buf, n, "proc%d", (int)r.proc);
}

inline int log_format_value(char* buf, size_t n, const LogRec& r) {
    switch (r.vtype) {
        case LOGV_I64:
            return snprintf(buf, n, "%lld", (long long)(int64_t)r.value);
        case LOGV_F64:
            return snprintf(buf, n, "%.17g", u64_as_double(r.value));
        default:
            return snprintf(buf, n, "%llu", (unsigned long long)r.value);
    }
}

// exactly the logger line (logger_vlog): "[trial] [seed] time who tag: msg"
// with msg = "<name> value=<value>"; returns snprintf's count
inline int log_format(char* buf, size_t n, const LogRec& r, uint32_t trial,
                      uint64_t seed, const char* name) {
    char who[16], val[40];
    log_format_who(who, sizeof who, r);
    log_format_value(val, sizeof val, r);
    return snprintf(buf, n, "[%u] [%016llx] %.6f %s %s: %s value=%s", trial,
                    (unsigned long long)seed, r.t, who, log_tag(r.flags),
                    name, val);
}

namespace detail {
inline void log_replay_line(uint32_t flag, const char* tag, const char* fmt,
                            ...) {
    va_list ap;
    va_start(ap, fmt);
    logger_vlog(flag, tag, fmt, ap);
    va_end(ap);
}
}  // namespace detail

// Walk a copied-back arena in (trial, seq) order and print every surviving
// record through the host logger: logger_vlog's gate applies the logger's
// CURRENT mask and stream.  seed_of(global trial) -> per-trial seed;
// name_of(record) -> record name (engine records carry a status code).
// Returns the number of records walked.
template <class SeedFn, class NameFn>
inline uint64_t log_replay(const LogRec* recs, const uint32_t* emitted,
                           uint64_t first, uint64_t count, uint32_t cap,
                           SeedFn seed_of, NameFn name_of) {
    uint64_t walked = 0;
    if (!cap) return 0;
    const LogCtx saved = logger_ctx();
    for (uint64_t s = 0; s < count; ++s) {
        const uint32_t n = emitted[s];
        const uint32_t kept = n < cap ? n : cap;
        for (uint32_t q = n - kept; q != n; ++q) {
            const LogRec& r = recs[s * cap + (q % cap)];
            char who[16], val[40];
            log_format_who(who, sizeof who, r);
            log_format_value(val, sizeof val, r);
            LogCtx& c = logger_ctx();
            c.trial = (uint32_t)(first + s);
            c.seed = seed_of(first + s);
            c.sim_time = r.t;
            c.who = who;
            detail::log_replay_line(r.flags, log_tag(r.flags), "%s value=%s",
                                    name_of(r), val);
            ++walked;
        }
    }
    logger_ctx() = saved;
    return walked;
}

}  // namespace cmb
