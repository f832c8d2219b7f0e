// cimba_amd simulation engine: clock + future-event list + state-machine
// processes + process-interaction toolkit, in one POD aggregate that runs
// identically as host code (CPU executive, unit tests) and as HIP device
// code with the whole trial resident in LDS (one trial per wavefront).
//
// This is the MI355X-native redesign of the reference's L2-L4 layers
// (SURVEY.md §1):
//  - reference src/cmb_event.c (thread-local clock + hash-heap event queue,
//    dispatch loop cmb_event.c:370-410)            -> Engine::dispatch_one()
//  - reference src/cmi_coroutine.c + the x86-64 context-switch assembly
//    (port/x86-64/linux/cmi_coroutine_context.asm) -> protothread-style
//    resumable process functions (CMB_BEGIN/CMB_HOLD/.../CMB_END below):
//    every blocking call site is a numbered resumption point, the
//    "coroutine switch rewritten as a state-machine scheduler" of
//    BASELINE.json's north star.  There is no stack to switch - a process
//    is (pc, frame) and the scheduler is the event loop itself.
//  - reference src/cmb_process.c (hold/wait/interrupt/stop + the
//    enqueue-intent -> yield -> revalidate -> resume-with-signal discipline,
//    cmb_process.c:481-508)                        -> Proc + await_cleanup()
//  - reference src/cmb_resourceguard.c (demand-predicate wait queue,
//    stale-grant handling :186-228)                -> Guard + guard_signal()
//  - reference src/cmb_resource.c / cmb_resourcepool.c / cmb_buffer.c /
//    cmb_objectqueue.c / cmb_priorityqueue.c / cmb_condition.c -> the
//    fixed-capacity toolkit structs in this header.
//
// Everything is bounded-capacity (Cfg) so a trial's engine fits in LDS;
// capacity overflow aborts the trial with a status code (the per-block
// trial-abort flag of SURVEY.md §5.3) rather than growing.
#pragma once

#include <type_traits>

#include "config.hpp"
#include "devlog.hpp"
#include "hashheap.hpp"
#include "rng.hpp"
#include "stats.hpp"
#include "tally.hpp"

namespace cmb {

// ---- signals (same contract as reference include/cmb_process.h:60-100) ----
typedef int64_t sig_t;
constexpr sig_t SIG_SUCCESS = 0;
constexpr sig_t SIG_PREEMPTED = -1;
constexpr sig_t SIG_INTERRUPTED = -2;
constexpr sig_t SIG_STOPPED = -3;
constexpr sig_t SIG_CANCELLED = -4;
constexpr sig_t SIG_TIMEOUT = -5;

// ---- engine status codes (trial abort reasons) ----
enum EngStatus : int32_t {
    ST_OK = 0,
    ST_HEAP_FULL = 1,
    ST_QUEUE_FULL = 2,
    ST_BAD_STATE = 3,
    ST_GUARD_OVERFLOW = 4,
    ST_USER_ABORT = 5,
    ST_EVENT_LIMIT = 6,
};

// name of a status word (host formatting of the device log's abort line)
inline const char* status_name(int32_t st) {
    switch (st) {
        case ST_OK: return "ok";
        case ST_HEAP_FULL: return "heap_full";
        case ST_QUEUE_FULL: return "queue_full";
        case ST_BAD_STATE: return "bad_state";
        case ST_GUARD_OVERFLOW: return "guard_overflow";
        case ST_USER_ABORT: return "user_abort";
        case ST_EVENT_LIMIT: return "event_limit";
    }
    return "status";
}

// ---- internal event kinds; model-defined kinds start at EV_USER ----
enum EvKind : uint16_t {
    EV_PROC_START = 1,
    EV_TIMER = 2,   // a=pidx, c=timer slot, b=signal
    EV_GRANT = 3,   // a=pidx, c=guard id,  b=wait key
    EV_RESUME = 4,  // a=pidx, c=epoch,     b=signal
    EV_USER = 16,
};

// ---- await kinds ----
enum AwaitKind : uint8_t {
    AW_NONE = 0,
    AW_TIME = 1,   // blocking hold; key = timer-0 event handle
    AW_GUARD = 2,  // guard wait;    key = wait_key
    AW_PROC = 3,   // wait_process;  key = target pidx
    AW_EVENT = 4,  // wait_event;    key = event handle
};

// ---- demand predicate kinds (guard wait conditions) ----
enum DemandKind : uint8_t {
    DEM_QSPACE = 1,  // ctx = queue idx: space in object queue
    DEM_QOBJ = 2,    // ctx = queue idx: object available
    DEM_RES = 3,     // ctx = resource idx: resource free
    DEM_POOL = 4,    // ctx = pool idx: any units free
    DEM_BUF_GE = 5,  // ctx = buf idx | amount<<8: level >= amount
    DEM_BUF_SP = 6,  // ctx = buf idx | amount<<8: space >= amount
    DEM_PQOBJ = 7,   // ctx = pq idx: object available
    DEM_PQSP = 8,    // ctx = pq idx: space available
    DEM_POOL_GE = 9, // ctx = pool idx | amount<<8: free >= amount
    DEM_USER = 32,   // >= DEM_USER: Model::demand(E, pidx, kind, ctx)
};

enum ProcState : uint8_t {
    PS_UNINIT = 0,
    PS_READY = 1,    // initialized, not started
    PS_RUNNING = 2,  // started (running or blocked)
    PS_FINISHED = 3,
};

constexpr int16_t PC_DONE = -1;

// ---------------------------------------------------------------------------
// Process record.  This replaces the reference's cmb_process + embedded
// cmi_coroutine (include/cmb_process.h:118-128): the coroutine stack becomes
// (pc, model frame); awaits/resources/waiters lists become the fields below.
// ---------------------------------------------------------------------------
template <int NT>
struct ProcRec {
    int16_t pc;
    uint8_t state;
    uint8_t func;       // model process-function id
    int16_t priority;
    uint8_t await_kind;
    uint8_t g_granted;  // guard grant consumed by the next try_*
    uint32_t await_key;
    uint32_t epoch;     // bumped at every blocking setup; staleness key for EV_RESUME
    sig_t sig;          // signal delivered at resume (CMB_SIG())
    // guard-wait bookkeeping (valid while await_kind == AW_GUARD)
    int16_t gid;
    int16_t gnext;      // intrusive waiter list link
    uint8_t demand_kind;
    uint8_t pad0_;
    uint16_t pad1_;
    uint32_t demand_ctx;
    uint64_t wseq;      // FIFO tie-break within a guard; 64-bit so an
                        // EV_GRANT can never alias a new wait on the same
                        // guard, whatever the trial length
    uint64_t grank;     // packed wait rank (32767-priority)<<48 | wseq:
                        // wseq is monotone in dispatch order, so entry_t
                        // never decides (it ties exactly when wseq does),
                        // and the guard-front scan loads ONE word per
                        // waiter instead of three fields
    double entry_t;     // guard entry time (ordering: pri desc, entry asc, seq asc)
    uint32_t timers[NT];  // pending timer event handles; 0 = free slot
    int16_t waiters_head;  // procs waiting for me to finish (wait_process)
    int16_t pnext;         // my link in another proc's waiter list
};

// ---------------------------------------------------------------------------
// Interaction toolkit (fixed capacity, all POD)
// ---------------------------------------------------------------------------

struct Guard {
    int16_t head;      // waiter list (proc indices via gnext), -1 = empty
    int16_t observer;  // condition index observing this guard, -1 = none
    uint32_t pad_;
    // Waiter BITMASK, maintained instead of the list when MAX_PROC <= 64:
    // guard_front's waiter walk becomes a bit-iterate whose ProcRec loads
    // are INDEPENDENT (memory-level parallel) instead of a serial
    // pointer-chase through gnext links — the dominant latency chain in
    // pool-heavy models (JobShop, profiles/r01_lane_divergence.md).
    uint64_t wmask;
};

// Time-weighted statistic of one queue, resource, pool or buffer: the
// running summary and the time of its last sample.  Only a `recording`
// object touches its record, so the records live in the cold half of the
// engine storage (Engine::Cold::qstats/rstats/pstats/bstats) and the
// toolkit headers below keep only the 1-byte `recording` flag.
struct WtdRec {
    WtdSummary stats;
    double t_last;
};

// spill-tier FIFO segment of an object queue (logical order: ring
// entries, then spill entries).  Only a model that declares Cfg::SPILL_Q
// carries the cursors; the header of a spill-less model has no such bytes
struct QSpillCursors {
    int32_t sp_head, sp_len;
};
struct QNoSpill {};

// FIFO object queue of 64-bit payloads (reference cmb_objectqueue: FIFO of
// void*, two guards, capacity limit, length history).
// This is the queue HEADER: the CAP-slot ring itself lives in the cold
// half of the engine storage (Engine::Cold::qring, reached through
// Engine::qslot) and so does the length history (Cold::qstats), so the
// header can sit in a small hot tier.
template <int CAP, bool SPILL = false>
struct ObjQueue : std::conditional_t<SPILL, QSpillCursors, QNoSpill> {
    int32_t head, len;
    int32_t limit;       // runtime capacity; CMB_UNLIMITED -> CAP (+spill)
    int16_t g_front;     // getters wait here
    int16_t g_rear;      // putters wait here
    uint8_t recording;   // time-weighted queue length -> Cold::qstats
};

// one-holder resource (reference cmb_resource: binary semaphore with
// priority queue + preemption)
struct Resource {
    int16_t holder;  // proc idx or -1
    int16_t gid;
    uint8_t recording;  // time-weighted utilization (0/1) -> Cold::rstats
};

// counting semaphore (reference cmb_resourcepool)
struct Pool {
    int32_t capacity;
    int32_t in_use;
    int16_t gid;
    uint8_t recording;  // time-weighted units in use -> Cold::pstats
};

// producer/consumer level store (reference cmb_buffer)
struct Buffer {
    int64_t level;
    int64_t capacity;
    int16_t g_get;  // getters wait here (front)
    int16_t g_put;  // putters wait here (rear)
    uint8_t recording;  // time-weighted level -> Cold::bstats
};

// priority-ordered object queue (reference cmb_priorityqueue: objects
// retrieved in (priority desc, FIFO) order)
template <int CAP>
struct PrioQueue {
    uint64_t key[CAP];  // (32767-pri)<<32 | seq
    uint64_t val[CAP];
    int32_t len;
    int32_t limit;
    uint32_t seq;
    int16_t g_front, g_rear;
    uint8_t recording;
    WtdSummary len_stats;
    double t_last;
};

// condition variable (reference cmb_condition: wait on arbitrary predicate;
// signal wakes EVERY satisfied waiter; may observe other guards)
struct Condition {
    int16_t gid;
};

constexpr int32_t CMB_UNLIMITED = 0x7FFFFFFF;

// Default model hooks: models inherit and override what they use.
struct ModelBase {
    struct Globals {};  // model-wide per-trial state (override as needed)
    template <class E_>
    CMB_FORCEINLINE static bool demand(E_&, int /*pidx*/, uint8_t /*kind*/, uint32_t /*ctx*/) {
        return false;
    }
    template <class E_>
    CMB_FORCEINLINE static void on_event(E_&, const EvEntry&) {}
};

template <int N>
struct ArrOf {
    static constexpr int n = (N > 0) ? N : 1;
};

// Optional Cfg spill capacities (default 0 = no spill tier, zero cost).
// Models opt in by declaring SPILL_EV / SPILL_Q in their Cfg — the
// MI355X answer to the reference's unbounded doubling growth
// (cmi_hashheap.c:380-432): bounded fast tier in LDS/scratch, bulk
// overflow in an HBM slab claimed on first use from a shared pool.
template <class C, class = void>
struct SpillEvOf {
    static constexpr int v = 0;
};
template <class C>
struct SpillEvOf<C, std::void_t<decltype(C::SPILL_EV)>> {
    static constexpr int v = C::SPILL_EV;
};
template <class C, class = void>
struct SpillQOf {
    static constexpr int v = 0;
};
template <class C>
struct SpillQOf<C, std::void_t<decltype(C::SPILL_Q)>> {
    static constexpr int v = C::SPILL_Q;
};
template <class C, class = void>
struct SpillPqOf {
    static constexpr int v = 0;
};
template <class C>
struct SpillPqOf<C, std::void_t<decltype(C::SPILL_PQ)>> {
    static constexpr int v = C::SPILL_PQ;
};
// optional Cfg::EV_MAP: handle->index back-map for host-scale heaps
template <class C, class = void>
struct EvMapOf {
    static constexpr bool v = false;
};
template <class C>
struct EvMapOf<C, std::void_t<decltype(C::EV_MAP)>> {
    static constexpr bool v = C::EV_MAP;
};

// optional Cfg::HOT_EV: leading event-heap entries kept in the hot half
// of the storage (hashheap.hpp hot tier); default 0 = no hot tier
template <class C, class = void>
struct HotEvOf {
    static constexpr int v = 0;
};
template <class C>
struct HotEvOf<C, std::void_t<decltype(C::HOT_EV)>> {
    static constexpr int v = C::HOT_EV;
};
// optional Cfg::LDS_HOT: the model's hot half is small enough for the
// per-lane LDS kernel (hip/deskernel_impl.hpp conv_lds_kernel)
template <class C, class = void>
struct LdsHotOf {
    static constexpr bool v = false;
};
template <class C>
struct LdsHotOf<C, std::void_t<decltype(C::LDS_HOT)>> {
    static constexpr bool v = C::LDS_HOT;
};

// N-element array member that takes no room at N == 0: the storage
// halves inherit one per toolkit kind, so an unused kind costs the hot
// half nothing (its one-element placeholder goes to the cold half)
template <class T, int N>
struct TierArr {
    T v[N];
};
template <class T>
struct TierArr<T, 0> {};

// ---------------------------------------------------------------------------
// The engine
// ---------------------------------------------------------------------------

// What a model's engine is made of — capacities, record types and the
// storage blocks — apart from the engine itself, so that every Engine
// flavour of one model (below) shares the same Storage and Spill types.
template <class Model>
struct EngineTypes {
    using Cfg = typename Model::Cfg;
    using Params = typename Model::Params;
    using Frame = typename Model::Frame;
    using ProcT = ProcRec<Cfg::TIMERS>;
    using QueueT = ObjQueue<Cfg::QCAP, (SpillQOf<Cfg>::v > 0)>;

    static constexpr int NQ = Cfg::NUM_QUEUES;
    static constexpr int NR = Cfg::NUM_RES;
    static constexpr int NP = Cfg::NUM_POOLS;
    static constexpr int NB = Cfg::NUM_BUFS;
    static constexpr int NPQ = Cfg::NUM_PQ;
    static constexpr int NC = Cfg::NUM_COND;
    static constexpr int SPILL_EV = SpillEvOf<Cfg>::v;
    static constexpr int SPILL_Q = SpillQOf<Cfg>::v;
    static constexpr int SPILL_PQ = SpillPqOf<Cfg>::v;
    static constexpr bool NEEDS_SPILL =
        (SPILL_EV > 0) || (SPILL_Q > 0) || (SPILL_PQ > 0);
    static constexpr bool EV_MAP = EvMapOf<Cfg>::v;
    // device log stream (devlog.hpp): ring cursor + sink live in the
    // LogState base, which is empty unless Cfg::DEVICE_LOG
    static constexpr bool DEVICE_LOG = DevLogOf<Cfg>::v;
    // device tally stream (tally.hpp): sink + slot pointer live in the
    // TallyState base, which is empty unless Cfg::DEVICE_TALLY
    static constexpr int TALLY_K = TallyOf<Cfg>::K;
    static constexpr int HOT_EV = HotEvOf<Cfg>::v;
    static constexpr bool LDS_HOT = LdsHotOf<Cfg>::v;
    static constexpr int32_t EV_MSIZE =
        HashHeap<Cfg::MAX_EV, SPILL_EV, EV_MAP, HOT_EV>::MSIZE;
    static constexpr int NGUARD =
        2 * NQ + NR + NP + 2 * NB + 2 * NPQ + NC > 0
            ? 2 * NQ + NR + NP + 2 * NB + 2 * NPQ + NC
            : 1;

    // ---- storage ----------------------------------------------------------
    // The POD block that holds every array, in two halves.  Hot is what a
    // dispatch walks — process records, frames, guards, the toolkit
    // headers and the first HOT_EV heap entries — a few hundred bytes for
    // a small model.  Cold is the bulk: queue rings, the rest of the
    // heap, the back-map, priority queues, pool holdings.  The two need
    // not be neighbours: conv_lds_kernel keeps Hot in a per-lane LDS slice
    // and Cold in scratch; every other user takes one contiguous Storage.
    // The engine scalars live in the Engine context below.
    struct Hot : TierArr<EvEntry, HOT_EV>,
                 TierArr<Resource, NR>,
                 TierArr<Pool, NP>,
                 TierArr<Buffer, NB>,
                 TierArr<Condition, NC> {
        typename Model::Globals globals;
        ProcT procs[Cfg::MAX_PROC];
        Frame frames[Cfg::MAX_PROC];
        Guard guards[NGUARD];
        QueueT queues[ArrOf<NQ>::n];
    };
    // the one-element placeholders of unused toolkit kinds live here
    struct Cold : TierArr<Resource, (NR > 0 ? 0 : 1)>,
                  TierArr<Pool, (NP > 0 ? 0 : 1)>,
                  TierArr<Buffer, (NB > 0 ? 0 : 1)>,
                  TierArr<Condition, (NC > 0 ? 0 : 1)> {
        EvEntry evbuf[Cfg::MAX_EV - HOT_EV];
        EvMapSlot evmap[EV_MAP ? EV_MSIZE : 1];
        uint64_t qring[ArrOf<NQ>::n][Cfg::QCAP];
        // time-weighted statistics of the toolkit objects, touched only
        // while the object is `recording`
        WtdRec qstats[ArrOf<NQ>::n];
        WtdRec rstats[ArrOf<NR>::n];
        WtdRec pstats[ArrOf<NP>::n];
        WtdRec bstats[ArrOf<NB>::n];
        // per-process pool holdings (reference tracks holders in a
        // hash-heap per pool for preemption victim choice,
        // include/cmb_resourcepool.h:23-26; here a dense [pool][proc]
        // table - bounded and branch-free)
        int32_t pool_held[ArrOf<NP>::n * Cfg::MAX_PROC];
        PrioQueue<Cfg::PQCAP> pqueues[ArrOf<NPQ>::n];
    };
    struct Storage {
        Hot hot;
        Cold cold;
    };

    // array of a toolkit kind: in Hot when the model has any, else the
    // Cold placeholder (never touched, it only binds the reference)
    template <class T, int N>
    CMB_FORCEINLINE static T (&tier_arr(TierArr<T, N>& h,
                                        TierArr<T, (N > 0 ? 0 : 1)>& c))
        [ArrOf<N>::n] {
        if constexpr (N > 0) {
            (void)c;
            return h.v;
        } else {
            (void)h;
            return c.v;
        }
    }
    CMB_FORCEINLINE static EvEntry* hot_ev(Hot& h) {
        if constexpr (HOT_EV > 0) {
            return static_cast<TierArr<EvEntry, HOT_EV>&>(h).v;
        } else {
            (void)h;
            return nullptr;
        }
    }

    // ---- spill tier (one slab per trial, claimed from a shared pool on
    // first overflow; slabs stay claimed across a lane's later trials) --
    struct Spill {
        EvEntry ev[ArrOf<SPILL_EV>::n];
        uint64_t q[ArrOf<NQ>::n][ArrOf<SPILL_Q>::n];
        uint64_t pqk[ArrOf<NPQ>::n][ArrOf<SPILL_PQ>::n];
        uint64_t pqv[ArrOf<NPQ>::n][ArrOf<SPILL_PQ>::n];
    };
};

// HotTier says where the caller keeps Hot: FlatTier (default) for any
// memory, LdsTier when it is in LDS (conv_lds_kernel) — see hashheap.hpp.
// Models are written against E_, so they run on either flavour.
template <class Model, class HotTier = FlatTier>
struct Engine : EngineTypes<Model>,
                LogState<DevLogOf<typename Model::Cfg>::v>,
                TallyState<TallyOf<typename Model::Cfg>::K> {
    using Types = EngineTypes<Model>;
    using Self = Engine<Model, HotTier>;
    using typename Types::Cfg;
    using typename Types::Params;
    using typename Types::Frame;
    using typename Types::ProcT;
    using typename Types::QueueT;
    using typename Types::Hot;
    using typename Types::Cold;
    using typename Types::Storage;
    using typename Types::Spill;
    using Types::NQ;
    using Types::NR;
    using Types::NP;
    using Types::NB;
    using Types::NPQ;
    using Types::NC;
    using Types::SPILL_EV;
    using Types::SPILL_Q;
    using Types::SPILL_PQ;
    using Types::NEEDS_SPILL;
    using Types::EV_MAP;
    using Types::DEVICE_LOG;
    using Types::TALLY_K;
    using Types::HOT_EV;
    using Types::LDS_HOT;
    using Types::NGUARD;
    using Types::hot_ev;
    using EvHeap = HashHeap<Cfg::MAX_EV, SPILL_EV, EV_MAP, HOT_EV, HotTier>;

    // ---- hot context (register-resident on the device) --------------------
    double now;
    uint64_t ev_dispatched;   // the benchmark metric: events executed
    uint64_t seq;             // event FIFO counter
    uint32_t next_handle;
    int32_t status;
    int32_t n_event_waiters;  // count of procs in AW_EVENT
    int16_t evw_head;         // intrusive event-waiter list head (pnext)
    uint32_t trial_index;
    const Params* params;
    Rng rng;
    EvHeap evq;  // entries in Storage, size here

    // ---- spill tier: this engine's slab and the pool it claims from ----
    Spill* spill = nullptr;        // this trial's slab (null = none yet)
    Spill* spill_arena = nullptr;  // pool base
    int32_t* spill_cursor = nullptr;
    int32_t spill_pool_cap = 0;

    // ---- references into storage (existing field syntax keeps working) ----
    typename Model::Globals& globals;
    ProcT (&procs)[Cfg::MAX_PROC];
    Frame (&frames)[Cfg::MAX_PROC];
    Guard (&guards)[NGUARD];
    QueueT (&queues)[ArrOf<NQ>::n];
    Resource (&resources)[ArrOf<NR>::n];
    Pool (&pools)[ArrOf<NP>::n];
    int32_t (&pool_held)[ArrOf<NP>::n * Cfg::MAX_PROC];
    Buffer (&buffers)[ArrOf<NB>::n];
    PrioQueue<Cfg::PQCAP> (&pqueues)[ArrOf<NPQ>::n];
    Condition (&conds)[ArrOf<NC>::n];
    uint64_t (&qring)[ArrOf<NQ>::n][Cfg::QCAP];  // object-queue rings (Cold)
    // time-weighted statistics records (Cold), indexed like their objects
    WtdRec (&qstats)[ArrOf<NQ>::n];
    WtdRec (&rstats)[ArrOf<NR>::n];
    WtdRec (&pstats)[ArrOf<NP>::n];
    WtdRec (&bstats)[ArrOf<NB>::n];

    CMB_FORCEINLINE Engine(Hot& h, Cold& c)
        : evq(c.evbuf, hot_ev(h)), globals(h.globals), procs(h.procs),
          frames(h.frames), guards(h.guards), queues(h.queues),
          resources(Types::template tier_arr<Resource, NR>(h, c)),
          pools(Types::template tier_arr<Pool, NP>(h, c)),
          pool_held(c.pool_held),
          buffers(Types::template tier_arr<Buffer, NB>(h, c)),
          pqueues(c.pqueues),
          conds(Types::template tier_arr<Condition, NC>(h, c)),
          qring(c.qring), qstats(c.qstats), rstats(c.rstats),
          pstats(c.pstats), bstats(c.bstats) {
        if constexpr (EV_MAP) evq.map = c.evmap;
    }
    CMB_FORCEINLINE explicit Engine(Storage& s) : Engine(s.hot, s.cold) {}

    // ring slot `idx` of object queue `qi` — the one door to the rings
    CMB_FORCEINLINE uint64_t& qslot(int qi, int32_t idx) const {
        return qring[qi][idx];
    }

    // ---- lifecycle --------------------------------------------------------

    CMB_FORCEINLINE void init(const Params* p, uint64_t trial_seed, uint32_t tidx,
                     double start_time = 0.0) {
        now = start_time;
        ev_dispatched = 0;
        seq = 0;
        next_handle = 1;
        status = ST_OK;
        n_event_waiters = 0;
        evw_head = -1;
        trial_index = tidx;
        params = p;
        rng.seed(trial_seed);
        evq.reset();
        for (int i = 0; i < Cfg::MAX_PROC; ++i) {
            ProcT& pr = procs[i];
            pr.pc = 0;
            pr.state = PS_UNINIT;
            pr.func = 0;
            pr.priority = 0;
            pr.await_kind = AW_NONE;
            pr.g_granted = 0;
            pr.await_key = 0;
            pr.epoch = 0;
            pr.sig = SIG_SUCCESS;
            pr.gid = -1;
            pr.gnext = -1;
            pr.waiters_head = -1;
            pr.pnext = -1;
            for (int t = 0; t < Cfg::TIMERS; ++t) pr.timers[t] = 0;
        }
        for (int i = 0; i < NGUARD; ++i) {
            guards[i].head = -1;
            guards[i].observer = -1;
            guards[i].wmask = 0;
        }
        int g = 0;
        for (int i = 0; i < NQ; ++i) {
            QueueT& q = queues[i];
            q.head = 0; q.len = 0; q.limit = Cfg::QCAP + SPILL_Q;
            q.g_front = (int16_t)g++; q.g_rear = (int16_t)g++;
            q.recording = 0; qstats[i].stats.reset(); qstats[i].t_last = now;
            if constexpr (SPILL_Q > 0) { q.sp_head = 0; q.sp_len = 0; }
        }
        if (spill) evq.attach_spill(spill->ev, SPILL_EV);  // keep held slab
        for (int i = 0; i < NR; ++i) {
            resources[i].holder = -1; resources[i].gid = (int16_t)g++;
            resources[i].recording = 0; rstats[i].stats.reset();
            rstats[i].t_last = now;
        }
        for (int i = 0; i < NP; ++i) {
            pools[i].capacity = 1; pools[i].in_use = 0; pools[i].gid = (int16_t)g++;
            pools[i].recording = 0; pstats[i].stats.reset(); pstats[i].t_last = now;
        }
        for (int i = 0; i < NP * Cfg::MAX_PROC; ++i) pool_held[i] = 0;
        for (int i = 0; i < NB; ++i) {
            buffers[i].level = 0; buffers[i].capacity = CMB_UNLIMITED;
            buffers[i].g_get = (int16_t)g++; buffers[i].g_put = (int16_t)g++;
            buffers[i].recording = 0; bstats[i].stats.reset();
            bstats[i].t_last = now;
        }
        for (int i = 0; i < NPQ; ++i) {
            PrioQueue<Cfg::PQCAP>& q = pqueues[i];
            q.len = 0; q.limit = Cfg::PQCAP + SPILL_PQ; q.seq = 0;
            q.g_front = (int16_t)g++; q.g_rear = (int16_t)g++;
            q.recording = 0; q.len_stats.reset(); q.t_last = now;
        }
        for (int i = 0; i < NC; ++i) conds[i].gid = (int16_t)g++;
        if constexpr (DEVICE_LOG) this->log_bind(tidx);
        if constexpr (TALLY_K > 0) this->tally_bind(tidx);
    }

    static constexpr bool GUARD_MASK = (Cfg::MAX_PROC <= 64);

    // direct slab attach (host runner: one slab per worker engine)
    CMB_FORCEINLINE void set_spill(Spill* s_) {
        spill = s_;
        if (s_) evq.attach_spill(s_->ev, SPILL_EV);
    }

    // shared-pool attach (device launchers): claim lazily on overflow
    CMB_FORCEINLINE void set_spill_pool(Spill* arena, int32_t* cursor,
                                        int32_t cap) {
        spill_arena = arena;
        spill_cursor = cursor;
        spill_pool_cap = cap;
    }

    CMB_FORCEINLINE bool claim_spill() {
        if (spill) return true;
        if (!spill_arena) return false;
        int32_t idx;
#ifdef __HIP_DEVICE_COMPILE__
        idx = atomicAdd(spill_cursor, 1);
#else
        idx = __atomic_fetch_add(spill_cursor, 1, __ATOMIC_RELAXED);
#endif
        if (idx >= spill_pool_cap) return false;  // pool dry: abort path
        set_spill(&spill_arena[idx]);
        return true;
    }

    CMB_FORCEINLINE bool guard_empty(int gid) const {
        if constexpr (GUARD_MASK) return guards[gid].wmask == 0;
        else return guards[gid].head < 0;
    }

    CMB_FORCEINLINE void fail(int32_t st) {
        if constexpr (DEVICE_LOG) {
            // first failure: the status word becomes a timestamped last line
            if (status == ST_OK)
                this->log_emit(now, LOG_ERROR, (uint16_t)st, -1, LOGV_I64,
                               (uint64_t)(int64_t)st);
        }
        if (status == ST_OK) status = st;
    }

    // ---- device log stream (no-ops unless Cfg::DEVICE_LOG) -----------------

    // emit one record; never blocks, draws or schedules (CMB_LOG_* below)
    CMB_FORCEINLINE void log(uint32_t flags, uint16_t code, int16_t proc,
                             uint8_t vtype, uint64_t bits) {
        if constexpr (DEVICE_LOG)
            this->log_emit(now, flags, code, proc, vtype, bits);
    }

    // end-of-trial hook: every launcher and run_host call it right after
    // Model::finish; publishes this trial's emission count
    CMB_FORCEINLINE void log_finish() {
        if constexpr (DEVICE_LOG) this->log_flush();
    }

    // ---- device tally stream (no-op unless Cfg::DEVICE_TALLY) -------------

    // one observation into tally `id`; never blocks, draws or schedules
    // (CMB_TALLY below).  A constant id outside [0, K) does not compile
    CMB_FORCEINLINE void tally(int id, double x)
#if defined(__clang__)
        __attribute__((diagnose_if(TALLY_K > 0 && (id < 0 || id >= TALLY_K),
                                   "CMB_TALLY id is not below Cfg::DEVICE_TALLY",
                                   "error")))
#endif
    {
        if constexpr (TALLY_K > 0) {
            cmb_assert_debug(id >= 0 && id < TALLY_K);
            this->tally_add(id, x);
        } else {
            (void)id;
            (void)x;
        }
    }

    CMB_FORCEINLINE int pidx_of(const ProcT* p) const { return (int)(p - procs); }

    // ---- event scheduling (reference cmb_event_schedule, cmb_event.c:199) --

    CMB_FORCEINLINE uint32_t schedule(uint16_t kind, uint16_t a, uint32_t c,
                                      uint64_t b, double t, int priority) {
        EvEntry ev;
        ev.t = t;
        ev.pseq = ev_pseq(priority, seq++);
        ev.b = b;
        ev.handle = next_handle++;
        if (next_handle == 0) next_handle = 1;
        ev.kind = kind;
        ev.a = a;
        ev.c = c;
        if (!evq.push(ev)) {
            if constexpr (SPILL_EV > 0) {
                // first overflow: claim an HBM slab and retry
                if (claim_spill() && evq.push(ev)) return ev.handle;
            }
            fail(ST_HEAP_FULL);
            return 0;
        }
        return ev.handle;
    }

    CMB_FORCEINLINE bool event_cancel(uint32_t handle) {
        EvEntry out;
        if (!evq.cancel(handle, &out)) return false;
        if (n_event_waiters) wake_event_waiters(handle, SIG_CANCELLED);
        return true;
    }

    CMB_FORCEINLINE bool event_reschedule(uint32_t handle, double t, int priority) {
        return evq.reschedule(handle, t, ev_pseq(priority, seq++));
    }

    // ---- timers (reference cmb_process_timer_add/set/cancel/clear,
    //      cmb_process.c:514-580; slot 0 reserved for hold/timeout) ---------

    CMB_FORCEINLINE bool timer_add(ProcT& p, int slot, double delay, sig_t sg) {
        cmb_assert_debug(slot >= 0 && slot < Cfg::TIMERS);
        if (p.timers[slot]) return false;  // slot busy
        const uint32_t h = schedule(EV_TIMER, (uint16_t)pidx_of(&p), (uint32_t)slot,
                                    (uint64_t)sg, now + delay, p.priority);
        p.timers[slot] = h;
        return h != 0;
    }

    CMB_FORCEINLINE void timer_cancel(ProcT& p, int slot) {
        if (p.timers[slot]) {
            evq.cancel(p.timers[slot]);
            p.timers[slot] = 0;
        }
    }

    // ---- process control ---------------------------------------------------

    CMB_FORCEINLINE void proc_init(int pidx, uint8_t func, int priority) {
        ProcT& p = procs[pidx];
        cmb_assert_debug(p.state == PS_UNINIT);
        p.state = PS_READY;
        p.func = (uint8_t)func;
        p.priority = (int16_t)priority;
        p.pc = 0;
    }

    // non-blocking start: schedules a start event (reference
    // cmb_process_start, cmb_process.c:247-254)
    CMB_FORCEINLINE void proc_start(int pidx, double delay = 0.0) {
        ProcT& p = procs[pidx];
        cmb_assert_debug(p.state == PS_READY);
        schedule(EV_PROC_START, (uint16_t)pidx, 0, 0, now + delay, p.priority);
    }

    // non-blocking interrupt: wake the target's current wait with `sg`
    // (reference cmb_process_interrupt)
    CMB_FORCEINLINE void proc_interrupt(int pidx, sig_t sg) {
        ProcT& p = procs[pidx];
        if (p.state != PS_RUNNING || p.await_kind == AW_NONE) return;
        schedule(EV_RESUME, (uint16_t)pidx, p.epoch, (uint64_t)sg, now, p.priority);
    }

    // kill a process: drop resources, cancel awaitables, wake waiters
    // (reference kill path, cmb_process.c:979-1004)
    CMB_FORCEINLINE void proc_stop(int pidx) {
        ProcT& p = procs[pidx];
        if (p.state == PS_FINISHED || p.state == PS_UNINIT) return;
        for (int t = 0; t < Cfg::TIMERS; ++t) timer_cancel(p, t);
        if (p.await_kind == AW_GUARD) guard_unlink(p);
        if (p.await_kind == AW_PROC) proc_waiter_unlink(p);
        if (p.await_kind == AW_EVENT) {
            ev_waiter_unlink(p);
            --n_event_waiters;
        }
        p.await_kind = AW_NONE;
        drop_held(pidx);
        finish_common(p, SIG_STOPPED);
    }

    CMB_FORCEINLINE void proc_priority_set(int pidx, int priority) {
        ProcT& p = procs[pidx];
        p.priority = (int16_t)priority;
        if (p.await_kind == AW_GUARD)  // live reprioritization of a wait
            p.grank = ((uint64_t)(uint16_t)(32767 - p.priority) << 48) |
                      (p.wseq & UINT64_C(0xFFFFFFFFFFFF));
    }

    // allocate a process slot, recycling finished ones — the device-native
    // replacement for reference cmb_process_create()'s heap allocation
    // (dynamic entities draw from a bounded slot pool, cf. cmi_mempool)
    CMB_FORCEINLINE int proc_alloc() {
        for (int i = 0; i < Cfg::MAX_PROC; ++i) {
            ProcT& p = procs[i];
            if (p.state == PS_UNINIT || p.state == PS_FINISHED) {
                p.pc = 0;
                p.state = PS_UNINIT;
                p.await_kind = AW_NONE;
                p.g_granted = 0;
                p.await_key = 0;
                p.sig = SIG_SUCCESS;
                p.gid = -1;
                p.gnext = -1;
                p.waiters_head = -1;
                p.pnext = -1;
                for (int t = 0; t < Cfg::TIMERS; ++t) p.timers[t] = 0;
                return i;
            }
        }
        return -1;
    }

    // preemptive takeover (reference cmb_resource_preempt): returns true if
    // the caller now holds the resource; a lower-priority holder is kicked
    // with SIG_PREEMPTED delivered to its current blocking call
    CMB_FORCEINLINE bool res_try_preempt(int ri, ProcT& p) {
        Resource& r = resources[ri];
        if (r.holder < 0) {
            p.g_granted = 1;  // bypass the no-queue-jump check
            return res_try_acquire(ri, p);
        }
        ProcT& h = procs[r.holder];
        if (h.priority >= p.priority) return false;
        const int old = r.holder;
        if (r.recording) {
            rstats[ri].stats.add(1.0, now - rstats[ri].t_last);
            rstats[ri].t_last = now;
        }
        r.holder = (int16_t)pidx_of(&p);
        proc_interrupt(old, SIG_PREEMPTED);
        return true;
    }

    // register a condition as an observer of another guard (reference
    // cmb_resourceguard_register, include/cmb_resourceguard.h:168-179):
    // any signal on that guard re-evaluates the condition's waiters
    CMB_FORCEINLINE void condition_observe(int ci, int gid) {
        guards[gid].observer = (int16_t)ci;
    }
    CMB_FORCEINLINE void condition_unobserve(int gid) {
        guards[gid].observer = -1;
    }

    // called by CMB_END / early exit
    CMB_FORCEINLINE void proc_finish(ProcT& p) {
        p.pc = PC_DONE;
        drop_held(pidx_of(&p));
        finish_common(p, SIG_SUCCESS);
    }

    CMB_FORCEINLINE void finish_common(ProcT& p, sig_t waiter_sig) {
        p.state = PS_FINISHED;
        int16_t w = p.waiters_head;
        p.waiters_head = -1;
        while (w >= 0) {
            ProcT& wp = procs[w];
            const int16_t nxt = wp.pnext;
            wp.pnext = -1;
            schedule(EV_RESUME, (uint16_t)w, wp.epoch, (uint64_t)waiter_sig, now,
                     wp.priority);
            w = nxt;
        }
    }

    // release everything a killed/finished process still holds (reference
    // cmi_holdable drop polymorphism, src/cmi_holdable.h:53-78); bounded
    // scans over the small toolkit arrays replace the intrusive list.
    CMB_FORCEINLINE void drop_held(int pidx) {
        for (int r = 0; r < NR; ++r) {
            if (resources[r].holder == (int16_t)pidx) resource_release(r);
        }
        for (int p = 0; p < NP; ++p) {
            const int32_t held = pool_held[p * Cfg::MAX_PROC + pidx];
            if (held > 0) pool_release_for(p, pidx, held);
        }
    }

    // ---- the await/resume discipline --------------------------------------
    // reference pattern: (enqueue intent) -> yield ->
    // (scheduled wakeup revalidates intent) -> resume with signal.

    CMB_FORCEINLINE void await_setup(ProcT& p, uint8_t kind, uint32_t key) {
        p.await_kind = kind;
        p.await_key = key;
        p.epoch++;
    }

    // runs at every resumption point before user code continues: clears any
    // residue of the primary await when the wake came from elsewhere
    // (timer/interrupt), mirroring the reference's revalidation discipline.
    CMB_FORCEINLINE void await_cleanup(ProcT& p) {
        switch (p.await_kind) {
            case AW_NONE: return;
            case AW_TIME:
                // woken by something other than the hold timer: cancel it
                // (reference cmb_process.c:467-471)
                timer_cancel(p, 0);
                break;
            case AW_GUARD:
                guard_unlink(p);
                break;
            case AW_PROC:
                proc_waiter_unlink(p);
                break;
            case AW_EVENT:
                ev_waiter_unlink(p);
                --n_event_waiters;
                break;
        }
        p.await_kind = AW_NONE;
    }

    // blocking-call setups (used by the CMB_* macros) ---------------------

    CMB_FORCEINLINE void hold_setup(ProcT& p, double dur) {
        timer_add(p, 0, dur, SIG_SUCCESS);
        await_setup(p, AW_TIME, p.timers[0]);
    }

    CMB_FORCEINLINE void timeout_arm(ProcT& p, double dur) {
        timer_add(p, 0, dur, SIG_TIMEOUT);
    }
    CMB_FORCEINLINE void timeout_disarm(ProcT& p) { timer_cancel(p, 0); }

    CMB_FORCEINLINE bool wait_proc_setup(ProcT& p, int target) {
        ProcT& t = procs[target];
        if (t.state == PS_FINISHED) return false;  // no wait needed
        p.pnext = t.waiters_head;
        t.waiters_head = (int16_t)pidx_of(&p);
        await_setup(p, AW_PROC, (uint32_t)target);
        return true;
    }

    CMB_FORCEINLINE void proc_waiter_unlink(ProcT& p) {
        ProcT& t = procs[p.await_key];
        int16_t* link = &t.waiters_head;
        const int16_t me = (int16_t)pidx_of(&p);
        while (*link >= 0) {
            if (*link == me) {
                *link = p.pnext;
                p.pnext = -1;
                return;
            }
            link = &procs[*link].pnext;
        }
    }

    // event waiters sit on ONE intrusive list (pnext — exclusive with its
    // AW_PROC use, a process has a single await): wake walks the actual
    // waiters instead of scanning all MAX_PROC slots (O(4096) per event
    // in the host configuration — VERDICT r01 weak #5)
    CMB_FORCEINLINE void wait_event_setup(ProcT& p, uint32_t handle) {
        await_setup(p, AW_EVENT, handle);
        p.pnext = evw_head;
        evw_head = (int16_t)pidx_of(&p);
        ++n_event_waiters;
    }

    CMB_FORCEINLINE void ev_waiter_unlink(ProcT& p) {
        int16_t* link = &evw_head;
        const int16_t me = (int16_t)pidx_of(&p);
        while (*link >= 0) {
            if (*link == me) {
                *link = p.pnext;
                p.pnext = -1;
                return;
            }
            link = &procs[*link].pnext;
        }
    }

    CMB_FORCEINLINE void wake_event_waiters(uint32_t handle, sig_t sg) {
        for (int16_t i = evw_head; i >= 0; i = procs[i].pnext) {
            ProcT& p = procs[i];
            if (p.await_key == handle) {
                schedule(EV_RESUME, (uint16_t)i, p.epoch, (uint64_t)sg, now,
                         p.priority);
            }
        }
    }

    // ---- guards (reference cmb_resourceguard.c) ---------------------------

    CMB_FORCEINLINE void guard_wait(ProcT& p, int gid, uint8_t demand,
                                    uint32_t ctx) {
        p.gid = (int16_t)gid;
        p.demand_kind = demand;
        p.demand_ctx = ctx;
        p.entry_t = now;
        p.wseq = seq++;
        p.grank = ((uint64_t)(uint16_t)(32767 - p.priority) << 48) |
                  (p.wseq & UINT64_C(0xFFFFFFFFFFFF));
        if constexpr (GUARD_MASK) {
            guards[gid].wmask |= (uint64_t)1 << pidx_of(&p);
        } else {
            p.gnext = guards[gid].head;
            guards[gid].head = (int16_t)pidx_of(&p);
        }
        await_setup(p, AW_GUARD, (uint32_t)p.wseq);  // key is informational
    }

    CMB_FORCEINLINE void guard_unlink(ProcT& p) {
        Guard& g = guards[p.gid];
        if constexpr (GUARD_MASK) {
            g.wmask &= ~((uint64_t)1 << pidx_of(&p));
            return;
        }
        int16_t* link = &g.head;
        const int16_t me = (int16_t)pidx_of(&p);
        while (*link >= 0) {
            if (*link == me) {
                *link = p.gnext;
                p.gnext = -1;
                return;
            }
            link = &procs[*link].gnext;
        }
    }

    // front waiter: max priority, then earliest entry time, then lowest seq
    // (reference cmb_resourceguard.c:66-89 ordering)
    CMB_FORCEINLINE int guard_front(int gid) const {
        int best = -1;
        if constexpr (GUARD_MASK) {
            uint64_t m = guards[gid].wmask;
            uint64_t bestr = ~UINT64_C(0);
            while (m) {
                const int i = __builtin_ctzll(m);
                m &= m - 1;
                const uint64_t r = procs[i].grank;
                if (r < bestr) {
                    bestr = r;
                    best = i;
                }
            }
            return best;
        }
        for (int16_t i = guards[gid].head; i >= 0; i = procs[i].gnext) {
            if (best < 0) { best = i; continue; }
            const ProcT& a = procs[i];
            const ProcT& b = procs[best];
            if (a.priority > b.priority ||
                (a.priority == b.priority &&
                 (a.entry_t < b.entry_t ||
                  (a.entry_t == b.entry_t && a.wseq < b.wseq))))
                best = i;
        }
        return best;
    }

    CMB_FORCEINLINE bool eval_demand(const ProcT& p) {
        const uint32_t ctx = p.demand_ctx;
        switch (p.demand_kind) {
            case DEM_QSPACE: return q_len(queues[ctx]) < queues[ctx].limit;
            case DEM_QOBJ: return q_len(queues[ctx]) > 0;
            case DEM_RES: return resources[ctx].holder < 0;
            case DEM_POOL: return pools[ctx].in_use < pools[ctx].capacity;
            case DEM_BUF_GE:
                return buffers[ctx & 0xFF].level >= (int64_t)(ctx >> 8);
            case DEM_BUF_SP:
                return buffers[ctx & 0xFF].capacity - buffers[ctx & 0xFF].level >=
                       (int64_t)(ctx >> 8);
            case DEM_PQOBJ: return pqueues[ctx].len > 0;
            case DEM_PQSP: return pqueues[ctx].len < pqueues[ctx].limit;
            case DEM_POOL_GE:
                return pools[ctx & 0xFF].capacity - pools[ctx & 0xFF].in_use >=
                       (int32_t)(ctx >> 8);
            default:
                return Model::demand(*this, (int)(&p - procs), p.demand_kind, ctx);
        }
    }

    // evaluate the front waiter's demand; if satisfied, schedule a grant
    // event (reference cmb_resourceguard.c:240-260 semantics: the grant is
    // a hint — the woken process revalidates in its acquire loop)
    CMB_FORCEINLINE bool guard_signal(int gid) {
        const int w = guard_front(gid);
        bool granted = false;
        if (w >= 0 && eval_demand(procs[w])) {
            ProcT& p = procs[w];
            schedule(EV_GRANT, (uint16_t)w, (uint32_t)gid, p.wseq, now,
                     p.priority);
            granted = true;
        }
        const int16_t obs = guards[gid].observer;
        if (obs >= 0) condition_signal(obs);
        return granted;
    }

    // condition signal: wake EVERY satisfied waiter (reference
    // include/cmb_condition.h:17-24)
    CMB_FORCEINLINE uint64_t condition_signal(int ci) {
        const int gid = conds[ci].gid;
        uint64_t cnt = 0;
        if constexpr (GUARD_MASK) {
            uint64_t m = guards[gid].wmask;
            while (m) {
                const int i = __builtin_ctzll(m);
                m &= m - 1;
                if (eval_demand(procs[i])) {
                    ProcT& p = procs[i];
                    schedule(EV_GRANT, (uint16_t)i, (uint32_t)gid, p.wseq,
                             now, p.priority);
                    ++cnt;
                }
            }
            return cnt;
        }
        for (int16_t i = guards[gid].head; i >= 0; i = procs[i].gnext) {
            if (eval_demand(procs[i])) {
                ProcT& p = procs[i];
                schedule(EV_GRANT, (uint16_t)i, (uint32_t)gid, p.wseq,
                         now, p.priority);
                ++cnt;
            }
        }
        return cnt;
    }

    // ---- toolkit operations ------------------------------------------------

    // entries in the ring plus, where the model has the tier, in the spill
    // segment; a spill-less header has no cursors to load
    CMB_FORCEINLINE static int32_t q_len(const QueueT& q) {
        if constexpr (SPILL_Q > 0) return q.len + q.sp_len;
        else return q.len;
    }
    CMB_FORCEINLINE static bool q_spilling(const QueueT& q) {
        if constexpr (SPILL_Q > 0) return q.sp_len > 0;
        else return false;
    }

    CMB_FORCEINLINE void q_record(int qi) {
        if (queues[qi].recording) {
            WtdRec& st = qstats[qi];
            st.stats.add((double)q_len(queues[qi]), now - st.t_last);
            st.t_last = now;
        }
    }

    CMB_FORCEINLINE bool q_try_put(int qi, ProcT& p, uint64_t val) {
        QueueT& q = queues[qi];
        const bool may = p.g_granted || guard_empty(q.g_rear);
        p.g_granted = 0;
        if (!may || q_len(q) >= q.limit) return false;
        if (q.len >= Cfg::QCAP || q_spilling(q)) {
            // ring full, or spill already active (FIFO: the spill segment
            // follows the ring, and gets refill the ring from its head)
            if constexpr (SPILL_Q > 0) {
                if (!claim_spill() || q.sp_len >= SPILL_Q) {
                    fail(ST_QUEUE_FULL);
                    return false;
                }
                q_record(qi);
                spill->q[qi][(q.sp_head + q.sp_len) % SPILL_Q] = val;
                ++q.sp_len;
                guard_signal(q.g_front);
                return true;
            } else {
                fail(ST_QUEUE_FULL);
                return false;
            }
        }
        q_record(qi);
        qslot(qi, (q.head + q.len) % Cfg::QCAP) = val;
        ++q.len;
        guard_signal(q.g_front);
        return true;
    }

    CMB_FORCEINLINE bool q_try_get(int qi, ProcT& p, uint64_t* out) {
        QueueT& q = queues[qi];
        const bool may = p.g_granted || guard_empty(q.g_front);
        p.g_granted = 0;
        if (!may || q_len(q) == 0) return false;
        q_record(qi);
        *out = qslot(qi, q.head);
        q.head = (q.head + 1) % Cfg::QCAP;
        --q.len;
        if constexpr (SPILL_Q > 0) {
            if (q.sp_len > 0) {  // refill the ring tail from the spill head
                qslot(qi, (q.head + q.len) % Cfg::QCAP) =
                    spill->q[qi][q.sp_head];
                q.sp_head = (q.sp_head + 1) % SPILL_Q;
                --q.sp_len;
                ++q.len;
            }
        }
        guard_signal(q.g_rear);
        return true;
    }

    CMB_FORCEINLINE int64_t q_length(int qi) const {
        return (int64_t)q_len(queues[qi]);
    }

    // priority-queue heap entries span the fast arrays and (when the
    // model declares Cfg::SPILL_PQ) the spill slab, index-contiguously —
    // same two-tier shape as the event heap
    CMB_FORCEINLINE uint64_t& pqkey_at(int qi, int32_t i) {
        PrioQueue<Cfg::PQCAP>& q = pqueues[qi];
        if constexpr (SPILL_PQ > 0) {
            return i < Cfg::PQCAP ? q.key[i] : spill->pqk[qi][i - Cfg::PQCAP];
        } else {
            return q.key[i];
        }
    }
    CMB_FORCEINLINE uint64_t& pqval_at(int qi, int32_t i) {
        PrioQueue<Cfg::PQCAP>& q = pqueues[qi];
        if constexpr (SPILL_PQ > 0) {
            return i < Cfg::PQCAP ? q.val[i] : spill->pqv[qi][i - Cfg::PQCAP];
        } else {
            return q.val[i];
        }
    }
    CMB_FORCEINLINE int32_t pq_capacity() {
        if constexpr (SPILL_PQ > 0) {
            return claim_spill() ? Cfg::PQCAP + SPILL_PQ : Cfg::PQCAP;
        } else {
            return Cfg::PQCAP;
        }
    }

    CMB_FORCEINLINE bool pq_try_put(int qi, ProcT& p, uint64_t val, int priority) {
        PrioQueue<Cfg::PQCAP>& q = pqueues[qi];
        const bool may = p.g_granted || guard_empty(q.g_rear);
        p.g_granted = 0;
        if (!may || q.len >= q.limit) return false;
        if (q.len >= Cfg::PQCAP && q.len >= pq_capacity()) {
            fail(ST_QUEUE_FULL);
            return false;
        }
        // binary heap push keyed (pri desc, seq asc)
        const uint64_t key =
            ((uint64_t)(uint16_t)(32767 - priority) << 32) | q.seq++;
        int32_t i = q.len++;
        while (i > 0) {
            const int32_t par = (i - 1) >> 1;
            if (pqkey_at(qi, par) <= key) break;
            pqkey_at(qi, i) = pqkey_at(qi, par);
            pqval_at(qi, i) = pqval_at(qi, par);
            i = par;
        }
        pqkey_at(qi, i) = key;
        pqval_at(qi, i) = val;
        guard_signal(q.g_front);
        return true;
    }

    CMB_FORCEINLINE bool pq_try_get(int qi, ProcT& p, uint64_t* out) {
        PrioQueue<Cfg::PQCAP>& q = pqueues[qi];
        const bool may = p.g_granted || guard_empty(q.g_front);
        p.g_granted = 0;
        if (!may || q.len == 0) return false;
        *out = q.val[0];
        --q.len;
        const uint64_t key = pqkey_at(qi, q.len);
        const uint64_t val = pqval_at(qi, q.len);
        int32_t i = 0;
        for (;;) {
            int32_t c = 2 * i + 1;
            if (c >= q.len) break;
            if (c + 1 < q.len && pqkey_at(qi, c + 1) < pqkey_at(qi, c)) ++c;
            if (pqkey_at(qi, c) >= key) break;
            pqkey_at(qi, i) = pqkey_at(qi, c);
            pqval_at(qi, i) = pqval_at(qi, c);
            i = c;
        }
        pqkey_at(qi, i) = key;
        pqval_at(qi, i) = val;
        guard_signal(q.g_rear);
        return true;
    }

    CMB_FORCEINLINE bool res_try_acquire(int ri, ProcT& p) {
        Resource& r = resources[ri];
        const bool may = p.g_granted || guard_empty(r.gid);
        p.g_granted = 0;
        if (!may || r.holder >= 0) return false;
        if (r.recording) {
            rstats[ri].stats.add(0.0, now - rstats[ri].t_last);
            rstats[ri].t_last = now;
        }
        r.holder = (int16_t)pidx_of(&p);
        return true;
    }

    CMB_FORCEINLINE void resource_release(int ri) {
        Resource& r = resources[ri];
        cmb_assert_debug(r.holder >= 0);
        if (r.recording) {
            rstats[ri].stats.add(1.0, now - rstats[ri].t_last);
            rstats[ri].t_last = now;
        }
        r.holder = -1;
        guard_signal(r.gid);
    }

    CMB_FORCEINLINE int32_t pool_try_take(int pi, ProcT& p, int32_t want) {
        Pool& pl = pools[pi];
        const bool may = p.g_granted || guard_empty(pl.gid);
        p.g_granted = 0;
        if (!may) return 0;
        const int32_t free_units = pl.capacity - pl.in_use;
        const int32_t take = free_units < want ? free_units : want;
        if (take > 0) {
            if (pl.recording) {
                pstats[pi].stats.add((double)pl.in_use, now - pstats[pi].t_last);
                pstats[pi].t_last = now;
            }
            pl.in_use += take;
            pool_held[pi * Cfg::MAX_PROC + pidx_of(&p)] += take;
        }
        return take;
    }

    CMB_FORCEINLINE int32_t pool_holding(int pi, int pidx) const {
        return pool_held[pi * Cfg::MAX_PROC + pidx];
    }

    // preemptive multi-unit acquire (reference cmb_resourcepool_preempt:
    // grabs from lowest-priority holders, include/cmb_resourcepool.h:23-26).
    // All-or-nothing: free units + units reclaimable from strictly-lower-
    // priority holders must cover `want`; each victim is interrupted with
    // SIG_PREEMPTED and its holding reduced (check pool_holding() after).
    CMB_FORCEINLINE bool pool_try_preempt(int pi, ProcT& p, int32_t want) {
        Pool& pl = pools[pi];
        p.g_granted = 0;
        const int me = pidx_of(&p);
        const int32_t free_units = pl.capacity - pl.in_use;
        int32_t need = want - free_units;
        if (need > 0) {
            int32_t reclaimable = 0;
            for (int i = 0; i < Cfg::MAX_PROC; ++i) {
                if (i != me && procs[i].priority < p.priority)
                    reclaimable += pool_held[pi * Cfg::MAX_PROC + i];
            }
            if (reclaimable < need) return false;
            while (need > 0) {
                // lowest-priority victim first
                int victim = -1;
                for (int i = 0; i < Cfg::MAX_PROC; ++i) {
                    if (i == me || pool_held[pi * Cfg::MAX_PROC + i] <= 0)
                        continue;
                    if (procs[i].priority >= p.priority) continue;
                    if (victim < 0 ||
                        procs[i].priority < procs[victim].priority)
                        victim = i;
                }
                cmb_assert_debug(victim >= 0);
                int32_t& vh = pool_held[pi * Cfg::MAX_PROC + victim];
                const int32_t take = vh < need ? vh : need;
                vh -= take;
                need -= take;
                proc_interrupt(victim, SIG_PREEMPTED);
            }
        }
        if (pl.recording) {
            pstats[pi].stats.add((double)pl.in_use, now - pstats[pi].t_last);
            pstats[pi].t_last = now;
        }
        // transferred units stay in_use; only the free portion is new use
        const int32_t from_free = want < free_units ? want : free_units;
        pl.in_use += from_free;
        pool_held[pi * Cfg::MAX_PROC + me] += want;
        return true;
    }

    // all-or-nothing take (deadlock-free alternative to the greedy partial
    // loop for multi-unit requests; companion of CMB_POOL_ACQUIRE_ALL)
    CMB_FORCEINLINE bool pool_try_take_all(int pi, ProcT& p, int32_t want) {
        Pool& pl = pools[pi];
        const bool may = p.g_granted || guard_empty(pl.gid);
        p.g_granted = 0;
        if (!may || pl.capacity - pl.in_use < want) return false;
        if (pl.recording) {
            pstats[pi].stats.add((double)pl.in_use, now - pstats[pi].t_last);
            pstats[pi].t_last = now;
        }
        pl.in_use += want;
        pool_held[pi * Cfg::MAX_PROC + pidx_of(&p)] += want;
        return true;
    }

    CMB_FORCEINLINE void pool_release_for(int pi, int pidx, int32_t amount) {
        Pool& pl = pools[pi];
        int32_t& held = pool_held[pi * Cfg::MAX_PROC + pidx];
        cmb_assert_debug(pl.in_use >= amount && held >= amount);
        if (pl.recording) {
            pstats[pi].stats.add((double)pl.in_use, now - pstats[pi].t_last);
            pstats[pi].t_last = now;
        }
        held -= amount;
        pl.in_use -= amount;
        guard_signal(pl.gid);
    }

    CMB_FORCEINLINE void pool_release(int pi, ProcT& p, int32_t amount) {
        pool_release_for(pi, pidx_of(&p), amount);
    }

    CMB_FORCEINLINE bool buf_try_get(int bi, ProcT& p, int64_t amount) {
        Buffer& b = buffers[bi];
        const bool may = p.g_granted || guard_empty(b.g_get);
        p.g_granted = 0;
        if (!may || b.level < amount) return false;
        if (b.recording) {
            bstats[bi].stats.add((double)b.level, now - bstats[bi].t_last);
            bstats[bi].t_last = now;
        }
        b.level -= amount;
        guard_signal(b.g_put);
        return true;
    }

    CMB_FORCEINLINE bool buf_try_put(int bi, ProcT& p, int64_t amount) {
        Buffer& b = buffers[bi];
        const bool may = p.g_granted || guard_empty(b.g_put);
        p.g_granted = 0;
        if (!may || b.capacity - b.level < amount) return false;
        if (b.recording) {
            bstats[bi].stats.add((double)b.level, now - bstats[bi].t_last);
            bstats[bi].t_last = now;
        }
        b.level += amount;
        guard_signal(b.g_get);
        return true;
    }

    // ---- dispatch loop (reference cmb_event.c:370-410) ---------------------

    CMB_FORCEINLINE void resume_proc(int pidx, sig_t sg) {
        ProcT& p = procs[pidx];
        p.sig = sg;
        Model::step(*this, pidx);
    }

    CMB_FORCEINLINE bool dispatch_one() {
        if (status != ST_OK || evq.empty()) return false;
        const EvEntry ev = evq.pop();
        now = ev.t;
        ++ev_dispatched;
        if (n_event_waiters) wake_event_waiters(ev.handle, SIG_SUCCESS);
        switch (ev.kind) {
            case EV_PROC_START: {
                ProcT& p = procs[ev.a];
                if (p.state != PS_READY) break;  // stale (stopped before start)
                p.state = PS_RUNNING;
                resume_proc(ev.a, SIG_SUCCESS);
                break;
            }
            case EV_TIMER: {
                ProcT& p = procs[ev.a];
                if (p.timers[ev.c] != ev.handle) break;  // stale
                p.timers[ev.c] = 0;
                if (p.state != PS_RUNNING || p.await_kind == AW_NONE) break;
                if (p.await_kind == AW_TIME && p.await_key == ev.handle) {
                    // normal hold wake
                    p.await_kind = AW_NONE;
                }
                // otherwise: interrupting timer (timeout) — leave the
                // primary await for await_cleanup at the resumption point
                resume_proc(ev.a, (sig_t)ev.b);
                break;
            }
            case EV_GRANT: {
                ProcT& p = procs[ev.a];
                if (p.state == PS_RUNNING && p.await_kind == AW_GUARD &&
                    p.wseq == ev.b && p.gid == (int16_t)ev.c) {
                    guard_unlink(p);
                    p.await_kind = AW_NONE;
                    p.g_granted = 1;
                    resume_proc(ev.a, SIG_SUCCESS);
                } else {
                    // stale grant: the signal must not be lost — re-evaluate
                    // the guard (reference cmb_resourceguard.c:163-180
                    // pass-the-grant-on semantics)
                    guard_signal((int)ev.c);
                }
                break;
            }
            case EV_RESUME: {
                ProcT& p = procs[ev.a];
                if (p.state != PS_RUNNING || p.await_kind == AW_NONE ||
                    p.epoch != ev.c)
                    break;  // stale
                if (p.await_kind == AW_TIME || p.await_kind == AW_PROC ||
                    p.await_kind == AW_EVENT || p.await_kind == AW_GUARD) {
                    // leave residue for await_cleanup
                }
                resume_proc(ev.a, (sig_t)ev.b);
                break;
            }
            default:
                Model::on_event(*this, ev);
                break;
        }
        return true;
    }

    // ---- path peek: support for the vote-gated converged lane kernel
    // (hip/deskernel_impl.hpp conv_lane_kernel) ----

    // Identify the code path the NEXT dispatch_one() will take:
    // (event kind, owning process function, its resume pc).  Lanes whose
    // peeked paths are equal execute the same instruction stream through
    // dispatch + model step, so the converged kernel votes on this id.
    // PATH_DONE = the trial is finished under (until, max_events) — the
    // same conditions as run()'s loop.
    static constexpr uint32_t PATH_DONE = 0xFFFFFFFEu;
    static constexpr uint32_t PATH_DEAD = 0xFFFFFFFFu;  // no trial in slot

    CMB_FORCEINLINE uint32_t peek_path(double until,
                                       uint64_t max_events) const {
        if (status != ST_OK || evq.n == 0 || ev_dispatched >= max_events)
            return PATH_DONE;
        const EvEntry& ev = evq.top();
        if (ev.t > until) return PATH_DONE;
        uint32_t func = 0, pc = 0;
        if (ev.kind >= EV_PROC_START && ev.kind <= EV_RESUME) {
            const ProcT& p = procs[ev.a];
            func = p.func;
            pc = (uint16_t)p.pc;
        }
        return (((uint32_t)ev.kind & 0x7Fu) << 24) | (func << 16) | pc;
    }

    // run until the event queue drains (reference cmb_event_queue_execute,
    // cmb_event.c:402) or a limit is hit
    CMB_FORCEINLINE void run(double until, uint64_t max_events) {
        while (status == ST_OK && !evq.empty()) {
            if (evq.top().t > until) {
                now = until;
                break;
            }
            dispatch_one();
            if (ev_dispatched >= max_events) {
                fail(ST_EVENT_LIMIT);
                break;
            }
        }
    }
};

// ---------------------------------------------------------------------------
// Protothread macros — the blocking-call surface.  A model process function
// has the shape:
//
//   template <class E_>
//   CMB_HD static void body(E_& E, typename E_::ProcT* self) {
//       auto& f = E.frames[E.pidx_of(self)].xxx;   // persistent locals
//       CMB_BEGIN();
//       ...
//       CMB_HOLD(E.rng.exponential(m));            // blocking call
//       if (CMB_SIG() != cmb::SIG_SUCCESS) ...     // signal inspection
//       ...
//       CMB_END();
//   }
//
// Constraints (documented in docs/PARITY.md): one CMB_* blocking macro per
// source line; locals that live across a blocking call go in the frame.
// ---------------------------------------------------------------------------

#define CMB_BEGIN() switch (self->pc) { case 0:
#define CMB_END() \
    }             \
    E.proc_finish(*self); \
    return;

#define CMB_SIG() (self->sig)

// internal: yield and name the resumption point
#define CMB_YIELD_()            \
    self->pc = (int16_t)__LINE__; \
    return;                     \
    case __LINE__:              \
        E.await_cleanup(*self);

// hold for `dur` sim time (reference cmb_process_hold, cmb_process.c:452)
#define CMB_HOLD(dur)                 \
    do {                              \
        E.hold_setup(*self, (dur));   \
        CMB_YIELD_();                 \
    } while (0)

// wait for another process to finish (reference cmb_process_wait_process)
#define CMB_WAIT_PROCESS(tgt)                      \
    do {                                           \
        if (E.wait_proc_setup(*self, (tgt))) {     \
            CMB_YIELD_();                          \
        } else {                                   \
            self->sig = cmb::SIG_SUCCESS;          \
        }                                          \
    } while (0)

// wait for a scheduled event to execute (reference cmb_process_wait_event)
#define CMB_WAIT_EVENT(handle)                  \
    do {                                        \
        E.wait_event_setup(*self, (handle));    \
        CMB_YIELD_();                           \
    } while (0)

// generic guarded-retry loop body shared by the toolkit macros
#define CMB_GUARDED_(try_expr, gid_expr, demand, ctx)           \
    for (;;) {                                                  \
        if (try_expr) {                                         \
            self->sig = cmb::SIG_SUCCESS;                       \
            break;                                              \
        }                                                       \
        if (E.status != cmb::ST_OK) { self->sig = cmb::SIG_CANCELLED; break; } \
        E.guard_wait(*self, (gid_expr), (demand), (ctx));       \
        CMB_YIELD_();                                           \
        if (self->sig != cmb::SIG_SUCCESS) break;               \
        self->g_granted = 1;                                    \
    }

// object queue put/get (reference cmb_objectqueue_put/get)
#define CMB_QPUT(qi, val)                                              \
    CMB_GUARDED_(E.q_try_put((qi), *self, (val)), E.queues[qi].g_rear, \
                 cmb::DEM_QSPACE, (uint32_t)(qi))

#define CMB_QGET(qi, outp)                                              \
    CMB_GUARDED_(E.q_try_get((qi), *self, (outp)), E.queues[qi].g_front, \
                 cmb::DEM_QOBJ, (uint32_t)(qi))

// priority queue put/get (reference cmb_priorityqueue_put/get)
#define CMB_PQPUT(qi, val, pri)                                \
    CMB_GUARDED_(E.pq_try_put((qi), *self, (val), (pri)),      \
                 E.pqueues[qi].g_rear, cmb::DEM_PQSP, (uint32_t)(qi))

#define CMB_PQGET(qi, outp)                                     \
    CMB_GUARDED_(E.pq_try_get((qi), *self, (outp)),             \
                 E.pqueues[qi].g_front, cmb::DEM_PQOBJ, (uint32_t)(qi))

// resource acquire/release (reference cmb_resource_acquire/release,
// cmb_resource.c:235-277)
#define CMB_RES_ACQUIRE(ri)                                         \
    CMB_GUARDED_(E.res_try_acquire((ri), *self), E.resources[ri].gid, \
                 cmb::DEM_RES, (uint32_t)(ri))

#define CMB_RES_RELEASE(ri) E.resource_release((ri))

// preemptive acquire: takes the resource from any lower-priority holder
// (reference cmb_resource_preempt); falls back to a priority-ordered wait
#define CMB_RES_PREEMPT(ri)                                            \
    CMB_GUARDED_(E.res_try_preempt((ri), *self), E.resources[ri].gid,  \
                 cmb::DEM_RES, (uint32_t)(ri))

// pool acquire: greedy partial acquisition (reference
// include/cmb_resourcepool.h:15-19); `remvar` is a frame lvalue tracking
// the amount still wanted
#define CMB_POOL_ACQUIRE(pi, amount, remvar)                          \
    do {                                                              \
        (remvar) = (amount);                                          \
        for (;;) {                                                    \
            (remvar) -= E.pool_try_take((pi), *self, (remvar));       \
            if ((remvar) <= 0) { self->sig = cmb::SIG_SUCCESS; break; } \
            if (E.status != cmb::ST_OK) { self->sig = cmb::SIG_CANCELLED; break; } \
            E.guard_wait(*self, E.pools[pi].gid, cmb::DEM_POOL,       \
                         (uint32_t)(pi));                             \
            CMB_YIELD_();                                             \
            if (self->sig != cmb::SIG_SUCCESS) break;                 \
            self->g_granted = 1;                                      \
        }                                                             \
    } while (0)

#define CMB_POOL_RELEASE(pi, amount) E.pool_release((pi), *self, (amount))

// preemptive multi-unit pool acquire (reference cmb_resourcepool_preempt)
#define CMB_POOL_PREEMPT(pi, amount)                                       \
    CMB_GUARDED_(E.pool_try_preempt((pi), *self, (amount)),               \
                 E.pools[pi].gid, cmb::DEM_POOL_GE,                        \
                 (uint32_t)(pi) | ((uint32_t)(amount) << 8))

// all-or-nothing pool acquire: waits until `amount` units are free and
// takes them atomically (deadlock-free for multi-unit requests, unlike the
// reference's greedy loop — see docs/PARITY.md)
#define CMB_POOL_ACQUIRE_ALL(pi, amount)                                   \
    CMB_GUARDED_(E.pool_try_take_all((pi), *self, (amount)),               \
                 E.pools[pi].gid, cmb::DEM_POOL_GE,                        \
                 (uint32_t)(pi) | ((uint32_t)(amount) << 8))

// buffer get/put of `amount` units (reference cmb_buffer_get/put)
#define CMB_BUF_GET(bi, amount)                                           \
    CMB_GUARDED_(E.buf_try_get((bi), *self, (amount)), E.buffers[bi].g_get, \
                 cmb::DEM_BUF_GE,                                         \
                 (uint32_t)(bi) | ((uint32_t)(amount) << 8))

#define CMB_BUF_PUT(bi, amount)                                           \
    CMB_GUARDED_(E.buf_try_put((bi), *self, (amount)), E.buffers[bi].g_put, \
                 cmb::DEM_BUF_SP,                                         \
                 (uint32_t)(bi) | ((uint32_t)(amount) << 8))

// device log records (devlog.hpp): plain statements — they never block,
// never draw from the RNG and never schedule.  `flag` is one LogFlag bit
// (or a user bit), `code` is model-defined; no-ops unless Cfg::DEVICE_LOG
#define CMB_LOG_U(flag, code, val)                                     \
    E.log((flag), (uint16_t)(code), (int16_t)E.pidx_of(self),          \
          cmb::LOGV_U64, (uint64_t)(val))
#define CMB_LOG_I(flag, code, val)                                     \
    E.log((flag), (uint16_t)(code), (int16_t)E.pidx_of(self),          \
          cmb::LOGV_I64, (uint64_t)(int64_t)(val))
#define CMB_LOG_D(flag, code, val)                                     \
    E.log((flag), (uint16_t)(code), (int16_t)E.pidx_of(self),          \
          cmb::LOGV_F64, cmb::double_as_u64((double)(val)))

// device tally (tally.hpp): a plain statement like the log records — it
// never blocks, draws or schedules.  `id` < Cfg::DEVICE_TALLY picks the
// tally; a no-op unless the model opts in
#define CMB_TALLY(id, x) E.tally((id), (double)(x))

// condition wait on a user demand predicate (reference cmb_condition_wait)
#define CMB_COND_WAIT(ci, demand_id, ctx)                                \
    do {                                                                 \
        E.guard_wait(*self, E.conds[ci].gid, (uint8_t)(demand_id),       \
                     (uint32_t)(ctx));                                   \
        CMB_YIELD_();                                                    \
    } while (0)

}  // namespace cmb — note: macros are file-scope; namespace closed after
