// Seeded random driver for the object queue's register-resident front
// (engine.hpp qfront): one put/get/re-init sequence, a pure function of
// (seed, nops), run on a host engine of a tiny model (4-slot ring, 8-slot
// spill segment, one queue) with the front cache on (FlatFrontTier) or
// off (FlatTier).  What the gets return must not depend on the cache.
// Host only; shared by the Python binding (_C.queue_front_fuzz) and the
// stand-alone sanitizer program (host/queuefuzz_main.cpp).  Storage and
// spill slab are exact-size heap allocations.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "engine.hpp"

namespace cmb {

struct QFuzzModel : ModelBase {
    struct Cfg {
        static constexpr int MAX_PROC = 1;
        static constexpr int MAX_EV = 4;
        static constexpr int TIMERS = 1;
        static constexpr int NUM_QUEUES = 1;
        static constexpr int QCAP = 4;
        static constexpr int NUM_RES = 0;
        static constexpr int NUM_POOLS = 0;
        static constexpr int NUM_BUFS = 0;
        static constexpr int NUM_PQ = 0;
        static constexpr int PQCAP = 1;
        static constexpr int NUM_COND = 0;
        static constexpr int SPILL_Q = 8;
    };
    struct Params {};
    struct Frame {};
    template <class E_>
    CMB_FORCEINLINE static void step(E_&, int) {}
};

struct QueueFuzzOut {
    std::vector<uint64_t> gets;  // every get's value, in order
    std::vector<int32_t> lens;   // queue length after each op
    int32_t status = 0;          // engine status at the end
    // how often the sequence reached each case the cache must survive
    uint64_t wraps = 0;        // get that wraps head to slot 0
    uint64_t ring_full = 0;    // put that opens the spill segment
    uint64_t refill_front = 0; // new front is a slot a refill wrote
    uint64_t drain_put = 0;    // put into a queue that gets had emptied
    uint64_t queue_full = 0;   // put refused with ST_QUEUE_FULL at 12 queued
    uint64_t reinits = 0;      // init() with objects still queued
};

template <class Tier>
inline QueueFuzzOut queue_front_fuzz(uint64_t seed, uint64_t nops) {
    using Eng = Engine<QFuzzModel, Tier>;
    constexpr int QCAP = QFuzzModel::Cfg::QCAP;
    constexpr int TOTAL = QCAP + QFuzzModel::Cfg::SPILL_Q;
    auto store = std::make_unique<typename Eng::Storage>();
    auto slab = std::make_unique<typename Eng::Spill>();
    auto eng = std::make_unique<Eng>(*store);
    Eng& E = *eng;
    const QFuzzModel::Params P{};
    E.set_spill(slab.get());
    auto start_trial = [&](uint32_t tidx) {
        E.init(&P, seed + tidx, tidx);
        E.queues[0].limit = CMB_UNLIMITED;  // the capacity is the only bound
    };
    start_trial(0);

    uint64_t x = seed;
    auto rnd = [&x]() {  // splitmix64
        uint64_t z = (x += UINT64_C(0x9E3779B97F4A7C15));
        z = (z ^ (z >> 30)) * UINT64_C(0xBF58476D1CE4E5B9);
        z = (z ^ (z >> 27)) * UINT64_C(0x94D049BB133111EB);
        return z ^ (z >> 31);
    };
    QueueFuzzOut o;
    bool refilled[QCAP] = {};  // slot last written by a spill refill
    bool emptied = false;      // the last successful op was a draining get
    uint32_t trial = 0;
    for (uint64_t op = 0; op < nops; ++op) {
        const uint64_t r = rnd();
        auto& q = E.queues[0];
        // alternate 64-op phases that fill the queue (to the 12th entry
        // and one put beyond) and drain it (to empty)
        const int nput = ((op >> 6) & 1) ? 5 : 11;
        const int what = (int)(r % 16);
        if ((r >> 8) % 997 == 0 && Eng::q_len(q) > 0) {
            // a lane's next trial: whatever is queued is abandoned
            ++o.reinits;
            start_trial(++trial);
            for (bool& f : refilled) f = false;
            emptied = false;
        } else if (what < nput) {
            const int32_t before = Eng::q_len(q);
            if (before == 0 && emptied) ++o.drain_put;
            if (q.len == QCAP && q.sp_len == 0) ++o.ring_full;
            const int32_t slot = (q.head + q.len) % QCAP;
            const bool ring = q.len < QCAP && q.sp_len == 0;
            const bool ok = E.q_try_put(0, E.procs[0], r | 1u);
            if (ok && ring) refilled[slot] = false;
            if (!ok && before == TOTAL && E.status == ST_QUEUE_FULL)
                ++o.queue_full;
            if (ok) emptied = false;
        } else {
            const int32_t old_head = q.head;
            const bool spilling = q.sp_len > 0;
            uint64_t v = 0;
            if (E.q_try_get(0, E.procs[0], &v)) {
                o.gets.push_back(v);
                if (old_head == QCAP - 1) ++o.wraps;
                // a spilling queue has a full ring: the refill goes into
                // the slot this get vacated
                if (spilling) refilled[old_head] = true;
                if (Eng::q_len(q) > 0 && refilled[q.head]) ++o.refill_front;
                emptied = Eng::q_len(q) == 0;
            }
        }
        o.lens.push_back(Eng::q_len(E.queues[0]));
    }
    o.status = E.status;
    return o;
}

inline QueueFuzzOut queue_front_fuzz_n(uint64_t seed, uint64_t nops,
                                       bool cached) {
    return cached ? queue_front_fuzz<FlatFrontTier>(seed, nops)
                  : queue_front_fuzz<FlatTier>(seed, nops);
}

}  // namespace cmb
