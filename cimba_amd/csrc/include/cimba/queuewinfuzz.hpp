// Seeded random driver for the object queue's register window
// (engine.hpp QWindowState): one put/get/re-init sequence, a pure
// function of (seed, nops), run on a host engine of a tiny model (8-slot
// ring, 8-slot spill segment, one queue) at a window width W from 0 (the
// plain flavour) to 7, the widest the ring permits (QWinOf: QCAP - 1).
// What the gets return must not depend on W.  The driver keeps a shadow
// of the queue's logical positions to count how often the sequence
// reached each case a W-wide window has to survive; the counts are a
// function of (seed, nops, count_w) alone, so the plain flavour can be
// asked for them too.  Host only; shared by the Python binding
// (_C.queue_window_fuzz) and the stand-alone sanitizer program
// (host/queuewinfuzz_main.cpp).  Storage and spill slab are exact-size
// heap allocations.
#pragma once

#include <cstdint>
#include <deque>
#include <memory>
#include <vector>

#include "engine.hpp"

namespace cmb {

struct QWinFuzzModel : ModelBase {
    struct Cfg {
        static constexpr int MAX_PROC = 1;
        static constexpr int MAX_EV = 4;
        static constexpr int TIMERS = 1;
        static constexpr int NUM_QUEUES = 1;
        static constexpr int QCAP = 8;
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
constexpr int QWIN_FUZZ_MAX_W = QWinFuzzModel::Cfg::QCAP - 1;

struct QueueWinFuzzOut {
    std::vector<uint64_t> gets;  // every get's value, in order
    std::vector<int32_t> lens;   // queue length after each op
    int32_t status = 0;          // engine status at the end
    int32_t window = 0;          // the engine's effective W
    // how often the sequence reached each case a window of count_w
    // entries must survive
    uint64_t win_put = 0;       // put into a window position
    uint64_t ring_put = 0;      // put that goes to the ring, window full
    uint64_t tail_load = 0;     // get that pulls a ring entry into the tail
    uint64_t short_get = 0;     // get that leaves len < W: no load
    uint64_t tail_wrap = 0;     // tail load whose ring index wrapped
    uint64_t refill_out = 0;    // spill-refilled entry that entered the
                                // window through the tail and was returned
    uint64_t drain_put = 0;     // put into a queue that gets had emptied
    uint64_t queue_full = 0;    // put refused with ST_QUEUE_FULL at 16 queued
    uint64_t reinit_win = 0;    // init() with the window full
    uint64_t reinit_ring = 0;   // init() with entries beyond it in the ring
};

template <class Tier>
inline QueueWinFuzzOut queue_window_fuzz(uint64_t seed, uint64_t nops,
                                         int count_w) {
    using Eng = Engine<QWinFuzzModel, Tier>;
    constexpr int QCAP = QWinFuzzModel::Cfg::QCAP;
    constexpr int TOTAL = QCAP + QWinFuzzModel::Cfg::SPILL_Q;
    const int W = count_w;
    auto store = std::make_unique<typename Eng::Storage>();
    auto slab = std::make_unique<typename Eng::Spill>();
    auto eng = std::make_unique<Eng>(*store);
    Eng& E = *eng;
    const QWinFuzzModel::Params P{};
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
    QueueWinFuzzOut o;
    o.window = Eng::QWIN;
    // shadow of the ring's logical positions (the spill segment is not
    // in it): bit 0 = written by a spill refill, bit 1 = and then pulled
    // into the window through the tail load
    std::deque<uint8_t> shadow;
    bool emptied = false;  // the last successful op was a draining get
    uint32_t trial = 0;
    for (uint64_t op = 0; op < nops; ++op) {
        const uint64_t r = rnd();
        auto& q = E.queues[0];
        // alternate 64-op phases that fill the queue (to the 16th entry
        // and one put beyond) and drain it (to empty)
        const int nput = ((op >> 6) & 1) ? 5 : 11;
        const int what = (int)(r % 16);
        if ((r >> 8) % 251 == 0 && Eng::q_len(q) > 0) {
            // a lane's next trial: whatever is queued is abandoned
            if (q.len >= W) ++o.reinit_win;
            if (q.len > W) ++o.reinit_ring;
            start_trial(++trial);
            shadow.clear();
            emptied = false;
        } else if (what < nput) {
            const int32_t before = Eng::q_len(q);
            const bool ring = q.len < QCAP && q.sp_len == 0;
            const int32_t pos = q.len;
            const bool ok = E.q_try_put(0, E.procs[0], r | 1u);
            if (ok && before == 0 && emptied) ++o.drain_put;
            if (ok && ring) {
                shadow.push_back(0);
                if (pos < W) ++o.win_put;
                else ++o.ring_put;
            }
            if (!ok && before == TOTAL && E.status == ST_QUEUE_FULL)
                ++o.queue_full;
            if (ok) emptied = false;
        } else {
            const bool spilling = q.sp_len > 0;
            uint64_t v = 0;
            if (E.q_try_get(0, E.procs[0], &v)) {
                o.gets.push_back(v);
                if (shadow.front() == 3) ++o.refill_out;
                shadow.pop_front();
                // a spilling queue has a full ring: the refill goes to
                // the last logical position
                if (spilling) shadow.push_back(1);
                if (W > 0 && q.len >= W) {
                    ++o.tail_load;
                    if (q.head + W - 1 >= QCAP) ++o.tail_wrap;
                    if (shadow[W - 1] & 1) shadow[W - 1] |= 2;
                } else {
                    ++o.short_get;
                }
                emptied = Eng::q_len(q) == 0;
            }
        }
        o.lens.push_back(Eng::q_len(E.queues[0]));
    }
    o.status = E.status;
    return o;
}

// window width w in [0, QWIN_FUZZ_MAX_W]; the counts are those of a
// window of count_w entries (pass w itself for a windowed flavour)
inline QueueWinFuzzOut queue_window_fuzz_n(uint64_t seed, uint64_t nops,
                                           int w, int count_w) {
    switch (w) {
        case 0: return queue_window_fuzz<FlatTier>(seed, nops, count_w);
        case 1: return queue_window_fuzz<FlatWindowTier<1>>(seed, nops, count_w);
        case 2: return queue_window_fuzz<FlatWindowTier<2>>(seed, nops, count_w);
        case 3: return queue_window_fuzz<FlatWindowTier<3>>(seed, nops, count_w);
        case 4: return queue_window_fuzz<FlatWindowTier<4>>(seed, nops, count_w);
        case 5: return queue_window_fuzz<FlatWindowTier<5>>(seed, nops, count_w);
        case 6: return queue_window_fuzz<FlatWindowTier<6>>(seed, nops, count_w);
        // anything wider is clamped to QCAP - 1 by QWinOf
        default: return queue_window_fuzz<FlatWindowTier<64>>(seed, nops, count_w);
    }
}

}  // namespace cmb
