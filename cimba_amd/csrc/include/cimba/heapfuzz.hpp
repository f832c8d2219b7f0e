// Seeded random driver for the event heap's hot tier (hashheap.hpp):
// one push/pop/cancel/reschedule sequence, a pure function of (seed,
// nops), run against HashHeap<16> with HOT leading entries in a separate
// array.  The pop sequence must not depend on HOT.  Host only; shared by
// the Python binding (_C.hashheap_tier_fuzz) and the stand-alone
// sanitizer program (host/heapfuzz_main.cpp).  Both tiers are exact-size
// heap allocations, so an index that strays across the boundary is an
// out-of-bounds access a sanitizer sees.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "hashheap.hpp"

namespace cmb {

struct HeapFuzzPop {
    double t;
    uint64_t pseq;
    uint32_t handle;
};

template <int HOT>
inline std::vector<HeapFuzzPop> heap_tier_fuzz(uint64_t seed, uint64_t nops) {
    constexpr int CAP = 16;
    using Heap = HashHeap<CAP, 0, false, HOT>;
    std::unique_ptr<EvEntry[]> cold(new EvEntry[CAP - HOT]);
    std::unique_ptr<EvEntry[]> hot(HOT > 0 ? new EvEntry[HOT] : nullptr);
    Heap hp(*reinterpret_cast<EvEntry(*)[CAP - HOT]>(cold.get()), hot.get());
    hp.reset();

    uint64_t x = seed;
    auto rnd = [&x]() {  // splitmix64
        uint64_t z = (x += UINT64_C(0x9E3779B97F4A7C15));
        z = (z ^ (z >> 30)) * UINT64_C(0xBF58476D1CE4E5B9);
        z = (z ^ (z >> 27)) * UINT64_C(0x94D049BB133111EB);
        return z ^ (z >> 31);
    };
    std::vector<uint32_t> live;
    std::vector<HeapFuzzPop> pops;
    uint64_t seq = 0;
    uint32_t next_handle = 1;
    double now = 0.0;
    auto forget = [&live](uint32_t h) {
        for (size_t i = 0; i < live.size(); ++i)
            if (live[i] == h) {
                live[i] = live.back();
                live.pop_back();
                return;
            }
    };
    auto pop_one = [&]() {
        const EvEntry ev = hp.pop();
        now = ev.t;
        forget(ev.handle);
        pops.push_back({ev.t, ev.pseq, ev.handle});
    };
    for (uint64_t op = 0; op < nops; ++op) {
        const uint64_t r = rnd();
        // alternate 512-op phases that fill the heap (to capacity) and
        // drain it (to empty), so every depth on both sides of the tier
        // boundary is visited again and again
        const int npush = ((op >> 9) & 1) ? 4 : 9;
        const int what = (int)(r % 16);
        // times on a coarse grid so (t, priority, seq) ties all occur
        const double t = now + (double)((r >> 8) % 6) * 0.5;
        const int prio = (int)((r >> 16) % 3);
        if (what < npush) {  // push
            if (hp.full()) continue;
            EvEntry ev{};
            ev.t = t;
            ev.pseq = ev_pseq(prio, seq++);
            ev.b = r;
            ev.handle = next_handle++;
            ev.kind = (uint16_t)(r >> 24);
            ev.a = (uint16_t)(r >> 40);
            hp.push(ev);
            live.push_back(ev.handle);
        } else if (what < npush + 3) {  // pop
            if (!hp.empty()) pop_one();
        } else if (what < npush + 5) {  // cancel a live event
            if (live.empty()) continue;
            const uint32_t h = live[(r >> 20) % live.size()];
            if (hp.cancel(h)) forget(h);
        } else {  // reschedule a live event
            if (live.empty()) continue;
            const uint32_t h = live[(r >> 20) % live.size()];
            hp.reschedule(h, t, ev_pseq(prio, seq++));
        }
    }
    while (!hp.empty()) pop_one();
    return pops;
}

// run-time `hot` in {0, 1, 2, 4}; anything else returns an empty sequence
inline std::vector<HeapFuzzPop> heap_tier_fuzz_n(uint64_t seed, uint64_t nops,
                                                 int hot) {
    switch (hot) {
        case 0: return heap_tier_fuzz<0>(seed, nops);
        case 1: return heap_tier_fuzz<1>(seed, nops);
        case 2: return heap_tier_fuzz<2>(seed, nops);
        case 4: return heap_tier_fuzz<4>(seed, nops);
    }
    return {};
}

}  // namespace cmb
