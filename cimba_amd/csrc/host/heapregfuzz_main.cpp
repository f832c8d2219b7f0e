// Stand-alone lockstep fuzzer for the event heap's register tier
// (hashheap.hpp, R = min(HOT, HotTier::EVREG)), meant to be built with
// -fsanitize=address,undefined:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -Icimba_amd/csrc/include cimba_amd/csrc/host/heapregfuzz_main.cpp
//       -o heapregfuzz && ./heapregfuzz
//
// One seeded push / pop / cancel / reschedule / pattern_cancel sequence is
// applied to two heaps at once: HashHeap<16, SCAP, false, HOT, FlatTier>
// and the same heap with its first R entries in the view.  After every
// operation the two must agree in n, top(), every at(i) and whatever the
// operation returned.  Every tier is an exact-size heap allocation (the
// hot array of the register flavour has HOT - R entries, none at all when
// R == HOT), so an index that strays across a boundary is an out-of-bounds
// access the sanitizer sees.  The deep phases (the first `nops` operations)
// fill the heap to capacity and drain it to empty, so sifts cross register
// -> hot array -> cold -> spill at every depth.  The shallow phase (as many
// operations again) keeps the heap between empty and R + 1 entries, where
// push and pop take the register-only paths (hashheap.hpp reg_push and
// pop) and leave them again one entry later; its times, priorities and
// sequence numbers come from two values each, so entries that tie in t, in
// (t, priority) and in the whole key meet all the time.  Exit status 0 =
// all equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cimba/hashheap.hpp"

namespace {

constexpr int CAP = 16;

template <int HOT, int SCAP, class Tier>
struct Rig {
    using Heap = cmb::HashHeap<CAP, SCAP, false, HOT, Tier>;
    std::unique_ptr<cmb::EvEntry[]> cold{new cmb::EvEntry[CAP - HOT]};
    std::unique_ptr<cmb::EvEntry[]> hot{
        Heap::HOT_MEM > 0 ? new cmb::EvEntry[Heap::HOT_MEM] : nullptr};
    std::unique_ptr<cmb::EvEntry[]> spill{
        SCAP > 0 ? new cmb::EvEntry[SCAP] : nullptr};
    Heap hp;
    Rig()
        : hp(*reinterpret_cast<cmb::EvEntry(*)[CAP - HOT]>(cold.get()),
             hot.get()) {
        hp.reset();
        if (SCAP > 0) hp.attach_spill(spill.get(), SCAP);
    }
};

bool same(const cmb::EvEntry& x, const cmb::EvEntry& y) {
    return x.t == y.t && x.pseq == y.pseq && x.b == y.b &&
           x.handle == y.handle && x.kind == y.kind && x.a == y.a &&
           x.c == y.c;
}

template <int HOT, int R, int SCAP>
int fuzz(uint64_t seed, uint64_t nops) {
    Rig<HOT, SCAP, cmb::FlatTier> ref;
    Rig<HOT, SCAP, cmb::FlatEvRegTier<R>> reg;
    static_assert(decltype(ref)::Heap::R == 0, "reference has no register tier");
    static_assert(decltype(reg)::Heap::R == R, "register tier size");
    static_assert(decltype(reg)::Heap::HOT_MEM == HOT - R, "hot array size");

    uint64_t x = seed;
    auto rnd = [&x]() {  // splitmix64
        uint64_t z = (x += UINT64_C(0x9E3779B97F4A7C15));
        z = (z ^ (z >> 30)) * UINT64_C(0xBF58476D1CE4E5B9);
        z = (z ^ (z >> 27)) * UINT64_C(0x94D049BB133111EB);
        return z ^ (z >> 31);
    };
    uint64_t seq = 0, pops = 0, maxn = 0;
    // shallow phase: operations that began at n <= R + 1, pushes that began
    // at n < R, pops that began at n <= R, pushes of a key already present
    uint64_t sh_ops = 0, sh_low = 0, sh_push = 0, sh_pop = 0, sh_tie = 0;
    uint32_t next_handle = 1;
    double now = 0.0;
    int bad = 0;
    auto check = [&](uint64_t op, const char* what) {
        bool ok = ref.hp.n == reg.hp.n && ref.hp.empty() == reg.hp.empty() &&
                  ref.hp.full() == reg.hp.full();
        if (ok && ref.hp.n > 0) ok = same(ref.hp.top(), reg.hp.top());
        for (int32_t i = 0; ok && i < ref.hp.n; ++i)
            ok = same(ref.hp.at(i), reg.hp.at(i));
        if (!ok && bad++ < 5)
            std::fprintf(stderr, "HOT %d R %d SCAP %d seed %llu: op %llu (%s) "
                         "differs, n %d / %d\n", HOT, R, SCAP,
                         (unsigned long long)seed, (unsigned long long)op,
                         what, ref.hp.n, reg.hp.n);
    };
    // a live handle picked by heap position, the same in both heaps
    auto pick = [&](uint64_t r) {
        return ref.hp.at((int32_t)((r >> 20) % (uint64_t)ref.hp.n)).handle;
    };
    for (uint64_t op = 0; op < 2 * nops; ++op) {
        const uint64_t r = rnd();
        const bool shallow = op >= nops;
        const int32_t n0 = ref.hp.n;
        // deep: alternate 512-op phases that fill the heap (to capacity)
        // and drain it (to empty).  shallow: 32-op phases that lean up and
        // down, and hardly a push once the heap has left the registers
        const int npush = !shallow          ? (((op >> 9) & 1) ? 3 : 9)
                          : n0 > R          ? 1
                          : ((op >> 5) & 1) ? 8
                                            : 3;
        // whatever the deep phase left is popped first
        const int what = shallow && n0 > R + 2 ? npush : (int)(r % 16);
        // times on a coarse grid so (t, priority, seq) ties all occur
        const double t = now + (double)((r >> 8) % (shallow ? 2 : 6)) * 0.5;
        const int prio = (int)((r >> 16) % (shallow ? 2 : 3));
        if (shallow) {
            ++sh_ops;
            if (n0 <= R + 1) ++sh_low;
        }
        if (what < npush) {
            cmb::EvEntry ev{};
            ev.t = t;
            // shallow: one of two sequence numbers, so whole keys repeat
            ev.pseq = cmb::ev_pseq(prio, shallow ? (r >> 12) % 2 : seq++);
            if (shallow) {
                if (n0 < R) ++sh_push;
                for (int32_t i = 0; i < n0; ++i)
                    if (ref.hp.at(i).t == ev.t && ref.hp.at(i).pseq == ev.pseq) {
                        ++sh_tie;
                        break;
                    }
            }
            ev.b = (r >> 32) % 3;
            ev.handle = next_handle++;
            ev.kind = (uint16_t)((r >> 24) % 4);
            ev.a = (uint16_t)((r >> 40) % 3);
            ev.c = (uint32_t)(r >> 44);
            const bool p0 = ref.hp.push(ev), p1 = reg.hp.push(ev);
            if (p0 != p1) ++bad;
            check(op, "push");
        } else if (what < npush + 3) {
            if (ref.hp.empty()) continue;
            const cmb::EvEntry e0 = ref.hp.pop(), e1 = reg.hp.pop();
            if (!same(e0, e1)) ++bad;
            now = e0.t;
            ++pops;
            if (shallow && n0 <= R) ++sh_pop;
            check(op, "pop");
        } else if (what < npush + 4) {
            if (ref.hp.empty()) continue;
            const uint32_t h = pick(r);
            cmb::EvEntry o0{}, o1{};
            const bool c0 = ref.hp.cancel(h, &o0), c1 = reg.hp.cancel(h, &o1);
            if (c0 != c1 || !same(o0, o1)) ++bad;
            // a handle that is gone: both must say so
            if (ref.hp.cancel(h) || reg.hp.cancel(h)) ++bad;
            check(op, "cancel");
        } else if (what < npush + 6) {
            if (ref.hp.empty()) continue;
            const uint32_t h = pick(r);
            const uint64_t ps =
                cmb::ev_pseq(prio, shallow ? (r >> 12) % 2 : seq++);
            if (ref.hp.find_index(h) != reg.hp.find_index(h)) ++bad;
            const bool r0 = ref.hp.reschedule(h, t, ps);
            const bool r1 = reg.hp.reschedule(h, t, ps);
            if (r0 != r1) ++bad;
            check(op, "reschedule");
        } else {
            // wildcard or exact (kind, a, b) pattern
            const uint16_t kind = (r >> 50) & 1 ? 0xFFFF : (uint16_t)((r >> 24) % 4);
            const uint16_t a = (r >> 51) & 1 ? 0xFFFF : (uint16_t)((r >> 40) % 3);
            const bool mb = (r >> 52) & 1;
            const uint64_t b = (r >> 32) % 3;
            if (ref.hp.pattern_count(kind, a, mb, b) !=
                reg.hp.pattern_count(kind, a, mb, b))
                ++bad;
            if (ref.hp.pattern_find(kind, a, mb, b) !=
                reg.hp.pattern_find(kind, a, mb, b))
                ++bad;
            // cancel by pattern only now and then, or the heap never fills
            if (((r >> 53) & 3) == 0) {
                if (ref.hp.pattern_cancel(kind, a, mb, b) !=
                    reg.hp.pattern_cancel(kind, a, mb, b))
                    ++bad;
            }
            check(op, "pattern");
        }
        if ((uint64_t)ref.hp.n > maxn) maxn = (uint64_t)ref.hp.n;
    }
    while (!ref.hp.empty()) {
        if (!same(ref.hp.pop(), reg.hp.pop())) ++bad;
        ++pops;
        check(2 * nops, "drain");
    }
    if (!reg.hp.empty()) ++bad;
    std::printf("HOT %d R %d SCAP %d seed %llu: %llu ops, %llu pops, "
                "deepest %llu of %d; shallow: %llu of %llu ops at n <= R + 1, "
                "%llu pushes at n < R, %llu pops at n <= R, %llu tied pushes: "
                "%s\n", HOT, R, SCAP,
                (unsigned long long)seed, (unsigned long long)(2 * nops),
                (unsigned long long)pops, (unsigned long long)maxn,
                CAP + SCAP, (unsigned long long)sh_low,
                (unsigned long long)sh_ops, (unsigned long long)sh_push,
                (unsigned long long)sh_pop, (unsigned long long)sh_tie,
                bad ? "DIFFER" : "equal");
    // every depth from empty to full must have been visited
    if (maxn != (uint64_t)(CAP + SCAP)) {
        std::fprintf(stderr, "heap never filled\n");
        ++bad;
    }
    // the shallow phase must have stayed shallow and used both short paths
    if (2 * sh_low < sh_ops || sh_push == 0 || sh_pop == 0 || sh_tie == 0) {
        std::fprintf(stderr, "shallow phase missed its depths\n");
        ++bad;
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t nops = argc > 1 ? strtoull(argv[1], nullptr, 0) : 20000;
    int bad = 0;
    for (uint64_t seed : {UINT64_C(1), UINT64_C(2), UINT64_C(0xDEADBEEF)}) {
        bad += fuzz<2, 2, 0>(seed, nops);
        bad += fuzz<1, 1, 0>(seed, nops);
        bad += fuzz<4, 2, 0>(seed, nops);
        bad += fuzz<4, 2, 8>(seed, nops);
        bad += fuzz<2, 2, 8>(seed, nops);
        // no flavour has R > 2 today; reg_push is written for any R
        bad += fuzz<4, 3, 0>(seed, nops);
        bad += fuzz<6, 5, 8>(seed, nops);
    }
    return bad ? 1 : 0;
}
