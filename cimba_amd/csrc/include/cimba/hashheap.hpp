// cimba_amd future-event list: fixed-capacity binary min-heap keyed by
// (time asc, priority desc, FIFO seq asc), with O(1)-amortized cancel by
// handle through a slot back-map.
//
// Counterpart of reference src/cmi_hashheap.c (binary min-heap + open
// addressing hash map in one allocation, pattern find/count/cancel,
// cmi_hashheap.h:335-357).  Redesigned for gfx950: the reference needs a
// hash map because its 64-bit handles are opaque; here the heap lives in
// LDS with a bounded capacity, so a handle is (slot-generation, pool index)
// and cancellation resolves by a direct scan over a small heap — no hash
// map, no tombstones, no growth path in the hot loop.  Host-side large
// models use the same structure with a bigger CAP (heap-allocated engine).
#pragma once

#include <type_traits>

#include "config.hpp"

namespace cmb {

// Event payload carried inline in the heap (reference keeps 4 pointers;
// we keep {kind, a, c, b} — kind = action id, a = subject (proc index or
// similar), c = auxiliary u32 (guard id / timer slot), b = 64-bit payload
// (signal value, object word)).
struct EvEntry {
    // NOTE: a "peek-hot head first" reorder ({t, kind, a, handle} in the
    // leading 16 B) was measured 2-4% SLOWER across all three lane
    // models: with the heap-top register cache a peek costs no memory at
    // all, and splitting the (t, pseq) comparator pair across chunks
    // taxes every sift compare instead.  Comparator-pair-first stays.
    double t;        // activation time
    uint64_t pseq;   // (INT16_MAX - priority) << 48 | seq  → min == next
    uint64_t b;      // payload
    uint32_t handle; // unique id for cancel/reschedule
    uint16_t kind;
    uint16_t a;
    uint32_t c;
    uint32_t pad_;
};

CMB_FORCEINLINE uint64_t ev_pseq(int priority, uint64_t seq) {
    const uint16_t k = (uint16_t)(32767 - priority);
    return ((uint64_t)k << 48) | (seq & UINT64_C(0xFFFFFFFFFFFF));
}

// lexicographic (t, pseq): earlier time first; at equal time higher
// priority first, then FIFO (same comparator contract as reference
// cmb_event.c:78-103)
CMB_FORCEINLINE bool ev_less(const EvEntry& x, const EvEntry& y) {
    if (x.t != y.t) return x.t < y.t;
    return x.pseq < y.pseq;
}

// The heap is a VIEW: `e` references a caller-owned entry array (LDS or
// HBM) while the size `n` lives in the view itself — on the device the
// view is part of the register-resident Engine context, so the hot-loop
// size checks and the count never round-trip through LDS.
//
// SCAP > 0 enables a SECOND TIER: entries [CAP, CAP+cap2) live in a
// spill buffer (HBM slab on the device, heap memory on the host) that
// the engine attaches on first overflow — the MI355X counterpart of the
// reference's unbounded doubling growth (cmi_hashheap.c:380-432).  The
// heap is index-contiguous across the tiers, so deep (cold) entries
// land in the slow tier naturally while the hot top stays fast.  With
// SCAP == 0 every access compiles to the plain fast-tier load — zero
// cost for models that never spill.
// MAP enables the handle->index BACK-MAP (reference cmi_hashheap.c
// open-addressing contract, :89-120): cancel/reschedule/find become an
// O(1) hash lookup + O(log n) sift instead of an O(n) scan.  Meant for
// the host C API configuration (MAX_EV 16384+); device models keep
// MAP=false and the O(small-n) scan, which wins at LDS heap sizes.
// Open addressing, linear probing, backward-shift deletion, fixed <=50%
// load (map is 2x total heap capacity, power of two).
struct EvMapSlot {
    uint32_t key;  // event handle; 0 = empty (handles start at 1)
    int32_t idx;   // heap index
};

constexpr int32_t cmb_pow2_atleast(int32_t v) {
    int32_t p = 2;
    while (p < v) p <<= 1;
    return p;
}

// HOT > 0 adds a HOT TIER in front, the mirror image of the spill tier:
// heap indices [0, HOT) live in a second caller-owned array `hot_e` (the
// per-lane LDS slice of conv_lds_kernel) and [HOT, CAP) in `e`.  The top
// of a binary heap is where every pop and almost every push works, so a
// few hot entries keep the whole sift out of far memory for models whose
// event list stays short.  Entries move between tiers BY VALUE (get/put,
// never a reference chosen at run time).  With HOT == 0 the tier
// compiles out.
//
// HotTier names the memory the hot array is in.  FlatTier is a plain
// pointer, good anywhere.  LdsTier is an LDS-qualified pointer for
// kernels that keep the hot array in LDS: without the qualifier both
// tiers are generic pointers by the time the optimizer sees get(i), it
// folds the two loads into ONE load through a run-time-selected pointer,
// and the whole heap compiles to flat_load/flat_store (seen in the
// gfx950 ISA: 2377 flat ops against 863 ds).  Loads through pointers of
// different address-space TYPES cannot be folded, so each tier keeps its
// own instruction kind.
//
// A tier tag also says how many leading entries of every object queue the
// engine keeps in registers (QWIN, engine.hpp QWindowState; 0 = none, the
// ring alone).  It is a property of the engine flavour, not of the model:
// the LDS kernel has the registers for it, the kernels under a tight VGPR
// cap do not pay for it.  A model may lower it (Cfg::QWIN_MAX) and the
// ring geometry bounds it (engine.hpp QWinOf).  FlatWindowTier<W> is
// FlatTier plus a W-entry window, for host tests of the windowed code
// path; FlatFrontTier is its one-entry case.
// M/M/1: 4 < 8 = 16 in events/s, and 16 costs M/G/1 its second wave per
// SIMD (profiles/r12_queue_window.md)
//
// SPLIT says whether the engine flavour defers an exponential hold from
// the process body to Engine::dispatch_tail() (engine.hpp HoldDeferState,
// CMB_HOLD_EXP), so that a lane kernel can run the draw and the timer
// push once, converged, after the divergent bodies.  The plain tags leave
// it off and compile as they always did; LdsSplitTier is LdsTier with it
// on (the fused loop of conv_lds_kernel), FlatSplitTier the host flavour
// for CPU tests of that code path.
//
// EVREG says how many leading heap entries the flavour keeps in the heap
// view itself, i.e. in registers on the device (HashHeap's register tier,
// R = min(HOT, EVREG) below).  Those entries leave the hot array, so the
// flavour's Engine::Hot is smaller by R entries (engine.hpp EngineTypes).
// 0 on the plain tags.  LdsRegTier is LdsSplitTier with EVREG = 2 (lane
// mode 6 of conv_lds_kernel's family, conv_lds_regheap_kernel),
// FlatRegTier the host flavour for CPU tests of that code path.
constexpr int LDS_QWIN = 8;
constexpr int LDS_EVREG = 2;
struct FlatTier {
    template <class T>
    using ptr = T*;
    static constexpr int QWIN = 0;
    static constexpr bool SPLIT = false;
    static constexpr int EVREG = 0;
};
template <int W>
struct FlatWindowTier {
    template <class T>
    using ptr = T*;
    static constexpr int QWIN = W;
    static constexpr bool SPLIT = false;
    static constexpr int EVREG = 0;
};
using FlatFrontTier = FlatWindowTier<1>;
struct FlatSplitTier : FlatTier {
    static constexpr bool SPLIT = true;
};
struct FlatRegTier : FlatSplitTier {
    static constexpr int EVREG = LDS_EVREG;
};
// FlatTier with the first N heap entries in the view and nothing else
// changed: the lockstep fuzzer's flavour (host/heapregfuzz_main.cpp)
template <int N>
struct FlatEvRegTier : FlatTier {
    static constexpr int EVREG = N;
};
#if defined(__HIP_DEVICE_COMPILE__)
struct LdsTier {
    template <class T>
    using ptr = __attribute__((address_space(3))) T*;
    static constexpr int QWIN = LDS_QWIN;
    static constexpr bool SPLIT = false;
    static constexpr int EVREG = 0;
};
#else
struct LdsTier {  // host pass of a kernel TU: never executed
    template <class T>
    using ptr = T*;
    static constexpr int QWIN = LDS_QWIN;
    static constexpr bool SPLIT = false;
    static constexpr int EVREG = 0;
};
#endif
struct LdsSplitTier : LdsTier {
    static constexpr bool SPLIT = true;
};
struct LdsRegTier : LdsSplitTier {
    static constexpr int EVREG = LDS_EVREG;
};

template <int CAP, int SCAP = 0, bool MAP = false, int HOT = 0,
          class HotTier = FlatTier>
struct HashHeap {
    using HotPtr = typename HotTier::template ptr<EvEntry>;
    static_assert(HOT >= 0 && HOT < CAP, "hot tier must leave a cold tier");
    static constexpr int32_t MSIZE =
        MAP ? cmb_pow2_atleast(2 * (CAP + SCAP)) : 2;
    // REGISTER TIER: heap indices [0, R) live in the view itself (rg[]),
    // the hot array holds [R, HOT).  Index i is the same binary-heap
    // position whatever R is, only its storage differs, so the pop order,
    // find_index, the pattern operations, remove_at and reschedule do not
    // depend on R.  rg[] is only ever indexed with compile-time constants
    // (reg_get / reg_put are select chains): a run-time index would send
    // the whole array to scratch on the device.  A chain costs ten
    // v_cndmask per entry and select, so push() and pop() do without one
    // while the heap lies wholly in rg[] (reg_push and the short pop
    // below); the generic sifts behind them run only once the heap has
    // outgrown the registers (profiles/r19_reg_sifts.md).
    static constexpr int R = HOT < HotTier::EVREG ? HOT : HotTier::EVREG;
    static constexpr int HOT_MEM = HOT - R;  // entries of the hot array
    static_assert(R >= 0, "register tier");

    EvEntry (&e)[CAP - HOT];
    HotPtr hot_e;    // hot tier base (HOT_MEM entries; null when none)
    EvEntry* e2;     // spill tier base (null until attached)
    EvMapSlot* map;  // back-map slots (storage-owned when MAP)
    int32_t cap2;    // usable spill entries (0 until attached)
    int32_t n;
    // R == 0: rg[0] is a register-cached copy of entry 0 (valid while
    // n > 0): the heap top is read by every peek and every pop — the
    // hottest dependent load in the dispatch chain — and every mutation
    // flows through place(), so the cache is maintained by construction.
    // R > 0: rg[0..R) ARE entries 0..R-1, and the top needs no copy.
    EvEntry rg[R > 0 ? R : 1];

    CMB_FORCEINLINE explicit HashHeap(EvEntry (&buf)[CAP - HOT],
                                      EvEntry* hot = nullptr)
        : e(buf), hot_e((HotPtr)hot), e2(nullptr), map(nullptr), cap2(0),
          n(0) {
        // entries at or past n are dead, but a select chain reads them all:
        // start them defined, once per engine
        if constexpr (R > 0) reg_clear();
    }

    template <int K = 0>
    CMB_FORCEINLINE void reg_clear() {
        rg[K] = EvEntry{};
        if constexpr (K + 1 < R) reg_clear<K + 1>();
    }
    // c ? x : y, field by field on scalars.  Whole-struct forms (`c ? x : y`
    // on two lvalues, or `if (c) r = x; else r = y;`) reach the optimizer
    // as ONE struct copy through a run-time-selected pointer, and a pointer
    // into the view chosen at run time keeps the whole engine context out
    // of registers (seen in the gfx950 ISA: every LDS access of the kernel
    // turned into a flat one, and the context went to scratch)
    static CMB_FORCEINLINE EvEntry ev_select(bool c, const EvEntry& x,
                                             const EvEntry& y) {
        const double xt = x.t, yt = y.t;
        const uint64_t xp = x.pseq, yp = y.pseq, xb = x.b, yb = y.b;
        const uint32_t xh = x.handle, yh = y.handle, xc = x.c, yc = y.c;
        const uint16_t xk = x.kind, yk = y.kind, xa = x.a, ya = y.a;
        EvEntry r;
        r.t = c ? xt : yt;
        r.pseq = c ? xp : yp;
        r.b = c ? xb : yb;
        r.handle = c ? xh : yh;
        r.kind = c ? xk : yk;
        r.a = c ? xa : ya;
        r.c = c ? xc : yc;
        r.pad_ = 0;
        return r;
    }
    // register-tier entry i < R, by select chain over constant indices
    template <int K = 0>
    CMB_FORCEINLINE EvEntry reg_get(int32_t i) const {
        if constexpr (K + 1 >= R) {
            (void)i;
            return rg[K];
        } else {
            return ev_select(i == K, rg[K], reg_get<K + 1>(i));
        }
    }
    // every register is rewritten, with `ev` where i names it and with
    // itself elsewhere: no store whose address depends on i
    template <int K = 0>
    CMB_FORCEINLINE void reg_put(int32_t i, const EvEntry& ev) {
        if constexpr (R == 1) {
            (void)i;
            rg[0] = ev;
        } else {
            rg[K] = ev_select(i == K, ev, rg[K]);
            if constexpr (K + 1 < R) reg_put<K + 1>(i, ev);
        }
    }

    // ---- back-map primitives (compiled out when !MAP) ----
    static CMB_FORCEINLINE uint32_t mhash(uint32_t h) {
        if constexpr (!MAP) return 0;
        return (h * 2654435769u) >> (32 - __builtin_ctz((uint32_t)MSIZE));
    }
    CMB_FORCEINLINE void map_clear() {
        if constexpr (MAP) {
            for (int32_t i = 0; i < MSIZE; ++i) map[i].key = 0;
        }
    }
    CMB_FORCEINLINE void map_set(uint32_t key, int32_t idx) {
        if constexpr (MAP) {
            uint32_t i = mhash(key);
            for (;;) {
                if (map[i].key == key || map[i].key == 0) {
                    map[i].key = key;
                    map[i].idx = idx;
                    return;
                }
                i = (i + 1) & (MSIZE - 1);
            }
        }
    }
    CMB_FORCEINLINE int32_t map_get(uint32_t key) const {
        if constexpr (!MAP) return -1;
        uint32_t i = mhash(key);
        for (;;) {
            if (map[i].key == key) return map[i].idx;
            if (map[i].key == 0) return -1;
            i = (i + 1) & (MSIZE - 1);
        }
    }
    CMB_FORCEINLINE void map_erase(uint32_t key) {
        if constexpr (MAP) {
            uint32_t i = mhash(key);
            for (;;) {
                if (map[i].key == key) break;
                if (map[i].key == 0) return;
                i = (i + 1) & (MSIZE - 1);
            }
            // backward-shift deletion keeps probe chains intact with no
            // tombstones, so no compaction pass is ever needed
            uint32_t j = i;
            for (;;) {
                map[i].key = 0;
                for (;;) {
                    j = (j + 1) & (MSIZE - 1);
                    if (map[j].key == 0) return;
                    const uint32_t h = mhash(map[j].key);
                    if (i <= j ? (h <= i || h > j) : (h <= i && h > j))
                        break;
                }
                map[i] = map[j];
                i = j;
            }
        }
    }

    // placement: every heap move goes through here so the map AND the
    // top cache track it
    CMB_FORCEINLINE void place(int32_t i, const EvEntry& ev) {
        put(i, ev);
        if constexpr (R == 0) {
            if (i == 0) rg[0] = ev;
        }
        map_set(ev.handle, i);
    }

    // hot-tier entry i.  A plain pointer copies the struct, exactly as the
    // other tiers do; an LDS-qualified one cannot bind to EvEntry's copy
    // operations, so it goes field by field (the compiler still merges
    // the fields into wide ds_read/ds_write)
    CMB_FORCEINLINE EvEntry hot_get(int32_t i) const {
        if constexpr (std::is_same<HotPtr, EvEntry*>::value) {
            return hot_e[i];
        } else {
            const HotPtr p = hot_e + i;
            EvEntry r;
            r.t = p->t;
            r.pseq = p->pseq;
            r.b = p->b;
            r.handle = p->handle;
            r.kind = p->kind;
            r.a = p->a;
            r.c = p->c;
            r.pad_ = 0;
            return r;
        }
    }
    CMB_FORCEINLINE void hot_put(int32_t i, const EvEntry& ev) {
        if constexpr (std::is_same<HotPtr, EvEntry*>::value) {
            hot_e[i] = ev;
        } else {
            const HotPtr p = hot_e + i;
            p->t = ev.t;
            p->pseq = ev.pseq;
            p->b = ev.b;
            p->handle = ev.handle;
            p->kind = ev.kind;
            p->a = ev.a;
            p->c = ev.c;
        }
    }

    // tiered entry access, by value: [0,R) registers, [R,HOT) hot,
    // [HOT,CAP) fast, [CAP, CAP+cap2) spill
    CMB_FORCEINLINE EvEntry get(int32_t i) const {
        if constexpr (R > 0) {
            if (i < R) return reg_get(i);
        }
        if constexpr (HOT_MEM > 0) {
            if (i < HOT) return hot_get(i - R);
        }
        if constexpr (SCAP > 0) {
            if (i >= CAP) return e2[i - CAP];
        }
        return e[i - HOT];
    }
    CMB_FORCEINLINE void put(int32_t i, const EvEntry& ev) {
        if constexpr (R > 0) {
            if (i < R) {
                reg_put(i, ev);
                return;
            }
        }
        if constexpr (HOT_MEM > 0) {
            if (i < HOT) {
                hot_put(i - R, ev);
                return;
            }
        }
        if constexpr (SCAP > 0) {
            if (i >= CAP) {
                e2[i - CAP] = ev;
                return;
            }
        }
        e[i - HOT] = ev;
    }
    // read-only view of entry i (const, so `at(i) = ev` cannot compile
    // and silently write a temporary; writes go through put/place)
    CMB_FORCEINLINE const EvEntry at(int32_t i) const { return get(i); }

    CMB_FORCEINLINE void attach_spill(EvEntry* buf, int32_t cap) {
        e2 = buf;
        cap2 = cap < SCAP ? cap : SCAP;
    }

    CMB_FORCEINLINE int32_t capacity() const {
        if constexpr (SCAP > 0) return CAP + cap2;
        else return CAP;
    }

    CMB_FORCEINLINE void reset() {
        n = 0;
        if (map) map_clear();
    }
    CMB_FORCEINLINE bool empty() const { return n == 0; }
    CMB_FORCEINLINE bool full() const { return n == capacity(); }
    CMB_FORCEINLINE const EvEntry& top() const { return rg[0]; }

    CMB_FORCEINLINE void sift_up(int32_t i) {
        const EvEntry tmp = get(i);
        while (i > 0) {
            const int32_t p = (i - 1) >> 1;
            const EvEntry par = get(p);
            if (!ev_less(tmp, par)) break;
            place(i, par);
            i = p;
        }
        place(i, tmp);
    }

    CMB_FORCEINLINE void sift_down(int32_t i) {
        const EvEntry tmp = get(i);
        for (;;) {
            int32_t c = 2 * i + 1;
            if (c >= n) break;
            EvEntry ch = get(c);
            if (c + 1 < n) {
                const EvEntry ch2 = get(c + 1);
                if (ev_less(ch2, ch)) {
                    ch = ch2;
                    ++c;
                }
            }
            if (!ev_less(ch, tmp)) break;
            place(i, ch);
            i = c;
        }
        place(i, tmp);
    }

    // ---- register-only sifts (R > 0) ----
    // A push into a heap of n < R entries and a pop from one of n <= R
    // touch rg[] alone, at indices known when the code is compiled, so they
    // need neither the get / put select chains nor a loop.  Both leave the
    // live entries exactly as sift_up / sift_down would, ties included (a
    // strict ev_less moves an entry, anything else stays put); entries at
    // or past n are dead and may differ.  They do not keep a back-map, and
    // no register flavour has one.  The pop is written out for R <= 2,
    // where the entry that moves up has no sibling to be compared with; a
    // larger R pops by the generic code.
    static constexpr bool REG_PUSH = R > 0 && !MAP;
    static constexpr bool REG_POP = R > 0 && R <= 2 && !MAP;

    // `ev` is on its way up and has reached index I if `mv`; P is I's parent
    template <int I>
    CMB_FORCEINLINE void reg_sift_up(const EvEntry& ev, bool mv) {
        if constexpr (I == 0) {
            rg[0] = ev_select(mv, ev, rg[0]);
        } else {
            constexpr int P = (I - 1) >> 1;
            const bool up = mv && ev_less(ev, rg[P]);
            rg[I] = ev_select(up, rg[P], ev_select(mv, ev, rg[I]));
            reg_sift_up<P>(ev, up);
        }
    }
    // n < R: enter the chain at index n
    template <int K = 0>
    CMB_FORCEINLINE void reg_push(const EvEntry& ev) {
        if constexpr (K + 1 < R) {
            if (n != K) {
                reg_push<K + 1>(ev);
                return;
            }
        }
        reg_sift_up<K>(ev, true);
    }

    // returns false when full (caller attaches spill or aborts the trial)
    CMB_FORCEINLINE bool push(const EvEntry& ev) {
        if constexpr (REG_PUSH) {
            if (__builtin_expect(n < R, 1)) {  // R < CAP: never full here
                reg_push(ev);
                ++n;
                return true;
            }
        }
        if (n == capacity()) return false;
        put(n, ev);
        sift_up(n);
        ++n;
        return true;
    }

    CMB_FORCEINLINE EvEntry pop() {
        EvEntry out = rg[0];
        map_erase(out.handle);
        --n;
        if constexpr (REG_POP) {
            if (__builtin_expect(n < R, 1)) {
                // the last entry, if there is a second one, is the new top
                if constexpr (R == 2) rg[0] = rg[1];
                return out;
            }
        }
        if (n > 0) {
            place(0, get(n));
            sift_down(0);
        }
        return out;
    }

    // find heap index by handle: O(1) with the back-map, O(n) scan else
    CMB_FORCEINLINE int32_t find_index(uint32_t handle) const {
        if constexpr (MAP) {
            const int32_t i = map_get(handle);
            return (i >= 0 && i < n) ? i : -1;
        }
        for (int32_t i = 0; i < n; ++i)
            if (at(i).handle == handle) return i;
        return -1;
    }

    CMB_FORCEINLINE bool cancel(uint32_t handle, EvEntry* out = nullptr) {
        const int32_t i = find_index(handle);
        if (i < 0) return false;
        if (out) *out = at(i);
        remove_at(i);
        return true;
    }

    CMB_FORCEINLINE void remove_at(int32_t i) {
        map_erase(at(i).handle);
        --n;
        if (i == n) return;
        place(i, get(n));
        sift_down(i);
        sift_up(i);
    }

    // reschedule (reference cmb_event_reschedule): new time, keep payload
    CMB_FORCEINLINE bool reschedule(uint32_t handle, double t, uint64_t pseq) {
        const int32_t i = find_index(handle);
        if (i < 0) return false;
        EvEntry ev = get(i);
        ev.t = t;
        ev.pseq = pseq;
        put(i, ev);
        sift_down(i);
        sift_up(i);
        return true;
    }

    // wildcard pattern ops over (kind, a, b) — reference
    // cmb_event_pattern_find/count/cancel (cmb_event.c:537-580) with
    // CMB_ANY_* wildcards.  kind == 0xFFFF / a == 0xFFFF / b-match disabled
    // via match_b=false act as wildcards.
    CMB_FORCEINLINE int32_t pattern_count(uint16_t kind, uint16_t a, bool match_b,
                                          uint64_t b) const {
        int32_t cnt = 0;
        for (int32_t i = 0; i < n; ++i) {
            if ((kind == 0xFFFF || at(i).kind == kind) &&
                (a == 0xFFFF || at(i).a == a) && (!match_b || at(i).b == b))
                ++cnt;
        }
        return cnt;
    }

    CMB_FORCEINLINE int32_t pattern_cancel(uint16_t kind, uint16_t a, bool match_b,
                                           uint64_t b) {
        // restart the scan after every removal: remove_at(i) refills slot i
        // with the last entry, and sift_up can carry that NOT-yet-examined
        // entry above i where a single ascending scan would never revisit
        // it (caught by the tests/test_hashheap.py fuzzer)
        int32_t cnt = 0;
        for (;;) {
            int32_t hit = -1;
            for (int32_t i = 0; i < n; ++i) {
                if ((kind == 0xFFFF || at(i).kind == kind) &&
                    (a == 0xFFFF || at(i).a == a) &&
                    (!match_b || at(i).b == b)) {
                    hit = i;
                    break;
                }
            }
            if (hit < 0) return cnt;
            remove_at(hit);
            ++cnt;
        }
    }

    CMB_FORCEINLINE uint32_t pattern_find(uint16_t kind, uint16_t a, bool match_b,
                                          uint64_t b) const {
        for (int32_t i = 0; i < n; ++i) {
            if ((kind == 0xFFFF || at(i).kind == kind) &&
                (a == 0xFFFF || at(i).a == a) && (!match_b || at(i).b == b))
                return at(i).handle;
        }
        return 0;  // 0 = no handle
    }
};

}  // namespace cmb
