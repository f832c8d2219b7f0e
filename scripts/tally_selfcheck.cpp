// Stand-alone host check of the device tally stream (engine + tally.hpp +
// the tallied M/M/1 model), meant to be built with sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -ffp-contract=off \
//       -Icimba_amd/csrc/include scripts/tally_selfcheck.cpp \
//       cimba_amd/csrc/host/support.cpp -lpthread -o tally_selfcheck
//
// Binds, adds and wraps the window on a host engine, checks the bin
// function's corners and runs the window check.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cimba/runner.hpp"
#include "../cimba_amd/csrc/models/mm1_tally.hpp"

using cmb::TallyRec;
using cmb::TallySink;
using cmb_models::MM1;
using cmb_models::MM1Tally;

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #x); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static_assert(std::is_empty<cmb::TallyState<0>>::value, "empty when off");
static_assert(sizeof(cmb::Engine<MM1Tally>::Storage) ==
                  sizeof(cmb::Engine<MM1>::Storage),
              "tallies add no per-trial storage");
static_assert(cmb::Engine<MM1>::TALLY_K == 0 &&
                  cmb::Engine<MM1Tally>::TALLY_K == 2,
              "opt-in detection");

constexpr int K = 2;

static uint64_t row_total(const TallyRec& r) {
    uint64_t n = 0;
    for (uint32_t b = 0; b < cmb::TALLY_NBINS; ++b) n += r.bins[b];
    return n;
}

int main() {
    // bin function corners
    const double lo = 0x1p-24, hi = 0x1p24;
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(cmb::tally_bin(0.0) == 0 && cmb::tally_bin(-0.0) == 0);
    CHECK(cmb::tally_bin(-1.0) == 0 && cmb::tally_bin(5e-324) == 0);
    CHECK(cmb::tally_bin(std::nextafter(lo, 0.0)) == 0);
    CHECK(cmb::tally_bin(lo) == 1 && cmb::tally_bin(1.0) == 385);
    CHECK(cmb::tally_bin(std::nextafter(2.0, 0.0)) == 400);
    CHECK(cmb::tally_bin(std::nextafter(hi, 0.0)) == 768);
    CHECK(cmb::tally_bin(hi) == 769 && cmb::tally_bin(inf) == 769);
    CHECK(cmb::tally_edge(0) == 0.0 && cmb::tally_edge(1) == lo);
    CHECK(cmb::tally_edge(385) == 1.0 && cmb::tally_edge(769) == hi);
    for (uint32_t b = 1; b < cmb::TALLY_NBINS; ++b) {
        const double e = cmb::tally_edge(b);
        CHECK(cmb::tally_bin(e) == b);
        CHECK(cmb::tally_bin(std::nextafter(e, 0.0)) == b - 1);
    }

    // window check: size guard on the window as requested, 32-bit indices
    const uint64_t fit = cmb::TALLY_ARENA_MAX_BYTES / sizeof(TallyRec) / K;
    TallySink req = {nullptr, 0, fit};
    CHECK(cmb::tally_sink_check(&req, K, 0, 1) == 0);
    req.count = fit + 1;
    CHECK(cmb::tally_sink_check(&req, K, 0, 1) == cmb::TALLY_ERR_ARENA_TOO_BIG);
    req.count = 1;
    CHECK(cmb::tally_sink_check(&req, K, UINT64_C(1) << 32, 1) ==
          cmb::TALLY_ERR_BAD_SINK);
    CHECK(cmb::tally_sink_check(&req, 9, 0, 1) == cmb::TALLY_ERR_BAD_SINK);
    CHECK(cmb::tally_sink_check(nullptr, K, 0, 1) == 0);
    uint64_t f, c;
    cmb::tally_clip_window(3, 100, 5, 4, &f, &c);
    CHECK(f == 5 && c == 4);
    cmb::tally_clip_window(6, ~UINT64_C(0), 5, 4, &f, &c);
    CHECK(f == 6 && c == 3);
    cmb::tally_clip_window(20, 5, 5, 4, &f, &c);
    CHECK(c == 0);

    // bind / add / wrap on a bare engine: window [5, 7)
    {
        std::vector<TallyRec> arena(2 * K);  // zeroed
        auto store = std::make_unique<cmb::Engine<MM1Tally>::Storage>();
        cmb::Engine<MM1Tally> E(*store);
        const MM1Tally::Params p{1.0, 1.0, 1};
        E.tally_attach({arena.data(), 5, 2});
        E.init(&p, 1, 4);  // below the window: g - first wraps
        CHECK(E.tally_slot == nullptr);
        E.tally(0, 1.0);
        E.init(&p, 1, 7);  // past the window
        CHECK(E.tally_slot == nullptr);
        E.tally(1, 1.0);
        for (const TallyRec& r : arena) CHECK(row_total(r) == 0 && r.s.n == 0.0);
        E.init(&p, 1, 6);
        CHECK(E.tally_slot == arena.data() + K);
        E.tally(0, 1.0);
        E.tally(0, -3.0);
        E.tally(0, std::nan(""));
        E.tally(1, inf);
        CHECK(arena[2].s.n == 2.0 && arena[2].s.mn == -3.0 &&
              arena[2].s.mx == 1.0 && arena[2].nan_cnt == 1);
        CHECK(arena[2].bins[385] == 1 && arena[2].bins[0] == 1 &&
              row_total(arena[2]) == 2);
        CHECK(arena[3].bins[769] == 1 && row_total(arena[3]) == 1);
        CHECK(row_total(arena[0]) == 0 && row_total(arena[1]) == 0);
        // a rebind resets the headers of its own slot only
        E.init(&p, 1, 6);
        CHECK(arena[2].s.n == 0.0 && arena[2].nan_cnt == 0);
    }

    // the model through run_host: 8 trials, window [2, 5), two threads
    const MM1Tally::Params p{1.0 / 0.9, 1.0, 200};
    std::vector<MM1Tally::Result> res(8), plain(8);
    std::vector<TallyRec> arena(3 * K);
    const TallySink sink = {arena.data(), 2, 3};
    cmb::run_host<MM1Tally>(p, 7, 8, 2, res.data(), {}, nullptr, 0, nullptr,
                            &sink);
    cmb::run_host<MM1>(p, 7, 8, 1, plain.data());
    CHECK(std::memcmp(res.data(), plain.data(), 8 * sizeof res[0]) == 0);
    for (int s = 0; s < 3; ++s) {
        const TallyRec& sys = arena[s * K];
        const TallyRec& que = arena[s * K + 1];
        CHECK(sys.s.n == (double)res[2 + s].obj_cnt && que.s.n == sys.s.n);
        CHECK(row_total(sys) == res[2 + s].obj_cnt);
        CHECK(row_total(que) == res[2 + s].obj_cnt);
        CHECK(sys.nan_cnt == 0 && que.nan_cnt == 0);
        CHECK(que.bins[0] > 0 && que.s.mn == 0.0);  // idle-server arrivals
        const double sum = sys.s.mean * sys.s.n;
        CHECK(std::fabs(sum - res[2 + s].sum_wait) <=
              1e-9 * res[2 + s].sum_wait);
    }
    std::printf("tally selfcheck OK\n");
    return 0;
}
