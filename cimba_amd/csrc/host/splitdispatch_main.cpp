// Stand-alone driver for the split-dispatch engine flavour (engine.hpp
// HoldDeferState, dispatch_head/body/tail), meant to be built with
// -fsanitize=address,undefined:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -Icimba_amd/csrc/include cimba_amd/csrc/host/splitdispatch_main.cpp
//       cimba_amd/csrc/host/support.cpp -o splitdispatch && ./splitdispatch
//
// Runs a few M/M/1 and M/G/1 trials on the plain host flavour (FlatTier)
// and on the split one (FlatSplitTier), unbounded, cut by a time limit and
// cut by an event limit, on one engine reused from trial to trial, and
// checks that every trial's result is the same byte for byte.  Exit
// status 0 = all equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../models/mg1.hpp"
#include "../models/mm1.hpp"

namespace {

uint64_t seed_of(uint64_t master, uint64_t t) {
    return cmb::fmix64(master ^ (UINT64_C(0x9E3779B97F4A7C15) * (t + 1)));
}

template <class Model, class Tier>
std::vector<typename Model::Result> run(const typename Model::Params& p,
                                        uint64_t master, uint64_t ntrials,
                                        double until, uint64_t max_events) {
    using Eng = cmb::Engine<Model, Tier>;
    auto store = std::make_unique<typename Eng::Storage>();
    auto slab = std::make_unique<typename Eng::Spill>();
    auto eng = std::make_unique<Eng>(*store);
    if constexpr (Eng::NEEDS_SPILL) eng->set_spill(slab.get());
    std::vector<typename Model::Result> out(ntrials);
    for (uint64_t t = 0; t < ntrials; ++t) {
        std::memset(&out[t], 0, sizeof(out[t]));
        eng->init(&p, seed_of(master, t), (uint32_t)t);
        Model::setup(*eng);
        eng->run(until, max_events);
        Model::finish(*eng, out[t]);
    }
    return out;
}

template <class Model>
int compare(const char* name, const typename Model::Params& p, uint64_t master,
            uint64_t ntrials, double until, uint64_t max_events) {
    const auto a = run<Model, cmb::FlatTier>(p, master, ntrials, until,
                                             max_events);
    const auto b = run<Model, cmb::FlatSplitTier>(p, master, ntrials, until,
                                                  max_events);
    uint64_t events = 0, limited = 0;
    int bad = 0;
    for (uint64_t t = 0; t < ntrials; ++t) {
        events += a[t].events;
        limited += a[t].status == cmb::ST_EVENT_LIMIT;
        if (std::memcmp(&a[t], &b[t], sizeof(a[t])) != 0) ++bad;
    }
    std::printf("%s seed %llu until %g max_events %llu: %llu events, "
                "%llu trials at the event limit: %s\n",
                name, (unsigned long long)master, until,
                (unsigned long long)max_events, (unsigned long long)events,
                (unsigned long long)limited, bad ? "DIFFER" : "equal");
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t objs = argc > 1 ? strtoull(argv[1], nullptr, 0) : 200;
    const uint64_t none = UINT64_C(0xFFFFFFFFFFFFFFFF);
    int bad = 0;
    for (uint64_t seed : {UINT64_C(1), UINT64_C(2), UINT64_C(0xDEADBEEF)}) {
        const cmb_models::MM1::Params mm1{1.0 / 0.9, 1.0, objs};
        bad += compare<cmb_models::MM1>("mm1", mm1, seed, 8, 1.0e308, none);
        bad += compare<cmb_models::MM1>("mm1", mm1, seed, 8, 0.5 * objs, none);
        bad += compare<cmb_models::MM1>("mm1", mm1, seed, 8, 1.0e308, objs);
        for (int dist = 0; dist < 4; ++dist) {
            const cmb_models::MG1::Params mg1{1.25, 1.0, 0.25, objs, dist, 0};
            bad += compare<cmb_models::MG1>("mg1", mg1, seed, 8, 1.0e308, none);
            bad += compare<cmb_models::MG1>("mg1", mg1, seed, 8, 0.5 * objs,
                                            none);
            bad += compare<cmb_models::MG1>("mg1", mg1, seed, 8, 1.0e308, objs);
        }
    }
    return bad ? 1 : 0;
}
