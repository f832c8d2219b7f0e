// M/M/1 with the device tally stream switched on — the worked example for
// Cfg::DEVICE_TALLY (include/cimba/tally.hpp).  Params, Result, Frame and
// Globals are MM1's; the process bodies are MM1's plus two tally
// statements, so for any seed the Result equals MM1's bit for bit (a tally
// never blocks, draws or schedules).
//
//   tally  name    observed when                 value
//   0      system  the service hold ended        time in system (the term
//                                                MM1 adds to its sum)
//   1      queue   the service get succeeded     wait in queue, exactly 0.0
//                                                when the server was idle
#pragma once

#include "mm1.hpp"

namespace cmb_models {

struct MM1Tally : MM1 {
    struct Cfg : MM1::Cfg {
        static constexpr int DEVICE_TALLY = 2;
    };

    enum TallyId : int { TL_SYSTEM = 0, TL_QUEUE = 1 };

    template <class E_>
    CMB_FORCEINLINE static void service(E_& E, typename E_::ProcT* self) {
        const Params& P = *E.params;
        SrvFrame& f = E.frames[1].srv;
        CMB_BEGIN();
        for (;;) {
            CMB_QGET(0, &f.obj);
            if (CMB_SIG() != cmb::SIG_SUCCESS) break;
            CMB_TALLY(TL_QUEUE, E.now - cmb::u64_as_double(f.obj));
            CMB_HOLD(E.rng.exponential(P.srv_mean));
            const double wait = E.now - cmb::u64_as_double(f.obj);
            CMB_TALLY(TL_SYSTEM, wait);
            acc_of(E).sum += wait;
            acc_of(E).cnt += 1u;
        }
        CMB_END();
    }

    template <class E_>
    CMB_FORCEINLINE static void step(E_& E, int pidx) {
        auto* self = &E.procs[pidx];
        if (self->func == F_ARRIVAL)
            arrival(E, self);
        else
            service(E, self);
    }
};

}  // namespace cmb_models
