// M/M/1 with the device log stream switched on — the worked example for
// Cfg::DEVICE_LOG (include/cimba/devlog.hpp).  Params, Result, Frame and
// Globals are MM1's; the process bodies are MM1's plus log calls, so for
// any seed the Result equals MM1's bit for bit (logging never blocks,
// draws or schedules).
//
//   code  name    flag        emitted when                  payload
//   1     arrive  LOG_INFO    the arrival put succeeded     object ordinal
//   2     start   user bit 4  the service get succeeded     arrival time
//   3     depart  LOG_INFO    the service hold ended        time in system
#pragma once

#include "mm1.hpp"

namespace cmb_models {

struct MM1Log : MM1 {
    struct Cfg : MM1::Cfg {
        static constexpr bool DEVICE_LOG = true;
    };

    enum LogCode : uint16_t { LC_ARRIVE = 1, LC_START = 2, LC_DEPART = 3 };
    static constexpr uint32_t LOG_START = 1u << 4;  // first user flag bit

    template <class E_>
    CMB_FORCEINLINE static void arrival(E_& E, typename E_::ProcT* self) {
        const Params& P = *E.params;
        ArrFrame& f = E.frames[0].arr;
        CMB_BEGIN();
        for (f.i = 0; f.i < P.num_objects; ++f.i) {
            CMB_HOLD(E.rng.exponential(P.arr_mean));
            CMB_QPUT(0, cmb::double_as_u64(E.now));
            if (CMB_SIG() != cmb::SIG_SUCCESS) break;
            CMB_LOG_U(cmb::LOG_INFO, LC_ARRIVE, f.i);
        }
        CMB_END();
    }

    template <class E_>
    CMB_FORCEINLINE static void service(E_& E, typename E_::ProcT* self) {
        const Params& P = *E.params;
        SrvFrame& f = E.frames[1].srv;
        CMB_BEGIN();
        for (;;) {
            CMB_QGET(0, &f.obj);
            if (CMB_SIG() != cmb::SIG_SUCCESS) break;
            CMB_LOG_D(LOG_START, LC_START, cmb::u64_as_double(f.obj));
            CMB_HOLD(E.rng.exponential(P.srv_mean));
            const double wait = E.now - cmb::u64_as_double(f.obj);
            CMB_LOG_D(cmb::LOG_INFO, LC_DEPART, wait);
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

    // host-only: record names for the formatter
    static const char* log_name(uint16_t code) {
        switch (code) {
            case LC_ARRIVE: return "arrive";
            case LC_START: return "start";
            case LC_DEPART: return "depart";
        }
        return "?";
    }
};

}  // namespace cmb_models
