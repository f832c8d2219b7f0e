// M/M/1 queue benchmark model — the reference's headline benchmark
// (reference benchmark/MM1_single.c / MM1_multi.c: arrival + service
// processes, one unlimited object queue, exponential interarrival/service,
// stop after num_objects objects; avg system time expected 1/(mu-lambda)).
//
// Written in the cimba_amd protothread style: each process body is a
// resumable state machine; the object is the arrival timestamp (a double in
// the queue's 64-bit payload), replacing the reference's mempool-allocated
// void* object (MM1_multi.c:56-63).
#pragma once

#include "../include/cimba/engine.hpp"

namespace cmb_models {

struct MM1 : cmb::ModelBase {
    struct Cfg {
        static constexpr int MAX_PROC = 2;
        static constexpr int MAX_EV = 16;
        static constexpr int TIMERS = 1;
        static constexpr int NUM_QUEUES = 1;
        static constexpr int QCAP = 512;  // P(Q > 512) at rho=0.9 ~ 4e-24
        static constexpr int NUM_RES = 0;
        static constexpr int NUM_POOLS = 0;
        static constexpr int NUM_BUFS = 0;
        static constexpr int NUM_PQ = 0;
        static constexpr int PQCAP = 1;
        static constexpr int NUM_COND = 0;
        // the event list never holds more than 2 entries (arrival hold +
        // service hold/grant), so 2 hot entries keep every sift in the
        // hot tier.  Measured on the LDS kernel at the bench shape
        // (profiles/r04_lds_hot_tier.md): HOT_EV 2 = 9.98 G ev/s (hot half
        // 392 B, 6 waves/CU), 4 = 8.88 G (472 B, 5 waves/CU), 1 = 9.40 G.
        // With the statistics records and the unused spill cursors out of
        // the queue header the hot half is 312 B, 8 waves/CU
        // (profiles/r09_hot_shrink.md)
        static constexpr int HOT_EV = 2;
        static constexpr bool LDS_HOT = true;
    };

    struct Params {
        double arr_mean;       // 1 / arrival rate
        double srv_mean;       // 1 / service rate
        uint64_t num_objects;  // objects generated per trial
    };

    struct Result {
        uint64_t obj_cnt;
        double sum_wait;
        uint64_t events;
        int32_t status;
        int32_t pad_;
    };

    struct ArrFrame {
        uint64_t i;
    };
    struct SrvFrame {
        uint64_t obj;  // bit-cast arrival time
    };
    // per-process persistent locals; frames[0] = arrival, frames[1] = service
    union Frame {
        ArrFrame arr;
        SrvFrame srv;
    };
    // model-wide per-trial accumulators
    struct Globals {
        uint64_t cnt;
        double sum;
    };

    enum Func : uint8_t { F_ARRIVAL = 0, F_SERVICE = 1 };

    // reference MM1_multi.c:56-69 arrivalfunc
    template <class E_>
    CMB_FORCEINLINE static void arrival(E_& E, typename E_::ProcT* self) {
        const Params& P = *E.params;
        ArrFrame& f = E.frames[0].arr;
        CMB_BEGIN();
        for (f.i = 0; f.i < P.num_objects; ++f.i) {
            CMB_HOLD(E.rng.exponential(P.arr_mean));
            CMB_QPUT(0, cmb::double_as_u64(E.now));
            if (CMB_SIG() != cmb::SIG_SUCCESS) break;
        }
        CMB_END();
    }

    // reference MM1_multi.c:71-88 servicefunc; accumulators are in acc_of(E)
    template <class E_>
    CMB_FORCEINLINE static void service(E_& E, typename E_::ProcT* self) {
        const Params& P = *E.params;
        SrvFrame& f = E.frames[1].srv;
        CMB_BEGIN();
        for (;;) {
            CMB_QGET(0, &f.obj);
            if (CMB_SIG() != cmb::SIG_SUCCESS) break;
            CMB_HOLD(E.rng.exponential(P.srv_mean));
            acc_of(E).sum += E.now - cmb::u64_as_double(f.obj);
            acc_of(E).cnt += 1u;
        }
        CMB_END();
    }

    template <class E_>
    CMB_FORCEINLINE static Globals& acc_of(E_& E) {
        return E.globals;
    }

    template <class E_>
    CMB_FORCEINLINE static void step(E_& E, int pidx) {
        auto* self = &E.procs[pidx];
        if (self->func == F_ARRIVAL)
            arrival(E, self);
        else
            service(E, self);
    }

    template <class E_>
    CMB_FORCEINLINE static void setup(E_& E) {
        E.queues[0].limit = cmb::CMB_UNLIMITED;
        acc_of(E).cnt = 0;
        acc_of(E).sum = 0.0;
        E.proc_init(0, F_ARRIVAL, 0);
        E.proc_init(1, F_SERVICE, 0);
        E.proc_start(0);
        E.proc_start(1);
    }

    template <class E_>
    CMB_FORCEINLINE static void finish(E_& E, Result& r) {
        r.obj_cnt = acc_of(E).cnt;
        r.sum_wait = acc_of(E).sum;
        r.events = E.ev_dispatched;
        r.status = E.status;
    }
};

// M/M/1 with a ONE-entry hot tier: the test model for the hot/cold heap
// boundary.  MM1 itself never leaves its 2 hot entries; here the second
// pending event lives in the cold tier, so every sift crosses the
// boundary.  Results equal MM1's bit for bit.
struct MM1Hot1 : MM1 {
    struct Cfg : MM1::Cfg {
        static constexpr int HOT_EV = 1;
    };
};

// M/M/1 with the queue's length history on: the test model for the
// time-weighted statistics records, which live in the cold half of the
// storage (Engine::Cold::qstats) and which no other LDS_HOT model
// touches.  The event order is MM1's; the Result carries the
// time-weighted mean queue length of the trial instead of the waits
// (sum_wait = mean, obj_cnt = 1).
struct MM1Rec : MM1 {
    template <class E_>
    CMB_FORCEINLINE static void setup(E_& E) {
        MM1::setup(E);
        E.queues[0].recording = 1;
    }

    template <class E_>
    CMB_FORCEINLINE static void finish(E_& E, Result& r) {
        // close the recording interval on a copy, as the C API does
        cmb::WtdRec st = E.qstats[0];
        st.stats.add((double)E.q_length(0), E.now - st.t_last);
        r.obj_cnt = 1;
        r.sum_wait = st.stats.mean;
        r.events = E.ev_dispatched;
        r.status = E.status;
    }
};

}  // namespace cmb_models
