// Stand-alone driver for the object-queue register-window fuzz
// (include/cimba/queuewinfuzz.hpp), meant to be built with
// -fsanitize=address,undefined:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -Icimba_amd/csrc/include cimba_amd/csrc/host/queuewinfuzz_main.cpp
//       -o queuewinfuzz && ./queuewinfuzz
//
// Runs the sequence on the plain flavour and at window widths 2, 4 and
// 7 (the widest the 8-slot ring permits) over a few seeds and checks
// that gets, lengths and status agree and that the sequence reached
// every case at every width.  Exit status 0 = all equal.
#include <cstdio>
#include <cstdlib>

#include "cimba/queuewinfuzz.hpp"

int main(int argc, char** argv) {
    const uint64_t nops = argc > 1 ? strtoull(argv[1], nullptr, 0) : 20000;
    const uint64_t seeds[] = {1, 2, UINT64_C(0xDEADBEEF), 4, 5};
    const int widths[] = {2, 4, cmb::QWIN_FUZZ_MAX_W};
    int bad = 0;
    for (uint64_t seed : seeds) {
        const auto ref = cmb::queue_window_fuzz_n(seed, nops, 0, 0);
        for (int w : widths) {
            const auto got = cmb::queue_window_fuzz_n(seed, nops, w, w);
            const bool same = got.window == w && got.gets == ref.gets &&
                              got.lens == ref.lens && got.status == ref.status;
            const bool reached =
                got.win_put && got.ring_put && got.tail_load &&
                got.short_get && got.tail_wrap && got.refill_out &&
                got.drain_put && got.queue_full && got.reinit_win &&
                got.reinit_ring;
            std::printf(
                "seed %llu W %d: %zu gets, win_put %llu ring_put %llu "
                "tail_load %llu short_get %llu tail_wrap %llu refill_out %llu "
                "drain_put %llu queue_full %llu reinit_win %llu "
                "reinit_ring %llu: %s%s\n",
                (unsigned long long)seed, w, got.gets.size(),
                (unsigned long long)got.win_put,
                (unsigned long long)got.ring_put,
                (unsigned long long)got.tail_load,
                (unsigned long long)got.short_get,
                (unsigned long long)got.tail_wrap,
                (unsigned long long)got.refill_out,
                (unsigned long long)got.drain_put,
                (unsigned long long)got.queue_full,
                (unsigned long long)got.reinit_win,
                (unsigned long long)got.reinit_ring,
                same ? "equal" : "DIFFER",
                reached ? "" : " (a case was not reached)");
            if (!same || !reached) ++bad;
        }
    }
    return bad ? 1 : 0;
}
