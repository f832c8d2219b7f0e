// Stand-alone host check of the device log stream (engine + devlog.hpp +
// the logged M/M/1 model), meant to be built with sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -ffp-contract=off \
//       -Icimba_amd/csrc/include scripts/devlog_selfcheck.cpp \
//       cimba_amd/csrc/host/support.cpp -lpthread -o devlog_selfcheck
//
// Runs the hand-checkable, ring-overflow and abort-line cases of
// tests/test_devlog.py against run_host, then formats and replays them.
#include <cstdio>
#include <cstring>
#include <vector>

#include "cimba/runner.hpp"
#include "../cimba_amd/csrc/models/mm1_logged.hpp"

using cmb::LogRec;
using cmb::LogSink;
using cmb_models::MM1Log;

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #x); \
            return 1;                                                  \
        }                                                              \
    } while (0)

struct Run {
    std::vector<LogRec> recs;
    std::vector<uint32_t> emitted;
    MM1Log::Result res;
    std::vector<LogRec> kept;  // un-rotated survivors
};

static Run run_one(double arr_rate, double srv_rate, uint64_t nobj,
                   uint32_t cap, uint32_t mask = 0xFFFFFFFFu) {
    Run r;
    r.recs.resize(cap);
    r.emitted.assign(1, 0);
    const LogSink sink = {r.recs.data(), r.emitted.data(), 0, 1, cap, mask};
    const MM1Log::Params p{1.0 / arr_rate, 1.0 / srv_rate, nobj};
    cmb::run_host<MM1Log>(p, 7, 1, 1, &r.res, {}, nullptr, 0, &sink);
    const uint32_t n = r.emitted[0], k = n < cap ? n : cap;
    for (uint32_t q = n - k; q != n; ++q) r.kept.push_back(r.recs[q % cap]);
    return r;
}

int main() {
    // hand-checkable content: 3 objects -> 9 records, three per code
    Run full = run_one(0.9, 1.0, 3, 64);
    CHECK(full.emitted[0] == 9 && full.kept.size() == 9);
    double sum = 0.0;
    int per_code[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < 9; ++i) {
        const LogRec& x = full.kept[i];
        CHECK(x.seq == i);
        CHECK(i == 0 || x.t >= full.kept[i - 1].t);
        CHECK(x.code >= 1 && x.code <= 3);
        CHECK(x.proc == (x.code == MM1Log::LC_ARRIVE ? 0 : 1));
        if (x.code == MM1Log::LC_ARRIVE)
            CHECK(x.value == (uint64_t)per_code[1]);
        if (x.code == MM1Log::LC_DEPART) sum += cmb::u64_as_double(x.value);
        ++per_code[x.code];
    }
    CHECK(per_code[1] == 3 && per_code[2] == 3 && per_code[3] == 3);
    CHECK(std::memcmp(&sum, &full.res.sum_wait, sizeof sum) == 0);

    // ring keeps the last records
    Run small = run_one(0.9, 1.0, 3, 4);
    CHECK(small.emitted[0] == 9 && small.kept.size() == 4);
    CHECK(std::memcmp(small.kept.data(), full.kept.data() + 5,
                      4 * sizeof(LogRec)) == 0);
    CHECK(std::memcmp(&small.res, &full.res, sizeof full.res) == 0);

    // abort line: the 512-slot queue overflows at rho = 4
    Run ab = run_one(4.0, 1.0, 4000, 8);
    CHECK(ab.res.status == cmb::ST_QUEUE_FULL);
    CHECK(ab.emitted[0] > 8 && ab.kept.size() == 8);
    const LogRec& last = ab.kept[7];
    CHECK(last.flags == cmb::LOG_ERROR && last.code == 2 && last.proc == -1);
    CHECK(last.vtype == cmb::LOGV_I64 && last.value == 2);
    CHECK(last.t >= ab.kept[6].t);

    // formatter + replay walk every surviving record
    char buf[256];
    cmb::log_format(buf, sizeof buf, last, 0, cmb::trial_seed(7, 0),
                    cmb::status_name(last.code));
    CHECK(std::strstr(buf, " engine error: queue_full value=2") != nullptr);
    cmb::logger_stream_set(stdout);
    const uint64_t walked = cmb::log_replay(
        ab.recs.data(), ab.emitted.data(), 0, 1, 8,
        [](uint64_t g) { return cmb::trial_seed(7, g); },
        [](const LogRec& r) {
            return r.proc < 0 ? cmb::status_name(r.code)
                              : MM1Log::log_name(r.code);
        });
    CHECK(walked == 8);
    std::printf("devlog selfcheck OK\n");
    return 0;
}
