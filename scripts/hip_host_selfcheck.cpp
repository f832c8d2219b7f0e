// Stand-alone host check of the HIP plumbing in
// cimba_amd/csrc/hip/hip_host.hpp (HIP_TRY, DevBuf, EventTimer, env_int):
//
//   hipcc -std=c++17 -O1 -g -Icimba_amd/csrc/hip \
//       scripts/hip_host_selfcheck.cpp -o hip_host_selfcheck
//
// (for a sanitizer run of the host code add
//  -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all).
//
// Passes with and without a device.  Without one every hipMalloc /
// hipEventCreate fails and leaves its handle null: each helper must then
// return non-zero, get() stay null and every destructor run clean -- the
// early-return path of the entry points.  With a device each helper
// returns 0 and 1 KiB makes the round trip.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "hip_host.hpp"

using cmb_hip::DevBuf;
using cmb_hip::env_int;
using cmb_hip::EventTimer;

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #x); \
            return 1;                                                  \
        }                                                              \
    } while (0)

constexpr size_t N = 256;  // ints: 1 KiB

// the shape of an entry point: owners first, HIP_TRY returns in between
static int entry_point_shape(int* steps) {
    DevBuf<int> a, b;
    EventTimer timer;
    *steps = 0;
    HIP_TRY(a.alloc(N));
    ++*steps;
    HIP_TRY(b.alloc(N));
    ++*steps;
    HIP_TRY(timer.start());
    ++*steps;
    double ms = -1.0;
    HIP_TRY(timer.stop(&ms));
    ++*steps;
    return 0;
}

static int check_env_int() {
    unsetenv("CIMBA_SELFCHECK_KNOB");
    CHECK(!env_int("CIMBA_SELFCHECK_KNOB").has_value());
    CHECK(env_int("CIMBA_SELFCHECK_KNOB").value_or(7) == 7);
    setenv("CIMBA_SELFCHECK_KNOB", "0", 1);
    CHECK(env_int("CIMBA_SELFCHECK_KNOB").has_value());
    CHECK(*env_int("CIMBA_SELFCHECK_KNOB") == 0);
    setenv("CIMBA_SELFCHECK_KNOB", "12", 1);
    CHECK(*env_int("CIMBA_SELFCHECK_KNOB") == 12);
    setenv("CIMBA_SELFCHECK_KNOB", "junk", 1);  // atoi semantics
    CHECK(*env_int("CIMBA_SELFCHECK_KNOB") == 0);
    unsetenv("CIMBA_SELFCHECK_KNOB");
    return 0;
}

static int check_without_device() {
    {
        DevBuf<int> never;  // destructor of a never-allocated buffer
        EventTimer idle;    // and of a never-started timer
        CHECK(never.get() == nullptr);
    }
    DevBuf<int> buf;
    CHECK(buf.alloc(N) != 0);
    CHECK(buf.get() == nullptr);
    int host[N] = {0};
    CHECK(buf.zero() != 0 || buf.get() == nullptr);
    CHECK(buf.upload(host, N) != 0);
    CHECK(buf.download(host, N) != 0);
    DevBuf<int> moved(std::move(buf));
    CHECK(moved.get() == nullptr && buf.get() == nullptr);
    CHECK(moved.release() == nullptr);
    EventTimer timer;
    CHECK(timer.start() != 0);
    double ms = -1.0;
    CHECK(timer.stop(&ms) != 0);
    CHECK(ms == -1.0);
    int steps = -1;
    CHECK(entry_point_shape(&steps) != 0);
    CHECK(steps == 0);
    return 0;
}

static int check_with_device() {
    int pattern[N], back[N];
    for (size_t i = 0; i < N; ++i) pattern[i] = (int)(i * 2654435761u);
    {
        DevBuf<int> never;
        EventTimer idle;
        CHECK(never.get() == nullptr);
    }
    DevBuf<int> buf;
    CHECK(buf.alloc(N) == 0);
    CHECK(buf.get() != nullptr);
    CHECK(buf.zero() == 0);
    std::memset(back, 0xFF, sizeof(back));
    CHECK(buf.download(back, N) == 0);
    for (size_t i = 0; i < N; ++i) CHECK(back[i] == 0);
    CHECK(buf.upload(pattern, N) == 0);
    CHECK(buf.download(back, N) == 0);
    CHECK(std::memcmp(pattern, back, sizeof(back)) == 0);

    int* const raw = buf.get();
    DevBuf<int> moved(std::move(buf));  // move construction
    CHECK(buf.get() == nullptr && moved.get() == raw);
    DevBuf<int> assigned;
    CHECK(assigned.alloc(N) == 0);
    assigned = std::move(moved);  // frees its own, takes the other
    CHECK(moved.get() == nullptr && assigned.get() == raw);
    std::memset(back, 0, sizeof(back));
    CHECK(assigned.download(back, N) == 0);
    CHECK(std::memcmp(pattern, back, sizeof(back)) == 0);
    CHECK(assigned.alloc(N) == 0);  // re-alloc frees the old one

    int* handle = assigned.release();  // the caller owns it now
    CHECK(handle != nullptr && assigned.get() == nullptr);
    CHECK(hipFree(handle) == hipSuccess);

    EventTimer timer;
    CHECK(timer.start() == 0);
    double ms = -1.0;
    CHECK(timer.stop(&ms) == 0);
    CHECK(ms >= 0.0);
    CHECK(timer.start() == 0);  // reusable
    CHECK(timer.stop(&ms) == 0);

    int steps = -1;
    CHECK(entry_point_shape(&steps) == 0);
    CHECK(steps == 4);
    return 0;
}

int main() {
    if (check_env_int()) return 1;
    int ndev = 0;
    const bool have = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    if (have ? check_with_device() : check_without_device()) return 1;
    std::printf("hip_host_selfcheck ok (%s)\n",
                have ? "device" : "no device");
    return 0;
}
