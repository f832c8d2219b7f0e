// Stand-alone driver for the hot-tier heap fuzz (include/cimba/heapfuzz.hpp),
// meant to be built with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined
//       -Icimba_amd/csrc/include cimba_amd/csrc/host/heapfuzz_main.cpp
//       -o heapfuzz && ./heapfuzz
//
// Runs every hot-tier size over a few seeds and checks that the pop
// sequences agree with the untiered heap.  Exit status 0 = all equal.
#include <cstdio>
#include <cstdlib>

#include "cimba/heapfuzz.hpp"

int main(int argc, char** argv) {
    const uint64_t nops = argc > 1 ? strtoull(argv[1], nullptr, 0) : 20000;
    const int hots[] = {1, 2, 4};
    int bad = 0;
    for (uint64_t seed = 1; seed <= 5; ++seed) {
        const auto ref = cmb::heap_tier_fuzz_n(seed, nops, 0);
        for (int hot : hots) {
            const auto got = cmb::heap_tier_fuzz_n(seed, nops, hot);
            bool same = got.size() == ref.size();
            for (size_t i = 0; same && i < ref.size(); ++i)
                same = got[i].t == ref[i].t && got[i].pseq == ref[i].pseq &&
                       got[i].handle == ref[i].handle;
            std::printf("seed %llu hot %d: %zu pops %s\n",
                        (unsigned long long)seed, hot, got.size(),
                        same ? "equal" : "DIFFER");
            if (!same) ++bad;
        }
    }
    return bad ? 1 : 0;
}
