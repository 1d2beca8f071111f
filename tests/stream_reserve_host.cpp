// stream_reserve_host.cpp — TEST INFRASTRUCTURE: the pure rules behind captured steps (sound-spaces_amd/csrc/ss_launch.hpp),
// without HIP: what a launch does about its per-stream scratch (sslaunch::scratch_decision: use / allocate / refuse), the size of
// the hand-off area with its replay epoch word, and ss_stream_reserve's argument rule.  One line per case:
//     scratch <capturing> <have> <need> <U|A|R>
//     reserve <stream_ok> <out_len> <rir_cap> <n_terms> <0|1>
//     handoff <rows> <bytes>
// tests/test_stream_reserve_args.py builds this with -fsanitize=address,undefined, runs it and checks every line.  Never part of
// the product.
#include <cstdio>

#include "../sound-spaces_amd/csrc/ss_launch.hpp"

int main() {
    using namespace sslaunch;
    const size_t sizes[4] = {0, 1, 4096, static_cast<size_t>(3) << 30};
    for (int cap = 0; cap < 2; ++cap)
        for (size_t have : sizes)
            for (size_t need : sizes) {
                const Scratch d = scratch_decision(cap != 0, have, need);
                std::printf("scratch %d %zu %zu %c\n", cap, have, need, d == Scratch::kUse ? 'U' : d == Scratch::kAllocate ? 'A' : 'R');
            }
    const int lens[7] = {0, ssk::kB, ssk::kB + 1, 22050, 44100, 3 * ssk::kB, 3 * ssk::kB + 1};
    const int caps[4] = {-1, 0, 1, 2048};
    const int terms[4] = {0, 1, 2, 3};
    for (int ok = 0; ok < 2; ++ok)
        for (int len : lens)
            for (int cap : caps)
                for (int t : terms) std::printf("reserve %d %d %d %d %d\n", ok, len, cap, t, reserve_args_ok(ok != 0, len, cap, t) ? 1 : 0);
    std::printf("handoff %d %zu\n", kSyncRows, handoff_bytes(kSyncRows));
    return 0;
}
