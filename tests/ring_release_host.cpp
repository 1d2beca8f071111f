// ring_release_host.cpp — TEST INFRASTRUCTURE: drives ssring::Release (sound-spaces_amd/csrc/ss_ring.hpp, the bookkeeping
// ctx_observe_on consults for its descriptor ring) through a sequence of steps and prints what it asks the caller to do.
//   argv[1]: one character per call of ss_ctx_observe
//     t  a step that took the unit-table route and uploaded nothing (the device reads nothing from its slot)
//     r  a step whose slot the device reads (descriptors in place / uploaded, a window upload)
//     f  a step that fails after its slot was taken (counts as read)
//     x  a step the planner refuses before a slot is taken (nothing changes but a group may have been begun)
//     T R  as t / r, issued on the OTHER stream than the step before
//   output, one line per call: "<slot> <group> wait=<0|1> early=<-1|group recorded on the old stream> record=<0|1> pace=<0|1|2>"
//   (pace: 1 = the pace event is recorded behind the step, 2 = after a host wait for its previous record; ssring::Pace)
//   and a last line "events=<n> waits=<n> pace_events=<n> pace_waits=<n>".
#include <cstdio>
#include <cstring>

#include "../sound-spaces_amd/csrc/ss_ring.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    constexpr int kRing = 16, kGroup = 4;
    ssring::Release<kRing, kGroup> ring;
    ssring::Pace<kRing> pace;
    int ring_k = 0, stream = 0, group_stream = 0;
    for (const char* p = argv[1]; *p; ++p) {
        const char c = *p;
        if (c == 'T' || c == 'R') stream ^= 1;
        int early = -1;
        if (ring.must_close_before(ring_k, stream == group_stream)) {     // (as ctx_observe_on)
            const int og = ring.open_group;
            if (ring.close_early()) early = og;
            ring_k = ring.next_slot();
        }
        const int k = ring_k, g = k / kGroup;
        const bool wait = ring.begin(k);
        if (k % kGroup == 0) group_stream = stream;
        bool record = false;
        int paced = 0;
        if (c != 'x') {
            ring_k = (k + 1) % kRing;
            record = ring.end(k, c == 'r' || c == 'R' || c == 'f');
            if (record) pace.ring_event();                                // (as close_slot in ctx_observe_on)
            else {
                bool wait_first = false;
                if (pace.step(&wait_first)) paced = wait_first ? 2 : 1;
            }
        }
        std::printf("%d %d wait=%d early=%d record=%d pace=%d\n", k, g, wait ? 1 : 0, early, record ? 1 : 0, paced);
    }
    std::printf("events=%lld waits=%lld pace_events=%lld pace_waits=%lld\n", ring.n_records, ring.n_waits, pace.n_records, pace.n_waits);
    return 0;
}
