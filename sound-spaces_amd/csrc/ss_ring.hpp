// ss_ring.hpp — which groups of the descriptor ring record a completion event, and which are waited for (pure host C++, no
// HIP: tests/ring_release_host.cpp drives it on its own; ss_hip.hip, ctx_observe_on, issues the HIP calls it asks for).
//
// A ring slot holds pinned memory the DEVICE may read after the call has returned: the step's unit descriptors (read in
// place by the kernels that take no unit table, or the source of the upload of a large step) and the step's new window rows
// (the source of their upload).  Before the host rewrites a slot, a full ring later, whatever read it must have finished:
// one completion event per group of kGroup consecutive slots, recorded behind the group's last launch.
// An event exists only for groups whose slots the device read.  A step whose launch carries its units in the kernel
// arguments (fill_unit_tab) and uploads no window leaves nothing in the slot for the device: a group of such steps records
// no event (a marker packet between two launches: 2.6-3 us of idle GPU, profiles/r7/NOTES.md) and its next round waits for
// nothing.
//
// The group events were also what kept the host from running more than a ring ahead of the device.  Without them a caller that
// never synchronises queues thousands of launches: the runtime then falls off its fast path (its pool of completion signals is
// finite) and the device stalls for tens of microseconds now and then.  Pace bounds the run-ahead on its own terms: one event
// per kPace steps that recorded no ring event, waited for one period later - a sixteenth of the markers the ring used to cost.
#pragma once

namespace ssring {

template <int RING, int GROUP>
struct Release {
    static constexpr int kGroups = RING / GROUP;
    bool recorded[kGroups] = {};      // the group's event holds a record of the group's LAST round that nobody has waited for yet
    bool open = false;                // a group has been started and not closed
    bool open_read = false;           // ... and the device was given one of its slots to read
    int open_group = 0;
    long long n_records = 0, n_waits = 0;

    void reset() {                    // everything issued so far has completed (device synchronise)
        for (int g = 0; g < kGroups; ++g) recorded[g] = false;
        open = open_read = false;
    }
    // The caller is about to take slot k on another stream than the open group's, or slot k lies in another group (a failed
    // step left the group open): the open group ends here.  True: record its event on the OLD stream.  Either way the next slot
    // is the first of the following group (next_slot()).
    bool must_close_before(int k, bool same_stream) const { return open && (!same_stream || k / GROUP != open_group); }
    bool close_early() {
        const bool rec = open_read;
        if (rec) { recorded[open_group] = true; ++n_records; }
        open = open_read = false;
        return rec;
    }
    int next_slot() const { return (open_group + 1) * GROUP % RING; }
    // Slot k is taken.  True (first slot of a group only): synchronise on the group's event first.
    bool begin(int k) {
        if (k % GROUP) return false;
        const int g = k / GROUP;
        const bool wait = recorded[g];
        if (wait) { recorded[g] = false; ++n_waits; }
        open = true;
        open_read = false;
        open_group = g;
        return wait;
    }
    // The step in slot k has issued its work (or failed after it may have issued some: slot_read = true).  True: record the
    // group's event behind it - the group's last slot, and some step of the group let the device read its slot.
    bool end(int k, bool slot_read) {
        open_read = open_read || slot_read;
        if (k % GROUP != GROUP - 1) return false;
        return close_early();
    }
};

// Host run-ahead bound for steps that record no ring event (see above).  Every step calls step(): true = record the pace event
// behind this step's launch, after synchronising on its previous record when `wait_first` says so.  A step that recorded or waited
// for a ring event restarts the period (that event bounds the host as it always did).
template <int PACE>
struct Pace {
    int since = 0;                    // steps since the last record of any kind
    bool recorded = false;            // the pace event holds a record nobody has waited for
    long long n_records = 0, n_waits = 0;

    void reset() { since = 0; recorded = false; }
    void ring_event() { since = 0; }
    bool step(bool* wait_first) {
        *wait_first = false;
        if (++since < PACE) return false;
        since = 0;
        if (recorded) { *wait_first = true; ++n_waits; }
        recorded = true;
        ++n_records;
        return true;
    }
};

}  // namespace ssring
