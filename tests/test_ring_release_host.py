"""The descriptor ring's release bookkeeping (csrc/ss_ring.hpp) on its own, without HIP: the step sequences of
tests/test_ring_release.py driven through tests/ring_release_host.cpp, checked against a model written from the rule - "an event
exists only for groups whose slots the device read; a group is waited for only when its event holds a record of its last round"."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RING, GROUP = 16, 4
PACE = RING              # steps without a ring event between two records of the pace event
PACE_TOTALS = [0, 0]     # pace events / waits of the last run()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("ring") / "ring_release_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "ring_release_host.cpp"), "-o", out])
    return out


def run(exe, seq):
    lines = subprocess.check_output([exe, seq], text=True).strip().splitlines()
    rows = []
    for ln in lines[:-1]:
        k, g, w, e, r, pc = ln.split()
        rows.append(dict(slot=int(k), group=int(g), wait=int(w.split("=")[1]), early=int(e.split("=")[1]), record=int(r.split("=")[1]),
                         pace=int(pc.split("=")[1])))
    tot = dict(kv.split("=") for kv in lines[-1].split())
    PACE_TOTALS[:] = [int(tot["pace_events"]), int(tot["pace_waits"])]
    return rows, int(tot["events"]), int(tot["waits"])


def model(seq):
    """the rule, restated step by step: returns the same rows"""
    recorded = [False] * (RING // GROUP)
    k, cur, stream, gstream = 0, None, 0, 0           # cur: [group, read] of the open group
    rows, events, waits = [], 0, 0
    since, paced_before = 0, False
    for c in seq:
        if c in "TR":
            stream ^= 1
        early = -1
        if cur is not None and (stream != gstream or k // GROUP != cur[0]):
            if cur[1]:
                recorded[cur[0]], early = True, cur[0]
                events += 1
            k = (cur[0] + 1) * GROUP % RING
            cur = None
        g = k // GROUP
        wait = 0
        if k % GROUP == 0:
            if recorded[g]:
                recorded[g], wait = False, 1
                waits += 1
            cur, gstream = [g, False], stream
        rec = pc = 0
        slot = k
        if c != "x":
            cur[1] = cur[1] or c in "rRf"
            k = (k + 1) % RING
            if slot % GROUP == GROUP - 1:
                if cur[1]:
                    recorded[g], rec = True, 1
                    events += 1
                cur = None
            if rec:
                since = 0
            else:
                since += 1
                if since == PACE:
                    since, pc = 0, 2 if paced_before else 1
                    paced_before = True
        rows.append(dict(slot=slot, group=g, wait=wait, early=early, record=rec, pace=pc))
    return rows, events, waits


WARM = "r" + "t" * 19                                   # the first step uploads the windows; 20 steps = 1.25 revolutions


def test_table_steps_record_nothing_and_wait_for_nothing(exe):
    rows, ev, wt = run(exe, WARM + "t" * 40)
    assert (rows, ev, wt) == model(WARM + "t" * 40)
    assert ev == 1 and wt == 1                          # the upload's group, waited for at slot 16
    assert rows[3]["record"] == 1 and rows[16]["wait"] == 1
    assert not any(r["record"] or r["wait"] or r["early"] >= 0 for r in rows[20:])


def test_mixed_route_records_exactly_the_groups_that_were_read(exe):
    seq = WARM + "".join("r" if (k // 4) % 2 == 0 and k % 4 == 1 else "t" for k in range(40))
    rows, ev, wt = run(exe, seq)
    assert (rows, ev, wt) == model(seq)
    assert ev - 1 == 5 and wt - 1 == 3
    assert [20 + k for k in range(40) if rows[20 + k]["record"]] == [23, 31, 39, 47, 55]      # the last slot of each read group
    assert [20 + k for k in range(40) if rows[20 + k]["wait"]] == [36, 44, 52]                # ring groups 1, 3, 1 revisited
    seq = WARM + "tr" * 20                              # alternating: every group
    rows, ev, wt = run(exe, seq)
    assert (rows, ev, wt) == model(seq)
    assert ev - 1 == 10 and wt - 1 == 10 - 4 + 0        # (the first visit of each of the four ring groups finds no record)


def test_new_key_stream_change_failed_and_refused_steps(exe):
    seq = WARM + "tttttt" + "r" + "t" * 34              # a window upload in the third slot of a group of table steps
    rows, ev, wt = run(exe, seq)
    assert (rows, ev, wt) == model(seq) and ev - 1 == 1
    assert rows[27]["record"] == 1 and rows[27]["group"] == 2
    seq = WARM + "t" * 8 + "r" + "T" + "t" * 12 + "T" + "t" * 7 + "T" + "t" * 9     # stream changes behind a read step / table steps
    rows, ev, wt = run(exe, seq)
    assert (rows, ev, wt) == model(seq) and ev - 1 == 1
    assert rows[29]["early"] == 3 and rows[29]["slot"] == 0                   # closed two slots in, on the old stream; next group
    assert rows[42]["early"] == -1 and rows[42]["slot"] % 4 == 0              # a group of table steps: closed without an event
    assert rows[41]["wait"] == 1 and rows[41]["group"] == 3                   # ... and group 3's record is consumed a ring later
    seq = "tft" + "x" + "t" + "tx" + "xt" * 14          # a failed step marks its group read; refused steps take no slot
    rows, ev, wt = run(exe, seq)
    assert (rows, ev, wt) == model(seq)
    assert rows[4]["record"] == 1 and rows[4]["slot"] == 3 and ev == 1
    assert [r["slot"] for r in rows[5:10]] == [4, 5, 5, 5, 6]
    assert wt == 1                                      # group 0 again after a full ring


@pytest.mark.parametrize("seed", range(8))
def test_random_sequences_follow_the_rule(exe, seed):
    import random
    rnd = random.Random(seed)
    seq = "".join(rnd.choice("ttttttrrfxTR") for _ in range(300))
    assert run(exe, seq) == model(seq)


def test_table_steps_are_paced_one_event_per_ring_length(exe):
    """steps that record no ring event: the pace event every 16th of them, waited for from its second record on - the host stays
    within two ring lengths of the device without a marker per group"""
    rows, ev, wt = run(exe, "t" * 100)
    assert (rows, ev, wt) == model("t" * 100) and ev == 0 and wt == 0
    assert [i for i, r in enumerate(rows) if r["pace"]] == [15, 31, 47, 63, 79, 95]
    assert [r["pace"] for r in rows if r["pace"]] == [1, 2, 2, 2, 2, 2] and PACE_TOTALS == [6, 5]
    rows, ev, wt = run(exe, "tr" * 40)                 # every group records its ring event: that bounds the host, no pace event
    assert (rows, ev, wt) == model("tr" * 40) and ev == 20 and PACE_TOTALS == [0, 0]
