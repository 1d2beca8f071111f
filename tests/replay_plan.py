"""TEST INFRASTRUCTURE: the steps the graph-replay tests render (tests/test_blocks_replay_host.py, tests/test_gpu_graph_replay.py).

A step = three units over two clips of three seconds each: one with a distractor term, one plain, one silent - and which slot is
which, the window starts and the bank entries all move with the step number k, while the SHAPES stay fixed (three window sets of
nby windows each, three unit descriptors), so that a captured graph can be fed by rewriting its inputs in place."""
import numpy as np

from ss_amd import planning as P

N_BANK = 4                             # bank entries
RIR_CAP = 2048                         # samples per bank row: one RIR block


def world(sr, seed):
    """-> (clips float32 [2, 3 sr] read-only, bank float32 [N_BANK, 2, RIR_CAP] read-only, lens int32 [N_BANK])"""
    from oracle import ss_oracle as O
    rng = np.random.default_rng(seed)
    clips = O.synth_sources(rng, sr, k=2, seconds=3)
    bank = O.synth_rir(rng, sr, length=RIR_CAP, n=N_BANK)
    lens = np.array([RIR_CAP, 1500, RIR_CAP, 777], np.int32)
    for r in range(N_BANK):
        bank[r, :, lens[r]:] = 0.0     # (rows are zero behind their length: include/ss_hip.h)
    clips.setflags(write=False); bank.setflags(write=False)
    return clips, bank, lens


def step_units(k, sr, n_units=3):
    """the units of step k: slot (k % n) is silent, slot (k + 1) % n carries a distractor term, the others are plain"""
    units = []
    for n in range(n_units):
        role = (n - k) % n_units
        if role == 0:
            units.append(dict(rir=-1))
        elif role == 1:
            units.append(dict(sound=k % 2, t0=sr * (k % 3), rir=k % N_BANK, dis_sound=(k + 1) % 2, dis_t0=sr * ((k + 1) % 3),
                              dis_rir=(k + 2) % N_BANK))
        else:
            units.append(dict(sound=(k + n) % 2, t0=sr * ((k + n + 2) % 3), rir=(k + n + 1) % N_BANK))
    return units


def plan(units, src_len, n_valid):
    """-> (win_desc int32 [W, 4], unit_desc int32 [N, 8]) for clips of src_len samples laid out back to back; one window set per
    term (no sharing between units: W = terms x nby whatever the step)"""
    nby = P.ceil_div(n_valid, P.KB)
    nbh = P.ceil_div(RIR_CAP, P.KB)
    rows, n_rows = [], 0
    desc = np.zeros((len(units), 8), np.int32)

    def term(sound, t0):
        nonlocal n_rows
        ws = P.plan_window_set(src_len, t0, nbh, nby)
        assert ws.count == nby, (t0, ws)
        slot = n_rows
        rows.append(P.window_desc_rows(ws, sound * src_len, src_len))
        n_rows += ws.count
        return slot, ws

    for n, u in enumerate(units):
        if u.get("rir", -1) < 0:
            desc[n] = P.unit_desc_row()
            continue
        s0, ws = term(u["sound"], u["t0"])
        if u.get("dis_rir", -1) >= 0:
            d0, dws = term(u["dis_sound"], u["dis_t0"])
            desc[n] = P.unit_desc_row(u["rir"], s0, ws, u["dis_rir"], d0, dws)
        else:
            desc[n] = P.unit_desc_row(u["rir"], s0, ws)
    return np.ascontiguousarray(np.concatenate(rows), np.int32), desc
