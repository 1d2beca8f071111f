"""The shared scene of tests/test_spec_half_bucket_rows_host.py and tests/test_gpu_spec_half_bucket_rows.py: a HALF bank in three
length buckets under rows of 2 or 3 partition blocks (k_obs_rows<true, false, BUCKETS, MEL, HALF>, k_obs_blocks<true, MEL, HALF, HBK>).

Buckets of 1 / 3 / 5 partition blocks (caps 16 384 / 49 152 / 81 920) with 3 / 3 / 2 entries.  RIR lengths (``LENS``, what the
kernels read from rir_len) against the bucket's depth:
  bucket 0 (1 block):  0 (empty) | 9 000 | 16 385 -> ceil(L / kB) = 2, CLAMPED to the bucket's one block (the row holds 16 384 taps)
  bucket 1 (3 blocks): 16 385 (2 blocks: below) | 40 000 (3: at) | 70 000 -> 5, CLAMPED to 3 (the row holds 49 152 taps)
  bucket 2 (5 blocks): 49 152 (3: below) | 70 000 (5: at)
Entry 1 (bucket 0) is scaled by 32 768 and entry 4 (bucket 1) by 1e-6.  Nothing here is written to after it was built."""
import numpy as np

from oracle import ss_oracle as O
from ss_amd import planning as P

CAPS = [16384, 49152, 81920]
COUNTS = [3, 3, 2]
FIRST = [0, 3, 6]
LENS = [0, 9000, 16385, 16385, 40000, 70000, 49152, 70000]
SCALE = {1: 32768.0, 4: 1e-6}
EMPTY = 0
RIR_SR = 44100                                         # (the synthetic RIRs' decay is drawn for this rate whatever the row length)


def bucket_of(g):
    return max(b for b in range(len(FIRST)) if g >= FIRST[b])


def taps(g):
    """the taps entry g's row holds: its length, clamped by its bucket's capacity"""
    return min(LENS[g], CAPS[bucket_of(g)])


_SCENE = {}


def scene():
    """rows: per bucket float32 [n_b, 2, cap_b] (zero behind the entry's taps); lens int32 [8]"""
    if not _SCENE:
        rng = np.random.default_rng(77)
        rows = [np.zeros((n, 2, cap), np.float32) for n, cap in zip(COUNTS, CAPS)]
        for g in range(len(LENS)):
            b, n = bucket_of(g), taps(g)
            if n:
                rows[b][g - FIRST[b], :, :n] = O.synth_rir_blocks(rng, RIR_SR, n, n=1)[0] * np.float32(SCALE.get(g, 1.0))
        for r in rows:
            r.setflags(write=False)
        lens = np.asarray(LENS, np.int32)
        lens.setflags(write=False)
        _SCENE.update(rows=rows, lens=lens)
    return _SCENE


_SOURCES = {}


def sources(sr):
    """a 1-s and a 3-s clip at rate sr"""
    if sr not in _SOURCES:
        rng = np.random.default_rng(sr + 1)
        _SOURCES[sr] = [O.synth_sources(rng, sr, k=1, seconds=1)[0], O.synth_sources(rng, sr, k=1, seconds=3)[0]]
    return _SOURCES[sr]


def units(sr):
    """0: the first entry of bucket 1, the 3-s clip at t0 = 1 s | 1: the last entry of bucket 0 with a distractor in bucket 2 (terms of
    different depth) | 2: silent | 3: the empty RIR | 4: the clamped entry of bucket 1 with the 32768-scaled one as distractor |
    5: the last entry of the bank with the 1e-6-scaled one as distractor | 6: the 3-block entry of the 5-block bucket, the 3-s
    clip at t0 = 1 s.  Every entry of the bank is read."""
    return [dict(sound=1, t0=sr, rir=3),
            dict(sound=0, t0=0, rir=2, dis_sound=1, dis_rir=7),
            dict(rir=-1),
            dict(sound=0, t0=0, rir=EMPTY),
            dict(sound=1, t0=sr, rir=5, dis_sound=0, dis_rir=1),
            dict(sound=0, t0=0, rir=7, dis_sound=1, dis_rir=4),
            dict(sound=1, t0=sr, rir=6)]


LIVE = [0, 1, 4, 5, 6]
DEAD = [2, 3]


def terms(u):
    """(sound, t0, entry) of every term of unit u"""
    if u.get("rir", -1) < 0:
        return []
    return [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else [])


def plan(srcs, us, n_valid):
    """window descriptors + unit descriptors of a launch over the deepest bucket's blocks, as hostsim plans them"""
    nbh_max = max(1, P.ceil_div(max(CAPS), P.KB))
    nby = max(1, P.ceil_div(n_valid, P.KB))
    offs = np.cumsum([0] + [len(s) for s in srcs])
    cache, rows = {}, []

    def slot_of(sound, t0):
        if (sound, t0) not in cache:
            ws = P.plan_window_set(len(srcs[sound]), t0, nbh_max, nby, False)
            cache[(sound, t0)] = (sum(len(r) for r in rows), ws)
            rows.append(P.window_desc_rows(ws, int(offs[sound]), len(srcs[sound]), False))
        return cache[(sound, t0)]

    desc = np.zeros((len(us), 8), np.int32)
    for n, u in enumerate(us):
        if u.get("rir", -1) < 0:
            desc[n] = P.unit_desc_row()
            continue
        s0, ws = slot_of(u["sound"], u["t0"])
        if u.get("dis_rir", -1) >= 0:
            d0, dws = slot_of(u["dis_sound"], 0)
            desc[n] = P.unit_desc_row(u["rir"], s0, ws, u["dis_rir"], d0, dws)
        else:
            desc[n] = P.unit_desc_row(u["rir"], s0, ws)
    wd = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), np.int32), np.int32)
    return wd, desc
