"""The scene shared by tests/test_spec_buckets_host.py and tests/test_gpu_spec_buckets.py: four tiny length buckets
(include/ss_hip.h "Spectral length buckets") and one launch of 12 units that touches every place where a bucket's base, scale
base or depth could be resolved wrongly.

Buckets: caps 16000 / 20000 / 40000 / 70000 samples = 1 / 2 / 3 / 5 partition blocks, 3 / 2 / 3 / 2 entries, global indices
0-2 / 3-4 / 5-7 / 8-9:

  0  as long as its cap (one block)                 5  as long as its cap, every block audible
  1  EMPTY                                          6  30000 taps, scaled by 1e-6
  2  16000 taps, scaled by 32768                    7  33000 taps, every block audible
  3  as long as its cap, every block audible        8  as long as its cap (70000), every block audible
  4  18000 taps                                     9  9000 taps in the 5-block bucket (the rir_len block skip)

Units: the first and the last entry of every bucket, the 3-s clip at t0 = 1 s through the two longest entries, a unit whose two
terms (distractor) live in different buckets, the empty entry and a silent unit."""
import numpy as np

from oracle import ss_oracle as O

SR = 16000
KB = 16384
CAPS = [16000, 20000, 40000, 70000]
COUNTS = [3, 2, 3, 2]
FIRST = [0, 3, 5, 8]
BIG, SMALL = 2, 6                       # the entries scaled by 32768 and by 1e-6 (buckets 0 and 2)
EMPTY = 1


def scene(seed=23):
    """-> dict(srcs=[two 1-s clips, one 3-s clip], rows=[per bucket float32 [n, 2, cap]], lens=int32 [10] over global indices,
    units=[dict(sound, t0, rir[, dis_sound, dis_rir]) | dict(rir=-1)])"""
    rng = np.random.default_rng(seed)
    srcs = list(O.synth_sources(rng, SR, k=2, seconds=1)) + [O.synth_sources(rng, SR, k=1, seconds=3)[0]]
    lens = np.asarray([16000, 0, 16000, 20000, 18000, 40000, 30000, 33000, 70000, 9000], np.int32)
    full = {0, 3, 5, 7, 8}                                            # every block audible
    rows = [np.zeros((n, 2, cap), np.float32) for n, cap in zip(COUNTS, CAPS)]
    for g, n in enumerate(lens):
        b = max(k for k in range(4) if FIRST[k] <= g)
        if n == 0:
            continue
        h = (O.synth_rir_blocks(rng, SR, int(n), n=1) if g in full else O.synth_rir(rng, SR, length=int(n), n=1))[0]
        if g == BIG:
            h = h * np.float32(32768.0)
        if g == SMALL:
            h = h * np.float32(1e-6)
        rows[b][g - FIRST[b], :, :n] = h
    units = [dict(sound=0, t0=0, rir=0), dict(sound=1, t0=0, rir=2),              # bucket 0: first, last (x 32768)
             dict(sound=0, t0=0, rir=3), dict(sound=1, t0=0, rir=4),              # bucket 1
             dict(sound=2, t0=SR, rir=5), dict(sound=0, t0=0, rir=7),             # bucket 2 (3-s clip at 1 s through 3 blocks)
             dict(sound=2, t0=SR, rir=8), dict(sound=1, t0=0, rir=9),             # bucket 3 (5 blocks; 9000 taps of 5 blocks)
             dict(sound=0, t0=0, rir=6),                                          # x 1e-6
             dict(sound=0, t0=0, rir=4, dis_sound=1, dis_rir=8),                  # two terms, buckets 1 and 3
             dict(sound=0, t0=0, rir=EMPTY), dict(rir=-1)]                        # empty entry, silent unit
    return dict(srcs=srcs, rows=rows, lens=lens, units=units)


def bucket_of(g):
    return max(k for k in range(len(FIRST)) if FIRST[k] <= g)


def row_of(sc, g):
    """time-domain RIR of global entry g, [2, len]"""
    b = bucket_of(g)
    return sc["rows"][b][g - FIRST[b]][:, :sc["lens"][g]]
