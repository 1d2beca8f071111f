"""The zero-column shortcut of the observation kernels, ssk::live_blocks(n_valid, len, t4) (csrc/ss_consts.hpp), checked
exhaustively and without a kernel: tests/live_host.cpp - a stand-alone program that includes ss_consts.hpp only, built with
AddressSanitizer and UBSan and run directly - prints the function for every n_valid in [0, len] of sixteen row lengths.

The truth comes from the STFT geometry alone.  Frame f covers positions 160 f .. 160 f + 511 of the centre-padded row; only the
taps of the zero-padded Hann window that are not zero count (asserted against the oracle's window: 56 zeros on each side, and
the periodic Hann's own first tap, position 56, is a 57th on the left); a padded position maps to a row sample as np.pad maps it
(reflect: as often as the row is short; constant: to no sample at all).  A pooled column is live when any such tap of any of
its four frames lands on a sample < n_valid, and the kernels must compute every column up to the last live one.

Asserted: live_blocks >= that truth at EVERY n_valid in [0, len], for both pad modes.  Not asserted, only recorded - how far the
formula sits above the truth (it ignores the window's zero taps and gives up, -> t4, once n_valid > len - 512).  Measured, the
largest excess in columns over n_valid in [0, len], reflect / constant:

    len     257    400   4000   8000  11025  16000  16384  16385  20000  22050  32000  32768  32769  44100  48000  49152
    t4        1      1      7     13     18     26     26     26     32     35     51     52     52     69     76     77
    reflect   1      1      1      1      1      1      1      1      1      1      1      1      1      1      1      1
    constant  1      1      1      1      1      1      1      1      1      1      1      1      1      1      1      1

Never more than one column: at n_valid = 0 (the formula says 1, nothing is live), and wherever the only taps of the last
counted column over rendered samples are zero taps, n_valid in (640 k - 256, 640 k - 199].  The formula is exact at about
nine values of n_valid in ten (44 100: 40 224 of 44 101); giving up behind len - 512 costs nothing here, the last column
is live there anyway.  test_excess_is_recorded prints the figures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import ss_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
LENS = [257, 400, 4000, 8000, 11025, 16000, 16384, 16385, 20000, 22050, 32000, 32768, 32769, 44100, 48000, 49152]
PADS = ("reflect", "constant")
NFFT, HOP, POOL = 512, 160, 4


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{len: (t4, live_blocks[0 .. len])} as the header computes it"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("live") / "live_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "live_host.cpp"), "-o", out])
    r = subprocess.run([out] + [str(n) for n in LENS], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {}
    for ln in r.stdout.splitlines():
        v = np.array(ln.split(), np.int64)
        got[int(v[0])] = (int(v[1]), v[2:])
    assert sorted(got) == sorted(LENS) and all(len(got[n][1]) == n + 1 for n in LENS)
    return got


def nonzero_taps():
    w = O.stft_window()
    assert w.shape == (NFFT,)
    assert not w[:56].any() and not w[-56:].any()            # the 56 zero taps on each side of the 400-tap window
    assert w[56] == 0.0 and (w[57:456] != 0).all()           # ... and the periodic Hann's own zero first tap
    return np.nonzero(w)[0]


def live_true(n, pad):
    """-> (t4, live[0 .. n]): 1 + the last pooled column with a non-zero-weight tap over a sample < n_valid (0: none)"""
    taps = nonzero_taps()
    n_frames = 1 + n // HOP
    t4 = (n_frames + POOL - 1) // POOL
    far = n + 1                                              # "no sample": never < n_valid
    if pad == "reflect":
        sample = np.pad(np.arange(n), NFFT // 2, mode="reflect")
    else:
        sample = np.pad(np.arange(n), NFFT // 2, mode="constant", constant_values=far)
    first = sample[HOP * np.arange(n_frames)[:, None] + taps[None, :]].min(axis=1)       # frames x taps -> earliest sample read
    first = np.concatenate([first, np.full(POOL * t4 - n_frames, far)]).reshape(t4, POOL).min(axis=1)
    live = np.zeros(n + 2, np.int64)
    np.maximum.at(live, np.minimum(first + 1, n + 1), np.arange(1, t4 + 1))              # column b is live from n_valid = first + 1 on
    return t4, np.maximum.accumulate(live)[:n + 1]


def test_truth_against_the_oracle_spectrogram():
    """the truth itself, against what it models: columns of compute_spectrogram of a noise row zeroed from n_valid on"""
    rng = np.random.default_rng(1)
    for n, pad in ((4000, "reflect"), (4000, "constant"), (400, "reflect"), (257, "constant")):
        x = rng.standard_normal((2, n))
        t4, live = live_true(n, pad)
        for nv in sorted({0, 1, 2, 57, 58, 184, 185, 200, 384, 385, 441, 442, 1024, n - 512, n - 456, n - 455, n - 1, n} & set(range(n + 1))):
            y = x.copy()
            y[:, nv:] = 0.0
            sg = O.compute_spectrogram(y, pad_mode=pad)
            assert sg.shape[1] == t4
            cols = np.nonzero(np.abs(sg).max(axis=(0, 2)) > 0)[0]
            assert (cols.max() + 1 if len(cols) else 0) == live[nv], (n, pad, nv)


@pytest.mark.parametrize("pad", PADS)
def test_live_blocks_covers_every_live_column_at_every_n_valid(table, pad):
    for n in LENS:
        t4, got = table[n]
        t4_true, want = live_true(n, pad)
        assert t4 == t4_true
        assert (got <= t4).all() and (got >= 0).all() and (np.diff(got) >= 0).all(), n
        short = np.nonzero(got < want)[0]
        assert not len(short), f"len={n} {pad}: live_blocks {got[short[0]]} < {want[short[0]]} live columns at n_valid={short[0]}"


def test_excess_is_recorded(table):
    """information, not a bound: how far live_blocks sits above the truth (the figures of the module docstring)"""
    for pad in PADS:
        row = []
        for n in LENS:
            t4, got = table[n]
            excess = got - live_true(n, pad)[1]
            at = int(np.argmax(excess))
            row.append(int(excess.max()))
            print(f"[live_blocks] len={n} t4={t4} {pad}: largest excess {excess.max()} column(s), first at n_valid={at}; "
                  f"exact at {int((excess == 0).sum())} of {n + 1} values")
        print(f"[live_blocks] {pad}: " + " ".join(str(v) for v in row))
