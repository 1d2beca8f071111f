"""A wave's two pooled blocks as interleaved chains (stft_block_pair, ss_kernels.hpp) against the same two blocks run one after the
other: the host build of the kernels (tests/stft_pair_host.cpp = tests/hostsim/hostsim.cpp) compiled twice, as the product does and
with -DSS_NO_STFT_PAIR, run on the same launches.  The pair only changes the order in which a wave issues its work, so the pooled
spectrogram and the waveform of the two builds are compared BYTE FOR BYTE; each launch is also held to the oracle at the project's
1e-4.  Launches: every fused one-block route (time-domain and spectral rows, loop-free and loop form with a distractor term,
cross-fade, WIDE), rows with 26 / 25 / 17 / 16 live blocks (ten pairs + six singles, nine pairs, one pair on wave 0, no pair),
both pad modes, a silent unit and an empty RIR, a split row and an 8000-sample row (neither has a wave with two blocks)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4
PAD_NAME = {0: "reflect", 1: "constant"}
SR = 16000


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(pair, one after the other): the two host builds, compiled side by side"""
    d = tmp_path_factory.mktemp("stft_pair")
    procs, sos = [], []
    for name, extra in (("pair", []), ("nopair", ["-DSS_NO_STFT_PAIR"])):
        so = str(d / f"libss_stft_{name}_host.so")
        procs.append(subprocess.Popen(hs.driver_command("stft_pair", so, extra), cwd=HERE))
        sos.append(so)
    assert [p.wait() for p in procs] == [0, 0]
    pair, nopair = (ctypes.CDLL(so) for so in sos)
    assert pair.hs_stft_pair_enabled() == 1 and nopair.hs_stft_pair_enabled() == 0
    return pair, nopair


def _run(lib, *args, **kw):
    """hostsim.hs.run (descriptor planning included) on `lib` instead of the suite's shared host build"""
    old = hs._LIB
    hs._LIB = lib
    try:
        return hs.run(*args, **kw)
    finally:
        hs._LIB = old


def _both(libs, *args, **kw):
    """the launch on both builds: byte-equal outputs -> (waveform, pooled spectrogram) of the pair build"""
    (a1, s1), (a0, s0) = _run(libs[0], *args, **kw), _run(libs[1], *args, **kw)
    assert s1 is not None and not np.isnan(s1).any()
    assert s1.tobytes() == s0.tobytes()
    assert (a1 is None) == (a0 is None)
    if a1 is not None:
        assert not np.isnan(a1).any() and a1.tobytes() == a0.tobytes()
    return a1, s1


def _n_valid_for(lib, live, out_len=SR):
    """the largest n_valid whose row has `live` live pooled blocks, by ssk::live_blocks itself (block live - 1 then reads
    samples in front of n_valid: its column is not zero)"""
    t4 = P.spectrogram_shape(out_len)[1]
    return max(nv for nv in range(out_len + 1) if lib.hs_live_blocks(nv, out_len, t4) == live)


_INPUTS = {}


def _inputs(sr=SR, lens=(9000, 12000, 0)):
    """two 1-s clips and a bank of RIRs of `lens` taps (0: an empty RIR), made once per key and never written to"""
    key = (sr, tuple(lens))
    if key not in _INPUTS:
        rng = np.random.default_rng(31)
        srcs = list(O.synth_sources(rng, sr, k=2, seconds=1))
        bank = np.zeros((len(lens), 2, max(lens)), np.float32)
        for i, L in enumerate(lens):
            if L:
                bank[i, :, :L] = O.synth_rir(rng, sr, length=L, n=1)[0]
        _INPUTS[key] = (srcs, bank)
    return _INPUTS[key]


def _wav(bank, lens, i):
    return np.ascontiguousarray(bank[i][:, :lens[i]].T)


_REFS = {}


def _ref_row(sr, lens, rir, dis_rir=-1):
    """the oracle's 1-s row of clip 0 through RIR `rir` (+ clip 1 through `dis_rir`), computed once"""
    key = (sr, tuple(lens), rir, dis_rir)
    if key not in _REFS:
        srcs, bank = _inputs(sr, lens)
        kw = dict(distractor=srcs[1], distractor_rir=_wav(bank, lens, dis_rir)) if dis_rir >= 0 else {}
        _REFS[key] = np.asarray(O.compute_audiogoal(srcs[0], _wav(bank, lens, rir), sr, **kw), np.float32)
    return _REFS[key]


def _check(a, sg, ref, n_valid, pad_mode, live):
    ref = ref.copy()
    ref[:, n_valid:] = 0
    if a is not None:
        assert O.relerr(a, ref) <= 1e-5
    assert O.relerr(sg, O.compute_spectrogram(ref, pad_mode=PAD_NAME[pad_mode])) <= TOL
    assert not sg[:, live:].any()                           # dead columns: exact zeros


LENS = (9000, 12000, 0)


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
@pytest.mark.parametrize("pad_mode", [0, 1])
def test_full_row_ten_pairs_six_singles(libs, pad_mode, spectral):
    """16 000 samples, n_valid = out_len: 26 live blocks, waves 0..9 run a pair and waves 10..15 one block; a silent unit and an
    empty RIR ride in the time-domain launches"""
    srcs, bank = _inputs()
    assert libs[0].hs_live_blocks(SR, SR, 26) == 26
    t0 = P.window_start_sim(SR, SR, 0)
    units = [dict(sound=0, t0=t0, rir=0)]
    if not spectral:
        units += [dict(rir=-1), dict(sound=0, t0=t0, rir=2)]
    a, sg = _both(libs, srcs, bank, LENS, units, SR, SR, fuse=True, pad_mode=pad_mode, spectral=spectral)
    _check(a[0], sg[0], _ref_row(SR, LENS, 0), SR, pad_mode, 26)
    for k in range(1, len(units)):
        assert not a[k].any() and not sg[k].any()


@pytest.mark.parametrize("live,pad_mode,spectral", [(16, 0, True), (17, 1, True), (25, 0, False), (17, 0, False)])
def test_live_blocks_at_the_pair_threshold(libs, live, pad_mode, spectral):
    """n_valid by live_blocks(): 16 live blocks (no wave has a second one), 17 (wave 0 alone runs a pair), 25 (nine pairs)"""
    srcs, bank = _inputs()
    nv = _n_valid_for(libs[0], live)
    assert 0 < nv < SR
    units = [dict(sound=0, t0=P.window_start_sim(SR, SR, 0), rir=1)]
    a, sg = _both(libs, srcs, bank, LENS, units, nv, SR, fuse=True, pad_mode=pad_mode, spectral=spectral)
    assert not a[0][:, nv:].any()
    _check(a[0], sg[0], _ref_row(SR, LENS, 1), nv, pad_mode, live)
    assert sg[0][:, live - 1].any()


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_loop_form_with_a_distractor_term(libs, spectral):
    srcs, bank = _inputs()
    t0 = P.window_start_sim(SR, SR, 0)
    units = [dict(sound=0, t0=t0, rir=0, dis_sound=1, dis_t0=0, dis_rir=1)]
    a, sg = _both(libs, srcs, bank, LENS, units, SR, SR, fuse=True, simple=False, pad_mode=int(spectral), spectral=spectral)
    _check(a[0], sg[0], _ref_row(SR, LENS, 0, dis_rir=1), SR, int(spectral), 26)


def test_crossfaded_row(libs):
    """k_conv<FUSE, loop, XFADE> on a whole 1-s row: the previous RIR is term 1"""
    srcs, bank = _inputs()
    src3 = O.tile_short_source(srcs[0], SR)
    idx, step_time = 30000, (SR - 160 + 0.5) / SR           # steady branch for both RIRs; n_valid = 15 840 -> 26 live blocks
    nv = int(SR * step_time)
    assert libs[0].hs_live_blocks(nv, SR, 26) == 26
    units = [dict(sound=0, t0=P.window_start_continuous(idx), rir=0, wrap=True, last_rir=1, last_wrap=True)]
    a, sg = _both(libs, [src3], bank, LENS, units, nv, SR, fuse=True, crossfade=True)
    ref = np.asarray(O.compute_audiogoal_continuous(src3, _wav(bank, LENS, 0), SR, idx, step_time, last_rir=_wav(bank, LENS, 1),
                                                    use_crossfade=True), np.float32)
    _check(a[0], sg[0], ref, nv, 0, 26)


def test_wide_row_26_live_blocks(libs):
    """k_conv<FUSE, loop, .., WIDE>: block 0 of a 44.1 kHz row, n_valid = kB: the 26 blocks the form can hold"""
    sr, lens = 44100, (20000,)
    srcs, bank = _inputs(sr, lens)
    src3 = O.tile_short_source(srcs[0], sr)
    nv, idx = P.KB, 60000
    step_time = (nv + 0.5) / sr
    assert int(sr * step_time) == nv and libs[0].hs_live_blocks(nv, sr, P.spectrogram_shape(sr)[1]) == 26
    units = [dict(sound=0, t0=P.window_start_continuous(idx), rir=0, wrap=True)]
    a, sg = _both(libs, [src3], bank, lens, units, nv, sr, fuse=True, simple=False)
    ref = np.asarray(O.convolve_with_rir(src3, _wav(bank, lens, 0), sr, idx, step_time), np.float32)
    _check(a[0], sg[0], ref, nv, 0, 26)


def test_split_row_is_unchanged(libs):
    """parts_log2 = 1: a workgroup's share is 13 blocks, no wave has two"""
    srcs, bank = _inputs()
    units = [dict(sound=0, t0=P.window_start_sim(SR, SR, 0), rir=0)]
    a, sg = _both(libs, srcs, bank, LENS, units, SR, SR, fuse=True, parts_log2=1)
    _check(a[0], sg[0], _ref_row(SR, LENS, 0), SR, 0, 26)


def test_8000_sample_row_has_no_pairs(libs):
    sr, lens = 8000, (5000,)
    srcs, bank = _inputs(sr, lens)
    assert P.spectrogram_shape(sr)[1] <= 16
    units = [dict(sound=0, t0=P.window_start_sim(sr, sr, 0), rir=0)]
    a, sg = _both(libs, srcs, bank, lens, units, sr, sr, fuse=True)
    _check(a[0], sg[0], _ref_row(sr, lens, 0), sr, 0, P.spectrogram_shape(sr)[1])
