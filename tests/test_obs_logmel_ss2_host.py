"""Log-mel form of the fused loop kernel on SoundSpaces 2.0 steps (k_conv<true, false, XFADE, false, WIDE, true>: the cross-faded
one-block row, and block 0 of a 44.1 / 48 kHz row with and without the cross-fade), compiled for the host on the host-sim fibers,
against the oracle: compute_logmel of compute_audiogoal_continuous.  Tolerances: the project's log-mel rule (1e-4 of the largest
value, tests/test_obs_logmel_host.py::_check_mel), relerr <= 1e-4 for the pooled spectrogram, 1e-5 for the waveform."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4
EPS = 1e-6
PAD_NAME = {0: "reflect", 1: "constant"}


@pytest.fixture(scope="module")
def ss2_lib(tmp_path_factory):
    so = hs.build_driver("obs_logmel_ss2", tmp_path_factory.mktemp("obs_logmel_ss2"))
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hs_obs_logmel_ss2.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float, ci, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    return lib


def _plan(sources, units, cap, n_valid, crossfade):
    """window descriptors + unit descriptors of a launch, as hostsim.hs.run plans them (units: see _unit)"""
    nbh_max = max(1, P.ceil_div(cap, P.KB))
    nby = max(1, P.ceil_div(n_valid, P.KB))
    offs = np.cumsum([0] + [len(s) for s in sources])
    cache, rows = {}, []

    def slot_of(sound, t0, wrap):
        key = (sound, t0, wrap)
        if key not in cache:
            ws = P.plan_window_set(len(sources[sound]), t0, nbh_max, nby, wrap)
            cache[key] = (sum(len(r) for r in rows), ws)
            rows.append(P.window_desc_rows(ws, int(offs[sound]), len(sources[sound]), wrap))
        return cache[key]

    desc = np.zeros((len(units), 8), np.int32)
    for n, u in enumerate(units):
        if u.get("rir", -1) < 0:
            desc[n] = P.unit_desc_row()
            continue
        s0, ws = slot_of(u["sound"], u["t0"], u["wrap"])
        if crossfade and u.get("last_rir", -1) >= 0:
            d0, dws = slot_of(u["sound"], u["t0"], u["last_wrap"])
            desc[n] = P.unit_desc_row(u["rir"], s0, ws, u["last_rir"], d0, dws)
        elif not crossfade and u.get("dis_rir", -1) >= 0:
            d0, dws = slot_of(u["dis_sound"], 0, False)
            desc[n] = P.unit_desc_row(u["rir"], s0, ws, u["dis_rir"], d0, dws)
        else:
            desc[n] = P.unit_desc_row(u["rir"], s0, ws)
    wd = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), np.int32), np.int32)
    return wd, desc


def _run(lib, sr, sources, bank, lens, units, n_valid, crossfade, pad_mode, n_mels, want_sg, want_wave=False):
    """-> (logmel [N, n_mels, T, 2], spectrogram [N, 65, T4, 2] | None, audiogoal | None), every output pre-filled with NaN"""
    assert len(units) <= 4
    bank = np.ascontiguousarray(bank, np.float32)
    cap = bank.shape[2]
    wd, desc = _plan(sources, units, cap, n_valid, crossfade)
    flat = np.concatenate([np.asarray(s, np.float32) for s in sources]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    start, w, max_len = P.mel_filterbank_sparse(sr, n_mels)
    start = np.ascontiguousarray(start, np.int32)
    w = np.ascontiguousarray(w, np.float32)
    N = len(units)
    T, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    mel = np.full((N, n_mels, T, 2), np.nan, np.float32)
    sg = np.full((N, 65, t4, 2), np.nan, np.float32) if want_sg else None
    wave = np.full((N, 2, sr), np.nan, np.float32) if want_wave else None
    rl = np.ascontiguousarray(lens, np.int32)
    rc = lib.hs_obs_logmel_ss2(int(crossfade), spec.ctypes.data, bank.ctypes.data, rl.ctypes.data, desc.ctypes.data,
                               wave.ctypes.data if want_wave else None, sg.ctypes.data if want_sg else None, mel.ctypes.data,
                               start.ctypes.data, w.ctypes.data, n_mels, max_len, EPS, N, cap, n_valid, sr, pad_mode)
    assert rc == 0, rc
    assert not np.isnan(mel).any() and (sg is None or not np.isnan(sg).any()) and (wave is None or not np.isnan(wave).any())
    return mel, sg, wave


def _check_mel(got, ref):
    assert got.shape == ref.shape and not np.isnan(got).any()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= TOL, err


_INPUTS = {}


def _inputs(sr, lens):
    """a 1-s clip tiled x3 (as the reference loads it), a second clip for distractor terms, and a bank of RIRs of `lens` taps
    (0: an empty RIR) - computed once per (sr, lens) and never written to"""
    key = (sr, tuple(lens))
    if key not in _INPUTS:
        rng = np.random.default_rng(23)
        a, b = O.synth_sources(rng, sr, k=2, seconds=1)
        bank = np.zeros((len(lens), 2, max(lens)), np.float32)
        for i, L in enumerate(lens):
            if L:
                bank[i, :, :L] = O.synth_rir(rng, sr, length=L, n=1)[0]
        _INPUTS[key] = ([O.tile_short_source(a, sr), b], bank)
    return _INPUTS[key]


def _wav(bank, lens, i):
    return np.ascontiguousarray(bank[i][:, :lens[i]].T)


def _unit(lens, sample_index, rir, last_rir=-1, **kw):
    """a unit at `sample_index` of the tiled clip: the steady branch (which wraps around the clip end) once the index has
    passed the RIR's length, per RIR (continuous_simulator.py:433)"""
    u = dict(sound=0, t0=P.window_start_continuous(sample_index), rir=rir, wrap=sample_index - lens[rir] >= 0, index=sample_index,
             last_rir=last_rir, **kw)
    if last_rir >= 0:
        u["last_wrap"] = sample_index - lens[last_rir] >= 0
    return u


def _reference(sr, srcs, bank, lens, u, n_valid, crossfade):
    """the oracle's row of a unit, None for a silent unit or an empty RIR without a previous one"""
    if u.get("rir", -1) < 0 or (lens[u["rir"]] == 0 and u.get("last_rir", -1) < 0):
        return None
    step_time = (n_valid + 0.5) / sr
    assert int(sr * step_time) == n_valid
    last = _wav(bank, lens, u["last_rir"]) if crossfade and u.get("last_rir", -1) >= 0 else None
    a = O.compute_audiogoal_continuous(srcs[0], _wav(bank, lens, u["rir"]), sr, u["index"], step_time, last_rir=last,
                                       use_crossfade=crossfade)
    if not crossfade and u.get("dis_rir", -1) >= 0:          # a distractor term: the second clip from its start, added
        a = a + O.convolve_with_rir(srcs[1], _wav(bank, lens, u["dis_rir"]), sr, 0, step_time)
    return np.asarray(a, np.float32)


def _check_launch(sr, out, srcs, bank, lens, units, n_valid, crossfade, pad_mode, n_mels):
    mel, sg, wave = out
    live = P.live_pooled_blocks(n_valid, sr)
    for k, u in enumerate(units):
        a = _reference(sr, srcs, bank, lens, u, n_valid, crossfade)
        if a is None:                                        # zero power in every band, exact zeros pooled
            assert np.allclose(mel[k], np.log(EPS), rtol=1e-6), k
            assert sg is None or not sg[k].any()
            assert wave is None or not wave[k].any()
            continue
        assert not a[:, n_valid:].any()
        _check_mel(mel[k], O.compute_logmel(a, sr, n_mels=n_mels, eps=EPS, pad_mode=PAD_NAME[pad_mode]))
        assert np.allclose(mel[k][:, 4 * live:], np.log(EPS), rtol=1e-6), k       # frames behind the live blocks
        if sg is not None:
            assert O.relerr(sg[k], O.compute_spectrogram(a, pad_mode=PAD_NAME[pad_mode])) <= TOL, k
            assert not sg[k][:, live:].any()                                        # dead columns: exact zeros
        if wave is not None:
            assert O.relerr(wave[k], a) <= 1e-5, k


LENS16 = [9000, 12000, 20000, 0]          # the last RIR spans two partition blocks; entry 3 is empty


@pytest.mark.parametrize("n_mels", [64, 40])
@pytest.mark.parametrize("pad_mode", [0, 1])
def test_crossfaded_one_block_rows_vs_oracle(ss2_lib, pad_mode, n_mels):
    """16 kHz, 0.25 s of a 1-s row, SS_FLAG_CROSSFADE: sample indices in the early branch (100; 15000 for the 20000-tap RIR only)
    and the steady one (30000; 46000 wraps around the clip end); a unit without a previous RIR, a silent one and one with an
    empty RIR in the same launches"""
    sr, n_valid = 16000, 4000
    srcs, bank = _inputs(sr, LENS16)
    want_sg = (n_mels == 64) == (pad_mode == 0)          # half of the cases also ask for the pooled spectrogram
    want_wave = n_mels == 64 and pad_mode == 0           # ... and one for the waveform
    launches = [[_unit(LENS16, 100, 0, last_rir=1), _unit(LENS16, 15000, 2, last_rir=0), _unit(LENS16, 30000, 1), dict(rir=-1)],
                [_unit(LENS16, 46000, 0, last_rir=2), _unit(LENS16, 30000, 2, last_rir=1), _unit(LENS16, 15000, 1, last_rir=0),
                 _unit(LENS16, 46000, 3)]]
    for units in launches:
        out = _run(ss2_lib, sr, srcs, bank, LENS16, units, n_valid, True, pad_mode, n_mels, want_sg, want_wave)
        _check_launch(sr, out, srcs, bank, LENS16, units, n_valid, True, pad_mode, n_mels)
    # the blend is there: the first unit's head differs from the same unit rendered without its previous RIR
    plain = _run(ss2_lib, sr, srcs, bank, LENS16, [_unit(LENS16, 100, 0)], n_valid, True, pad_mode, n_mels, False)[0]
    faded = _run(ss2_lib, sr, srcs, bank, LENS16, launches[0][:1], n_valid, True, pad_mode, n_mels, False)[0]
    assert np.abs(plain[0][:, :4] - faded[0][:, :4]).max() > 1e-3
    assert np.abs(plain[0][:, 8:] - faded[0][:, 8:]).max() == 0.0      # frames that start behind the ramp (800 + 256 < 8 * 160)


LENS44 = [20000, 9000, 40000]


@pytest.mark.parametrize("crossfade", [True, False], ids=["crossfade", "plain"])
@pytest.mark.parametrize("pad_mode", [0, 1])
def test_block_0_of_a_44k_row_vs_oracle(ss2_lib, pad_mode, crossfade):
    """44.1 kHz, out_len 44100, n_valid 11025 (18 live pooled blocks of 69): frames behind the live blocks are log(eps), the
    pooled spectrogram's dead columns exact zeros; without the flag one unit carries a distractor term"""
    sr, n_valid = 44100, 11025
    srcs, bank = _inputs(sr, LENS44)
    units = [_unit(LENS44, 50000, 0, last_rir=2, dis_sound=1, dis_rir=1),     # previous RIR: 3 blocks, steady; or a distractor
             _unit(LENS44, 9000, 1, last_rir=0),                              # previous RIR in the early branch
             _unit(LENS44, 125000, 0),                                        # wraps around the clip end
             dict(rir=-1)]
    n_mels = 64 if pad_mode == 0 else 40
    out = _run(ss2_lib, sr, srcs, bank, LENS44, units, n_valid, crossfade, pad_mode, n_mels, True, want_wave=pad_mode == 1)
    assert P.live_pooled_blocks(n_valid, sr) == 18
    _check_launch(sr, out, srcs, bank, LENS44, units, n_valid, crossfade, pad_mode, n_mels)


@pytest.mark.parametrize("crossfade", [True, False], ids=["crossfade", "plain"])
def test_largest_wide_step_and_empty_step(ss2_lib, crossfade):
    """n_valid = KB at 44.1 kHz: 26 live blocks, the most the WIDE form accepts (the last frame of block 25 reads samples behind
    the block); n_valid = 0: every frame is log(eps)"""
    sr = 44100
    srcs, bank = _inputs(sr, LENS44)
    assert P.live_pooled_blocks(P.KB, sr) == 26
    units = [_unit(LENS44, 60000, 0, last_rir=1), _unit(LENS44, 60000, 1)]
    out = _run(ss2_lib, sr, srcs, bank, LENS44, units, P.KB, crossfade, 0, 64, True)
    _check_launch(sr, out, srcs, bank, LENS44, units, P.KB, crossfade, 0, 64)
    mel, sg, _ = _run(ss2_lib, sr, srcs, bank, LENS44, units, 0, crossfade, 0, 64, True)
    assert np.allclose(mel, np.log(EPS), rtol=1e-6) and not sg.any()


def test_crossfade_at_48k_near_the_ramp_cap(ss2_lib):
    """48 kHz, n_valid 12000, cross-faded: fade_len = 2400 of the 2414 the kernel keeps"""
    sr, n_valid = 48000, 12000
    lens = [20000, 12000]
    srcs, bank = _inputs(sr, lens)
    units = [_unit(lens, 70000, 0, last_rir=1), _unit(lens, 5000, 1, last_rir=0), _unit(lens, 70000, 1)]
    out = _run(ss2_lib, sr, srcs, bank, lens, units, n_valid, True, 0, 64, True, want_wave=True)
    _check_launch(sr, out, srcs, bank, lens, units, n_valid, True, 0, 64)
