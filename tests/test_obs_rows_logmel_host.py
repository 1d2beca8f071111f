"""Log-mel form of the fused row kernels for rows of 2 or 3 partition blocks (k_obs_rows<.., MEL> / k_obs_blocks<.., MEL>:
convolution -> framing -> window -> rFFT -> |.|^2 -> mel bands -> log in one launch, no waveform buffer), compiled for the host on
the host-sim fibers, against the oracle: compute_logmel of compute_audiogoal zeroed from n_valid on.  44.1 and 48 kHz and one
two-block length (32768), both bank forms, both kernels, both pad modes, 64 and 40 bands, with and without the pooled spectrogram
and the waveform, silent / empty-RIR / steady-branch / distractor units in one batch, n_valid < out_len, fewer workgroups than
rows, rows split over 2 and 4 workgroups.
Tolerances: the project's log-mel rule (tests/test_obs_logmel_host.py::_check_mel, 1e-4 of the largest value per unit) and
relerr <= 1e-4 for the pooled spectrogram.  On these inputs today's two-step host path (hs.run(row_wgs=2) then hs.logmel) sits at
<= 1.4e-5 (44.1 kHz) and <= 5.9e-5 (48 kHz, the distractor unit: the convolution's fp32 rounding) against the same oracle expression.
Every output is pre-filled with NaN, every unit is compared, nothing is masked out."""
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
def mel_lib(tmp_path_factory):
    so = hs.build_driver("obs_rows_logmel", tmp_path_factory.mktemp("obs_rows_logmel"))
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hs_obs_rows_logmel.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float,
                                       ci, ci, ci, ci, ci, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    lib.hs_rir_spectra.argtypes = [vp, vp, ci, ctypes.c_longlong, ci, ci]
    return lib


def _plan(sources, units, cap, n_valid):
    """window descriptors + unit descriptors of a launch, as hostsim.hs.run plans them"""
    nbh_max = max(1, P.ceil_div(cap, P.KB))
    nby = max(1, P.ceil_div(n_valid, P.KB))
    offs = np.cumsum([0] + [len(s) for s in sources])
    cache, rows = {}, []

    def slot_of(sound, t0):
        if (sound, t0) not in cache:
            ws = P.plan_window_set(len(sources[sound]), t0, nbh_max, nby, False)
            cache[(sound, t0)] = (sum(len(r) for r in rows), ws)
            rows.append(P.window_desc_rows(ws, int(offs[sound]), len(sources[sound]), False))
        return cache[(sound, t0)]

    desc = np.zeros((len(units), 8), np.int32)
    for n, u in enumerate(units):
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


def _run(lib, sr, sources, bank, lens, units, *, n_valid=None, blocks=False, spectral=False, pad_mode=0, n_mels=64,
         want_sg=True, want_wave=False, wgs=2, parts_log2=0):
    """-> (logmel [N, n_mels, T, 2], spectrogram [N, 65, T4, 2] | None, audiogoal | None), every output pre-filled with NaN"""
    n_valid = sr if n_valid is None else n_valid
    bank = np.ascontiguousarray(bank, np.float32)
    R, _, cap = bank.shape
    wd, desc = _plan(sources, units, cap, n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in sources]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    hb = P.ceil_div(cap, P.KB)
    dev_bank = bank
    if spectral:
        dev_bank = np.zeros((R, 2, hb, P.SPEC_FLOATS), np.float32)
        assert lib.hs_rir_spectra(bank.ctypes.data, dev_bank.ctypes.data, R, 2 * cap, cap, cap) == 0
    start, w, max_len = P.mel_filterbank_sparse(sr, n_mels)
    start = np.ascontiguousarray(start, np.int32)
    w = np.ascontiguousarray(w, np.float32)
    N = len(units)
    T, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    mel = np.full((N, n_mels, T, 2), np.nan, np.float32)
    sg = np.full((N, 65, t4, 2), np.nan, np.float32) if want_sg else None
    wave = np.full((N, 2, sr), np.nan, np.float32) if want_wave else None
    rl = np.ascontiguousarray(lens, np.int32)
    no_dis = not any(u.get("dis_rir", -1) >= 0 for u in units)
    rc = lib.hs_obs_rows_logmel(int(blocks), int(spectral), spec.ctypes.data, dev_bank.ctypes.data, rl.ctypes.data,
                                desc.ctypes.data, wave.ctypes.data if want_wave else None, sg.ctypes.data if want_sg else None,
                                mel.ctypes.data, start.ctypes.data, w.ctypes.data, n_mels, max_len, EPS, N, cap, hb, n_valid, sr,
                                pad_mode, wgs, parts_log2, int(no_dis))
    assert rc == 0, rc
    return mel, sg, wave


def _mel_err(got, ref):
    assert got.shape == ref.shape and not np.isnan(got).any()
    return np.abs(got - ref).max() / np.abs(ref).max()


def _check_mel(got, ref):
    err = _mel_err(got, ref)
    assert err <= TOL, err


_INPUTS = {}


def _inputs(sr):
    """the inputs the 1e-4 rule was checked on: rng 23, a 1-s and a 3-s source, RIRs of sr / 30000 / 9001 taps (+ an empty one)"""
    if sr not in _INPUTS:
        rng = np.random.default_rng(23)
        srcs = [O.synth_sources(rng, sr, k=1, seconds=s)[0] for s in (1, 3)]
        lens = [sr, 30000, 9001, 0]
        bank = np.zeros((len(lens), 2, sr), np.float32)
        for i, L in enumerate(lens):
            if L:
                bank[i, :, :L] = O.synth_rir(rng, sr, length=L, n=1)[0]
        _INPUTS[sr] = (srcs, bank, lens)
    return _INPUTS[sr]


def _wav(row, L):
    return np.ascontiguousarray(row[:, :L].T)


def _units_and_refs(sr):
    """plain | silent | empty RIR | steady branch of the 3-s clip | distractor - the quiet ones in the middle of the batch"""
    srcs, bank, lens = _inputs(sr)
    t0 = P.window_start_sim(3 * sr, sr, 2)
    units = [dict(sound=0, t0=0, rir=0),
             dict(rir=-1),
             dict(sound=0, t0=0, rir=3),
             dict(sound=1, t0=t0, rir=1),
             dict(sound=0, t0=0, rir=2, dis_sound=1, dis_rir=1)]
    key = ("refs", sr)
    if key not in _INPUTS:
        _INPUTS[key] = [O.compute_audiogoal(srcs[0], _wav(bank[0], lens[0]), sr), None, None,
                        O.compute_audiogoal(srcs[1], _wav(bank[1], lens[1]), sr, audio_index=2),
                        O.compute_audiogoal(srcs[0], _wav(bank[2], lens[2]), sr, distractor=srcs[1],
                                            distractor_rir=_wav(bank[1], lens[1]))]
    return units, _INPUTS[key]


def _check_all(sr, mel, sg, wave, refs, n_valid, pad_mode, n_mels, tag):
    assert not np.isnan(mel).any() and (sg is None or not np.isnan(sg).any()), tag
    for k, a in enumerate(refs):
        if a is None:                                    # silent / empty RIR: zero power in every band, exact zeros pooled
            assert np.allclose(mel[k], np.log(EPS), rtol=1e-6), (tag, k)
            assert sg is None or not sg[k].any(), (tag, k)
            assert wave is None or not wave[k, :, :n_valid].any(), (tag, k)
            continue
        a = np.array(a, np.float32)
        a[:, n_valid:] = 0.0
        ref = O.compute_logmel(a, sr, n_mels=n_mels, eps=EPS, pad_mode=PAD_NAME[pad_mode])
        err = _mel_err(mel[k], ref)
        print(f"{tag} unit {k}: log-mel err {err:.3g}")
        assert err <= TOL, (tag, k, err)
        if sg is not None:
            e = O.relerr(sg[k], O.compute_spectrogram(a, pad_mode=PAD_NAME[pad_mode]))
            assert e <= TOL, (tag, k, e)
        if wave is not None:
            assert not np.isnan(wave[k, :, :n_valid]).any() and O.relerr(wave[k, :, :n_valid], a[:, :n_valid]) <= 1e-5, (tag, k)


# (pad_mode, n_mels, want_sg, want_wave) per (kernel, bank form): every value of each on both kernels and both bank forms
_OPTS = {(False, False): (0, 64, True, False), (False, True): (1, 40, False, True),
         (True, False): (1, 40, True, True), (True, True): (0, 64, False, False)}


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
@pytest.mark.parametrize("blocks", [False, True], ids=["rows", "blocks"])
@pytest.mark.parametrize("sr", [44100, 48000])
def test_rows_logmel_vs_oracle(mel_lib, sr, blocks, spectral):
    srcs, bank, lens = _inputs(sr)
    units, refs = _units_and_refs(sr)
    pad_mode, n_mels, want_sg, want_wave = _OPTS[(blocks, spectral)]
    if sr == 48000:                                      # the other half of the option table at the other rate
        pad_mode, n_mels, want_sg, want_wave = 1 - pad_mode, 104 - n_mels, not want_sg, not want_wave
    mel, sg, wave = _run(mel_lib, sr, srcs, bank, lens, units, blocks=blocks, spectral=spectral, pad_mode=pad_mode, n_mels=n_mels,
                         want_sg=want_sg, want_wave=want_wave, wgs=3)
    _check_all(sr, mel, sg, wave, refs, sr, pad_mode, n_mels, f"{sr} blocks={blocks} spectral={spectral}")


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
@pytest.mark.parametrize("blocks", [False, True], ids=["rows", "blocks"])
@pytest.mark.parametrize("parts_log2", [1, 2])
def test_rows_logmel_split_over_parts(mel_lib, parts_log2, blocks, spectral):
    """a row on 2 / 4 workgroups: every part writes the log-mel frames (and pooled columns) of its own pooled blocks only"""
    sr = 44100
    srcs, bank, lens = _inputs(sr)
    units, refs = _units_and_refs(sr)
    sel = [0, 1, 4] if parts_log2 == 1 else [2, 3]       # (between them: every kind of unit)
    want_sg = parts_log2 == 1
    mel, sg, _ = _run(mel_lib, sr, srcs, bank, lens, [units[k] for k in sel], blocks=blocks, spectral=spectral,
                      n_mels=64 if spectral else 40, want_sg=want_sg, parts_log2=parts_log2)
    _check_all(sr, mel, sg, None, [refs[k] for k in sel], sr, 0, 64 if spectral else 40, f"parts {parts_log2} blocks={blocks}")


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_rows_logmel_one_workgroup_walks_every_row(mel_lib, spectral):
    """wgs = 1: one workgroup renders all ten rows one after the other and reuses the collection buffer"""
    sr = 44100
    srcs, bank, lens = _inputs(sr)
    units, refs = _units_and_refs(sr)
    mel, sg, _ = _run(mel_lib, sr, srcs, bank, lens, units, spectral=spectral, pad_mode=1, want_sg=not spectral, wgs=1)
    _check_all(sr, mel, sg, None, refs, sr, 1, 64, f"wgs 1 spectral={spectral}")


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_rows_logmel_short_step(mel_lib, spectral):
    """n_valid = 27000 < out_len on k_obs_rows: the frames of the pooled blocks behind it are log(eps), written not computed"""
    sr, n_valid = 44100, 27000
    srcs, bank, lens = _inputs(sr)
    units, refs = _units_and_refs(sr)
    mel, sg, wave = _run(mel_lib, sr, srcs, bank, lens, units, n_valid=n_valid, spectral=spectral, want_sg=True, want_wave=True,
                         wgs=3)
    _check_all(sr, mel, sg, wave, refs, n_valid, 0, 64, f"n_valid {n_valid} spectral={spectral}")
    first_quiet = 4 * P.live_pooled_blocks(n_valid, sr)      # 43 of 69 pooled blocks are live
    assert first_quiet < mel.shape[2] and np.allclose(mel[0][:, first_quiet:], np.log(EPS), rtol=1e-6)


@pytest.mark.parametrize("blocks", [False, True], ids=["rows", "blocks"])
def test_rows_logmel_two_block_rows(mel_lib, blocks):
    """out_len = 32768: two partition blocks, phases of 25 + 27 pooled blocks (the collection buffer's widest phase)"""
    sr = 32768
    rng = np.random.default_rng(23)
    srcs = [O.synth_sources(rng, sr, k=1, seconds=1)[0]]
    lens = [sr, 9001]
    bank = np.zeros((2, 2, sr), np.float32)
    for i, L in enumerate(lens):
        bank[i, :, :L] = O.synth_rir(rng, sr, length=L, n=1)[0]
    units = [dict(sound=0, t0=0, rir=0), dict(rir=-1), dict(sound=0, t0=0, rir=1)]
    refs = [O.compute_audiogoal(srcs[0], _wav(bank[0], sr), sr), None, O.compute_audiogoal(srcs[0], _wav(bank[1], 9001), sr)]
    for spectral in (False, True):
        mel, sg, wave = _run(mel_lib, sr, srcs, bank, lens, units, blocks=blocks, spectral=spectral, want_sg=True,
                             want_wave=True, wgs=2)
        _check_all(sr, mel, sg, wave, refs, sr, 0, 64, f"32768 blocks={blocks} spectral={spectral}")


def test_rows_logmel_vs_feature_kernel_on_the_same_waveform(mel_lib):
    """the fused values against hs.logmel (k_logmel) of the waveform the SAME launch wrote: the two STFT implementations on
    identical samples (16 kHz form: 7.7e-7)"""
    sr = 44100
    srcs, bank, lens = _inputs(sr)
    units, refs = _units_and_refs(sr)
    worst = 0.0
    for blocks in (False, True):
        mel, _, wave = _run(mel_lib, sr, srcs, bank, lens, units, blocks=blocks, want_sg=False, want_wave=True, wgs=3)
        ref = hs.logmel(wave, sr, n_mels=64, eps=EPS, pad_mode=0)
        for k in range(len(units)):
            worst = max(worst, _mel_err(mel[k], ref[k]))
    print(f"fused log-mel vs k_logmel of the same waveform: {worst:.3g}")
    assert worst <= TOL, worst
