"""Log-mel form of the fused observation kernels (k_conv<.., MEL> / k_conv_spec<.., MEL>: convolution -> framing -> window ->
rFFT -> |.|^2 -> mel bands -> log in one launch, no waveform buffer), compiled for the host on the host-sim fibers, against the
oracle: compute_logmel of compute_audiogoal zeroed from n_valid on.  16 kHz, both bank forms, loop-free and loop kernels, both
pad modes, 64 and 40 bands, whole and short (n_valid 4000) steps; the pooled spectrogram of the same launch where asked.
Tolerances: the project's log-mel rule (tests/test_logmel.py::check, 1e-4 of the largest value) and relerr <= 1e-4 for the pooled
spectrogram; today's two-step host path sits at 6.1e-6 against the same oracle expression."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 16000
TOL = 1e-4
EPS = 1e-6
PAD_NAME = {0: "reflect", 1: "constant"}


@pytest.fixture(scope="module")
def mel_lib(tmp_path_factory):
    so = hs.build_driver("obs_logmel", tmp_path_factory.mktemp("obs_logmel"))
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hs_obs_logmel.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float, ci, ci, ci, ci, ci, ci]
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


def _run(lib, sources, bank, lens, units, n_valid, spectral, simple, pad_mode, n_mels, want_sg, want_wave=False):
    """-> (logmel [N, n_mels, T, 2], spectrogram [N, 65, T4, 2] | None, audiogoal | None), every output pre-filled with NaN"""
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
    start, w, max_len = P.mel_filterbank_sparse(SR, n_mels)
    start = np.ascontiguousarray(start, np.int32)
    w = np.ascontiguousarray(w, np.float32)
    N = len(units)
    T, t4 = 1 + SR // 160, P.spectrogram_shape(SR)[1]
    mel = np.full((N, n_mels, T, 2), np.nan, np.float32)
    sg = np.full((N, 65, t4, 2), np.nan, np.float32) if want_sg else None
    wave = np.full((N, 2, SR), np.nan, np.float32) if want_wave else None
    rl = np.ascontiguousarray(lens, np.int32)
    rc = lib.hs_obs_logmel(int(spectral), int(simple), spec.ctypes.data, dev_bank.ctypes.data, rl.ctypes.data, desc.ctypes.data,
                           wave.ctypes.data if want_wave else None, sg.ctypes.data if want_sg else None, mel.ctypes.data,
                           start.ctypes.data, w.ctypes.data, n_mels, max_len, EPS, N, cap, hb, n_valid, SR, pad_mode)
    assert rc == 0, rc
    return mel, sg, wave


def _check_mel(got, ref):
    assert got.shape == ref.shape and not np.isnan(got).any()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= TOL, err


def _inputs():
    rng = np.random.default_rng(5)
    srcs = list(O.synth_sources(rng, SR, k=2, seconds=1)) + [O.synth_sources(rng, SR, k=1, seconds=3)[0]]
    lens = [SR, SR, 0, 9000]
    bank = np.zeros((len(lens), 2, SR), np.float32)
    for i, L in enumerate(lens):
        if L:
            bank[i, :, :L] = O.synth_rir(rng, SR, length=L, n=1)[0]
    long_len = 40000                                                   # three partition blocks, every one audible
    long_bank = np.zeros((2, 2, long_len), np.float32)
    long_bank[0] = O.synth_rir_blocks(rng, SR, long_len, n=1)[0]
    long_bank[1, :, :SR] = bank[1]
    return srcs, bank, lens, long_bank, [long_len, SR]


def _zeroed(a, n_valid):
    a = np.array(a, np.float32)
    a[:, n_valid:] = 0.0
    return a


def _wav(row, L):
    return np.ascontiguousarray(row[:, :L].T)


@pytest.mark.parametrize("n_valid", [SR, 4000])
@pytest.mark.parametrize("n_mels", [64, 40])
@pytest.mark.parametrize("pad_mode", [0, 1])
@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_fused_logmel_vs_oracle(mel_lib, spectral, pad_mode, n_mels, n_valid):
    srcs, bank, lens, _, _ = _inputs()
    plain = [dict(sound=0, t0=0, rir=0),                 # plain unit
             dict(rir=-1),                               # silent unit
             dict(sound=1, t0=0, rir=2),                 # empty RIR
             dict(sound=1, t0=0, rir=3)]                 # ragged RIR (9000 taps)
    refs = [O.compute_audiogoal(srcs[0], _wav(bank[0], SR), SR), None, None,
            O.compute_audiogoal(srcs[1], _wav(bank[3], 9000), SR)]
    loop = plain + [dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=3)]          # a distractor term: the loop form
    refs_loop = refs + [O.compute_audiogoal(srcs[0], _wav(bank[1], SR), SR, distractor=srcs[1],
                                            distractor_rir=_wav(bank[3], 9000))]
    want_sg = (n_mels == 64) == (pad_mode == 0)          # half of the cases also ask for the pooled spectrogram
    for simple, units, ref_a in ((True, plain, refs), (False, loop, refs_loop)):
        mel, sg, _ = _run(mel_lib, srcs, bank, lens, units, n_valid, spectral, simple, pad_mode, n_mels, want_sg)
        assert not np.isnan(mel).any() and (sg is None or not np.isnan(sg).any())
        for k, a in enumerate(ref_a):
            if a is None:                                # silent / empty RIR: zero power in every band, exact zeros pooled
                assert np.allclose(mel[k], np.log(EPS), rtol=1e-6), (simple, k)
                assert sg is None or not sg[k].any()
                continue
            a = _zeroed(a, n_valid)
            _check_mel(mel[k], O.compute_logmel(a, SR, n_mels=n_mels, eps=EPS, pad_mode=PAD_NAME[pad_mode]))
            if sg is not None:
                assert O.relerr(sg[k], O.compute_spectrogram(a, pad_mode=PAD_NAME[pad_mode])) <= TOL, (simple, k)


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_fused_logmel_multi_block_rir_on_the_loop_form(mel_lib, spectral):
    """a 40000-tap RIR (three partition blocks, synth_rir_blocks: every block audible) under a 3-s clip in its steady branch,
    next to a one-block unit of the same launch; the waveform is written as well and must match the oracle's"""
    srcs, _, _, long_bank, long_lens = _inputs()
    t0 = P.window_start_sim(3 * SR, SR, 2)
    units = [dict(sound=2, t0=t0, rir=0), dict(sound=0, t0=0, rir=1)]
    mel, sg, wave = _run(mel_lib, srcs, long_bank, long_lens, units, SR, spectral, False, 0, 64, True, want_wave=True)
    refs = [O.compute_audiogoal(srcs[2], _wav(long_bank[0], long_lens[0]), SR, audio_index=2),
            O.compute_audiogoal(srcs[0], _wav(long_bank[1], SR), SR)]
    for k, a in enumerate(refs):
        a = np.array(a, np.float32)
        assert not np.isnan(wave[k]).any() and O.relerr(wave[k], a) <= 1e-5
        _check_mel(mel[k], O.compute_logmel(a, SR, n_mels=64, eps=EPS))
        assert O.relerr(sg[k], O.compute_spectrogram(a)) <= TOL
