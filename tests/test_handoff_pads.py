"""The row -> LDS hand-off of the fused observation kernels (fused_stft_phase, csrc/ss_kernels.hpp) materialises librosa's two
centre pads around the row: reflect (excluding the edge sample) or zeros, of the row as it is zeroed behind n_valid.
What can go wrong there is an O(1) error in the first or last frames - a mirrored sample off by one, the edge sample included,
a sample behind n_valid mirrored instead of a zero, a pad missing in the workgroup of a split row that needs it - so every case
compares the fused spectrogram with k_spectrogram run over the waveform of the NON-fused launch of the same units, and with the
oracle, and looks at the first two and last two pooled columns on their own.

Tolerances: the oracle at the suite's 1e-4 (max error over max magnitude).  Fused against two launches: both evaluate the
same fp32 convolution and the same 512-point fp32 transform in different kernels (butterfly order, one against two rounds of
rounding through memory): 1e-5 of the largest value, the bound tests/test_context.py already holds the two routes to - a wrong
pad sample is four orders of magnitude above it."""
import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

DEV = "cuda:0"
RTOL_ROUTES = 1e-5
RTOL_ORACLE = 1e-4


def close(got, ref, rtol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    den = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got - ref).max()) / den
    assert err <= rtol, f"{what}: {err:.3e}"


def check_columns(got, ref, rtol, what):
    """[.., 65, T4, 2]: the columns that hold the padded frames on their own, then everything"""
    t4 = got.shape[-2]
    for col in (0, 1, t4 - 2, t4 - 1):
        close(got[..., col, :], ref[..., col, :], rtol * float(np.abs(ref).max()) / max(float(np.abs(ref[..., col, :]).max()), 1e-30),
              f"{what}, pooled column {col}")
    close(got, ref, rtol, what)


def make(sr, n_src, n_rir, seed):
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    rng = np.random.default_rng(seed)
    src = list(O.synth_sources(rng, sr, k=n_src))
    rirs = [np.ascontiguousarray(h.T) for h in O.synth_rir(rng, sr, n=n_rir)]
    r = BatchedAudioRenderer(sr, device=DEV)
    for i, s in enumerate(src):
        r.add_source(f"s{i}", s)
    r.set_rir_bank(RirBank.from_arrays(rirs, DEV))
    return r, src, rirs, rng


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [8000, 11025, 16000])            # out_len even / odd, on both sides of 2048-sample chunk seams
@pytest.mark.parametrize("n_units", [1, 3, 129])                # split rows (8 and 8 parts per row), one workgroup per row
def test_fused_spectrogram_equals_two_launches_and_oracle(sr, n_units):
    import torch
    from ss_amd import ops
    r, src, rirs, rng = make(sr, 3, 5, 1000 * n_units + sr)
    sound = rng.integers(0, 3, n_units)
    rir = rng.integers(0, 5, n_units)
    plan = r.plan_arrays(sound, np.zeros(n_units, np.int64), rir)
    shape = (n_units,) + P.spectrogram_shape(sr)
    picks = sorted({0, n_units - 1})
    full = {i: O.conv_window_fft(src[sound[i]], rirs[rir[i]], 0, sr) for i in picks}     # (computed once per case, read only)
    for spectral in (False, True):
        if spectral:
            r.rirs.build_spectra()
        for pad_mode in ("reflect", "constant"):
            # the whole row; an odd / even tail; a right pad that mirrors zeros; a left pad that mirrors past n_valid
            for n_valid in (sr, sr - 1, sr - 300, 255):
                what = f"sr={sr} units={n_units} spectral={spectral} {pad_mode} n_valid={n_valid}"
                sg = torch.full(shape, float("nan"), device=DEV)
                ag = torch.full((n_units, 2, sr), float("nan"), device=DEV)
                if spectral:
                    ops.audio_obs_spec_into(r._spec, r.rirs.spectra, r.rirs.lengths, plan.desc, None, sg, n_valid, sr, pad_mode,
                                            flags=plan.flags)
                    ops.fftconv_binaural_spec_into(r._spec, r.rirs.spectra, r.rirs.lengths, plan.desc, ag, n_valid, flags=plan.flags)
                else:
                    ops.audio_obs_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, None, sg, n_valid, sr, pad_mode, flags=plan.flags)
                    ops.fftconv_binaural_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag, n_valid, flags=plan.flags)
                two = ops.spectrogram(ag, pad_mode)
                got = sg.cpu().numpy()
                assert np.isfinite(got).all(), what
                check_columns(got, two.cpu().numpy(), RTOL_ROUTES, what + " vs k_spectrogram")
                for i in picks:
                    a = full[i].astype(np.float32).copy()
                    a[:, n_valid:] = 0.0
                    check_columns(got[i], O.compute_spectrogram(a, pad_mode=pad_mode), RTOL_ORACLE, what + f" unit {i} vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_wide_rows_of_a_soundspaces2_step_at_44k(pad_mode):
    """k_conv<.., WIDE>: 0.25 s of a 44.1 kHz row - no right edge, zeros behind the block"""
    import torch
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, RirBank, UnitRequest
    sr = 44100
    rng = np.random.default_rng(44)
    src = O.tile_short_source(O.synth_sources(rng, sr, k=1)[0], sr)
    rirs = [np.ascontiguousarray(O.synth_rir(rng, sr, length=L, n=1)[0].T) for L in (9000, 20000)]
    r = BatchedAudioRenderer(sr, device=DEV, pad_mode=pad_mode, step_time=0.25, wrap=True)
    r.add_source("s", src)
    r.set_rir_bank(RirBank.from_arrays(rirs, DEV))
    idx = [100, 30000, 50000]
    cur = [0, 1, 1]
    units = [UnitRequest(0, i, c, wrap=i - rirs[c].shape[0] >= 0) for i, c in zip(idx, cur)]
    plan = r.plan(units)
    assert P.wide_one_block(r.out_len, r.n_valid, False)
    _, sg = r.render(plan)
    two = ops.spectrogram(r.render_audiogoal(plan), pad_mode)
    torch.cuda.synchronize()
    got = sg.cpu().numpy()
    check_columns(got, two.cpu().numpy(), RTOL_ROUTES, f"WIDE {pad_mode} vs k_spectrogram")
    for n, (i, c) in enumerate(zip(idx, cur)):
        ref = O.convolve_with_rir(src, rirs[c], sr, i, 0.25)
        check_columns(got[n], O.compute_spectrogram(ref.astype(np.float32), pad_mode=pad_mode), RTOL_ORACLE,
                      f"WIDE {pad_mode} unit {n} vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("pad_mode,n_valid", [("reflect", 16000), ("constant", 15999), ("reflect", 15700), ("reflect", 255)])
def test_logmel_form_on_one_unit(pad_mode, n_valid):
    """k_conv<.., MEL> and k_conv_spec<.., MEL>: log-mel and pooled spectrogram of one unit from the same hand-off"""
    import torch
    from ss_amd import ops
    sr, n_mels, eps = 16000, 64, 1e-6
    r, src, rirs, rng = make(sr, 1, 1, 5 + n_valid)
    plan = r.plan_arrays(np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64))
    ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
    msd, mwd = torch.from_numpy(ms).to(DEV), torch.from_numpy(mw).to(DEV)
    a = O.conv_window_fft(src[0], rirs[0], 0, sr).astype(np.float32)
    a[:, n_valid:] = 0.0
    ref_sg, ref_lm = O.compute_spectrogram(a, pad_mode=pad_mode), O.compute_logmel(a, sr, n_mels, eps, pad_mode=pad_mode)
    ag = torch.empty((1, 2, sr), device=DEV)
    ops.fftconv_binaural_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag, n_valid, flags=plan.flags)
    two_sg = ops.spectrogram(ag, pad_mode).cpu().numpy()
    two_lm = torch.empty((1, n_mels, 1 + sr // 160, 2), device=DEV)
    ops.logmel_into(ag, two_lm, msd, mwd, eps, pad_mode)
    two_lm = two_lm.cpu().numpy()
    for spectral in (False, True):
        sg = torch.full((1,) + P.spectrogram_shape(sr), float("nan"), device=DEV)
        lm = torch.full((1, n_mels, 1 + sr // 160, 2), float("nan"), device=DEV)
        if spectral:
            r.rirs.build_spectra()
            ops.audio_obs_logmel_spec_into(r._spec, r.rirs.spectra, r.rirs.lengths, plan.desc, None, sg, lm, msd, mwd, n_valid, sr, eps,
                                           pad_mode, flags=plan.flags)
        else:
            ops.audio_obs_logmel_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, None, sg, lm, msd, mwd, n_valid, sr, eps,
                                      pad_mode, flags=plan.flags)
        what = f"MEL spectral={spectral} {pad_mode} n_valid={n_valid}"
        got_sg, got_lm = sg.cpu().numpy(), lm.cpu().numpy()
        check_columns(got_sg, two_sg, RTOL_ROUTES, what + " spectrogram vs k_spectrogram")
        check_columns(got_sg[0], ref_sg, RTOL_ORACLE, what + " spectrogram vs oracle")
        nf = got_lm.shape[2]
        for fr in (0, 1, nf - 2, nf - 1):                          # the frames that read a pad
            assert np.abs(got_lm[0][:, fr] - ref_lm[:, fr]).max() <= RTOL_ORACLE * np.abs(ref_lm).max(), (what, fr)
            assert np.abs(got_lm[0][:, fr] - two_lm[0][:, fr]).max() <= RTOL_ORACLE * np.abs(two_lm).max(), (what, fr)
        assert np.abs(got_lm[0] - ref_lm).max() <= RTOL_ORACLE * np.abs(ref_lm).max(), what
        assert np.abs(got_lm[0] - two_lm[0]).max() <= RTOL_ORACLE * np.abs(two_lm).max(), what
