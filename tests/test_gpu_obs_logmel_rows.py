"""Log-mel observations of rows of 2 or 3 partition blocks (44.1 / 48 kHz) in one launch, without a waveform buffer:
ss_audio_obs_logmel_rows_f32 / _spec_f32 (k_obs_blocks<.., MEL> for small steps, k_obs_rows<.., MEL> beyond) against the oracle and
against today's two launches on the same kernel route, and the context route behind ss_ctx_set_logmel_rows_policy (default:
never - the scratch route, bit-equal to observe-then-features).  Tolerances: the project's log-mel rule (1e-4 of the largest
value per unit) and relerr <= 1e-4 for the pooled spectrogram.  Every output is pre-filled with NaN, every unit is compared.
Nothing here captures a graph (a k_obs_blocks launch must not be replayed from one)."""
import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
EPS = 1e-6
ALWAYS = (1, 2 ** 31 - 1)
_CACHE = {}


def _mel(sr, n_mels=64):
    ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
    return torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)


def _new(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _inputs(sr):
    """rng 23: a 1-s and a 3-s source; RIRs of sr / 30000 / 9001 taps (wav layout) and an empty file.  Unit kinds and their
    oracle waveforms: plain | steady branch of the 3-s clip | distractor | silent | empty RIR | plain through the short RIR"""
    if sr not in _CACHE:
        rng = np.random.default_rng(23)
        srcs = [O.synth_sources(rng, sr, k=1, seconds=s)[0] for s in (1, 3)]
        rirs = [np.ascontiguousarray(O.synth_rir(rng, sr, length=L, n=1)[0].T) for L in (sr, 30000, 9001)]
        rirs.append(np.zeros((0, 2), np.float32))
        t0 = P.window_start_sim(3 * sr, sr, 2)
        kinds = [dict(sound=0, t0=0, rir=0), dict(sound=1, t0=t0, rir=1), dict(sound=0, t0=0, rir=2, dis_sound=1, dis_rir=1),
                 dict(sound=0, t0=0, rir=-1), dict(sound=0, t0=0, rir=3), dict(sound=0, t0=0, rir=2)]
        waves = [O.compute_audiogoal(srcs[0], rirs[0], sr), O.compute_audiogoal(srcs[1], rirs[1], sr, audio_index=2),
                 O.compute_audiogoal(srcs[0], rirs[2], sr, distractor=srcs[1], distractor_rir=rirs[1]), None, None,
                 O.compute_audiogoal(srcs[0], rirs[2], sr)]
        _CACHE[sr] = (srcs, rirs, kinds, [None if a is None else np.asarray(a, np.float32) for a in waves])
    return _CACHE[sr]


def _ref_mel(sr, kind, n_mels, pad_mode="reflect"):
    key = ("mel", sr, kind, n_mels, pad_mode)
    if key not in _CACHE:
        a = _inputs(sr)[3][kind]
        _CACHE[key] = None if a is None else O.compute_logmel(a, sr, n_mels=n_mels, eps=EPS, pad_mode=pad_mode)
    return _CACHE[key]


def _ref_sg(sr, kind, pad_mode="reflect"):
    key = ("sg", sr, kind, pad_mode)
    if key not in _CACHE:
        a = _inputs(sr)[3][kind]
        _CACHE[key] = None if a is None else O.compute_spectrogram(a, pad_mode=pad_mode)
    return _CACHE[key]


def _kinds_of(n):
    """unit i of an n-unit step: every kind in turn (one unit: the plain one)"""
    return [(i + (n % 5)) % 6 if n > 1 else 0 for i in range(n)]


def _check_vs_oracle(sr, kinds, lm, sg, n_mels=64, pad_mode="reflect"):
    """every unit of the step against the oracle of its kind"""
    lm = lm.cpu().numpy()
    sg = None if sg is None else sg.cpu().numpy()
    assert not np.isnan(lm).any() and (sg is None or not np.isnan(sg).any())
    worst = 0.0
    for i, k in enumerate(kinds):
        ref = _ref_mel(sr, k, n_mels, pad_mode)
        if ref is None:                                  # silent / empty RIR: log(eps) everywhere, exact-zero spectrogram
            assert np.allclose(lm[i], np.log(EPS), rtol=1e-6), i
            assert sg is None or not sg[i].any(), i
            continue
        err = np.abs(lm[i] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= TOL, (i, k, err)
        if sg is not None:
            e = O.relerr(sg[i], _ref_sg(sr, k, pad_mode))
            assert e <= TOL, (i, k, e)
    print(f"sr {sr} n {len(kinds)}: worst log-mel error vs oracle {worst:.3g}")


def _renderer(sr):
    key = ("renderer", sr)
    if key not in _CACHE:
        from ss_amd.renderer import BatchedAudioRenderer, RirBank
        srcs, rirs, _, _ = _inputs(sr)
        r = BatchedAudioRenderer(sr, device=DEV)
        for i, c in enumerate(srcs):
            r.add_source(str(i), c)
        r.set_rir_bank(RirBank.from_arrays(rirs, DEV))
        r.rirs.build_spectra()
        _CACHE[key] = r
    return _CACHE[key]


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
@pytest.mark.parametrize("sr,n_units", [(44100, 1), (44100, 5), (44100, 42), (44100, 43), (44100, 128), (44100, 150),
                                        (48000, 5), (48000, 128)])
def test_stateless_entries_vs_oracle_and_two_launches(sr, n_units, spectral):
    """unit counts on both sides of the k_obs_blocks limit (42 | 43 units at three blocks per row) and past one row per CU"""
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    r = _renderer(sr)
    kinds_tab = _inputs(sr)[2]
    kinds = _kinds_of(n_units)
    plan = r.plan([UnitRequest(sound=u["sound"], t0=u["t0"], rir=u["rir"], silent=u["rir"] < 0, dis_sound=u.get("dis_sound", -1),
                               dis_rir=u.get("dis_rir", -1)) for u in (kinds_tab[k] for k in kinds)])
    n_mels = 64 if (n_units % 2 or spectral) else 40
    msd, mwd = _mel(sr, n_mels)
    N, T, t4 = n_units, 1 + sr // 160, P.spectrogram_shape(sr)[1]
    bank = r.rirs.spectra if spectral else r.rirs.data
    obs = ops.audio_obs_spec_into if spectral else ops.audio_obs_into
    fused = ops.audio_obs_logmel_rows_spec_into if spectral else ops.audio_obs_logmel_rows_into
    ag0, sg0 = _new(N, 2, sr), _new(N, 65, t4, 2)
    obs(r._spec, bank, r.rirs.lengths, plan.desc, ag0, sg0, sr, sr, "reflect", flags=plan.flags)
    lm0 = ops.logmel(ag0, msd, mwd, EPS, "reflect")
    ag1, sg1, lm1 = _new(N, 2, sr), _new(N, 65, t4, 2), _new(N, n_mels, T, 2)          # all three outputs: one launch
    fused(r._spec, bank, r.rirs.lengths, plan.desc, ag1, sg1, lm1, msd, mwd, sr, sr, EPS, "reflect", flags=plan.flags)
    lm2 = _new(N, n_mels, T, 2)                                                          # log-mel alone: no buffer at all
    fused(r._spec, bank, r.rirs.lengths, plan.desc, None, None, lm2, msd, mwd, sr, sr, EPS, "reflect", flags=plan.flags)
    sg3, lm3 = _new(N, 65, t4, 2), _new(N, n_mels, T, 2)                                 # log-mel + pooled spectrogram
    fused(r._spec, bank, r.rirs.lengths, plan.desc, None, sg3, lm3, msd, mwd, sr, sr, EPS, "reflect", flags=plan.flags)
    torch.cuda.synchronize()
    assert torch.equal(ag1, ag0)                                         # (same convolution code, same order: same bits)
    assert not torch.isnan(sg1).any() and O.relerr(sg1.cpu().numpy(), sg0.cpu().numpy()) <= TOL
    assert torch.equal(sg3, sg1) and torch.equal(lm2, lm1) and torch.equal(lm3, lm1)
    ref_max = lm0.abs().amax(dim=(1, 2, 3))                              # per unit
    err = ((lm1 - lm0).abs().amax(dim=(1, 2, 3)) / ref_max).max()
    assert not torch.isnan(lm1).any() and float(err) <= TOL, float(err)
    _check_vs_oracle(sr, kinds, lm1, sg1, n_mels)
    _check_vs_oracle(sr, kinds, lm3, sg3, n_mels)


def test_stateless_entry_short_step_and_constant_padding():
    """n_valid < out_len (k_obs_rows: the frames behind it are log(eps)) with librosa >= 0.10's padding, 40 bands"""
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    sr, n_valid, N = 44100, 27000, 7
    r = _renderer(sr)
    kinds_tab = _inputs(sr)[2]
    kinds = [0, 3, 4, 5, 0, 5, 0]
    plan = r.plan([UnitRequest(sound=u["sound"], t0=u["t0"], rir=u["rir"], silent=u["rir"] < 0) for u in (kinds_tab[k] for k in kinds)])
    msd, mwd = _mel(sr, 40)
    T, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    for spectral in (False, True):
        bank = r.rirs.spectra if spectral else r.rirs.data
        fused = ops.audio_obs_logmel_rows_spec_into if spectral else ops.audio_obs_logmel_rows_into
        lm, sg = _new(N, 40, T, 2), _new(N, 65, t4, 2)
        fused(r._spec, bank, r.rirs.lengths, plan.desc, None, sg, lm, msd, mwd, n_valid, sr, EPS, "constant", flags=plan.flags)
        torch.cuda.synchronize()
        lmn, sgn = lm.cpu().numpy(), sg.cpu().numpy()
        assert not np.isnan(lmn).any() and not np.isnan(sgn).any()
        for i, k in enumerate(kinds):
            a = _inputs(sr)[3][k]
            if a is None:
                assert np.allclose(lmn[i], np.log(EPS), rtol=1e-6) and not sgn[i].any()
                continue
            a = a.copy()
            a[:, n_valid:] = 0.0
            ref = O.compute_logmel(a, sr, n_mels=40, eps=EPS, pad_mode="constant")
            assert np.abs(lmn[i] - ref).max() <= TOL * np.abs(ref).max(), (spectral, i)
            assert O.relerr(sgn[i], O.compute_spectrogram(a, pad_mode="constant")) <= TOL, (spectral, i)
        assert np.allclose(lmn[0][:, 4 * P.live_pooled_blocks(n_valid, sr):], np.log(EPS), rtol=1e-6)


def _context(sr, binding, **kw):
    """a fresh context on one of the bank bindings: time | both | only (spectral-only)"""
    from ss_amd.context import AudioContext
    from ss_amd.renderer import RirBank
    srcs, rirs, _, _ = _inputs(sr)
    bank = RirBank.from_arrays(rirs, DEV)
    ctx = AudioContext(sr, **kw)
    for i, c in enumerate(srcs):
        ctx.add_source(str(i), c)
    if binding == "only":
        ctx.set_rir_spectra_only(bank.build_spectra(), bank.lengths, bank.cap)
    else:
        ctx.set_rir_bank(bank.data, bank.lengths)
        if binding == "both":
            ctx.set_rir_spectra(bank.build_spectra())
    return ctx, bank


def _cols(sr, kinds):
    tab = _inputs(sr)[2]
    us = [tab[k] for k in kinds]
    cols = dict(sound=np.array([u["sound"] for u in us]), t0=np.array([u["t0"] for u in us]), rir=np.array([u["rir"] for u in us]))
    if any("dis_rir" in u for u in us):
        cols.update(dis_sound=np.array([u.get("dis_sound", 0) for u in us]), dis_rir=np.array([u.get("dis_rir", -1) for u in us]))
    return cols


@pytest.mark.parametrize("binding", ["time", "both", "only"])
def test_context_route_default_is_the_scratch_and_the_policy_opts_in(binding):
    from ss_amd import ops
    sr = 44100
    kinds = _kinds_of(7)
    cols = _cols(sr, kinds)
    msd, mwd = _mel(sr)
    n, T, t4 = len(kinds), 1 + sr // 160, P.spectrogram_shape(sr)[1]
    # default policy: the scratch route, bit-equal to observe-then-features
    ctx, bank = _context(sr, binding)
    assert ctx.wave_scratch_bytes() == 0
    ag = _new(n, 2, sr)
    ctx.observe(audiogoal_out=ag, **cols)
    lm0 = _new(n, 64, T, 2)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm = _new(n, 64, T, 2)
    ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert torch.equal(lm, lm0) and ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    _check_vs_oracle(sr, kinds, lm, None)
    ctx.close()
    # a fresh context that opts in: one fused launch, no waveform anywhere
    ctx, bank = _context(sr, binding)
    ctx.set_logmel_rows_policy(*ALWAYS)
    lm1, lm2, sg2 = _new(n, 64, T, 2), _new(n, 64, T, 2), _new(n, 65, t4, 2)
    ctx.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, **cols)
    ctx.observe(spectrogram_out=sg2, logmel_out=lm2, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    _check_vs_oracle(sr, kinds, lm1, None)
    _check_vs_oracle(sr, kinds, lm2, sg2)
    assert ctx.wave_scratch_bytes() == 0
    ctx.set_logmel_rows_policy(8, 100)                                   # 7 units: outside the range -> the scratch route
    lm3 = _new(n, 64, T, 2)
    ctx.observe(logmel_out=lm3, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert torch.equal(lm3, lm0) and ctx.wave_scratch_bytes() > 0
    ctx.close()


def test_cross_faded_steps_and_bucketed_banks_keep_the_scratch_route():
    from ss_amd import ops
    from ss_amd.context import AudioContext
    from ss_amd.renderer import BucketedRirBank
    sr = 44100
    srcs, rirs, _, _ = _inputs(sr)
    msd, mwd = _mel(sr)
    T = 1 + sr // 160
    # SS2.0 at 44.1 kHz: 0.25-s steps with a cross-fade from the previous RIR
    ctx, bank = _context(sr, "time", step_time=0.25, wrap=True)
    ctx.set_logmel_rows_policy(*ALWAYS)
    idx = np.array([100, 40000, 90000])
    cur, last = np.array([0, 1, 2]), np.array([1, 2, 0])
    Ls = np.array([sr, 30000, 9001])
    cols = dict(sound=np.ones(3), t0=idx, rir=cur, last_rir=last, wrap=(idx >= Ls[cur]).astype(np.uint8),
                last_wrap=(idx >= Ls[last]).astype(np.uint8))
    ag = _new(3, 2, sr)
    ctx.observe(audiogoal_out=ag, **cols)
    lm0 = _new(3, 64, T, 2)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm = _new(3, 64, T, 2)
    ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert not torch.isnan(lm).any() and torch.equal(lm, lm0) and ctx.wave_scratch_bytes() > 0
    ctx.close()
    # a length-bucketed bank
    bb = BucketedRirBank.from_arrays(rirs, DEV, caps=[30000, sr])
    c2 = AudioContext(sr)
    for i, c in enumerate(srcs):
        c2.add_source(str(i), c)
    c2.set_rir_buckets(bb)
    c2.set_logmel_rows_policy(*ALWAYS)
    io = bb.index_of
    cols = dict(sound=np.zeros(4), t0=np.zeros(4), rir=np.array([io[0], io[2], -1, io[1]]))
    ag = _new(4, 2, sr)
    c2.observe(audiogoal_out=ag, **cols)
    lm0 = _new(4, 64, T, 2)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm = _new(4, 64, T, 2)
    c2.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert not torch.isnan(lm).any() and torch.equal(lm, lm0) and c2.wave_scratch_bytes() > 0
    c2.close()


def test_overlap_lanes_under_the_always_policy():
    """two internal lanes, three consecutive steps of different units: each within the rule of the oracle, no waveform scratch"""
    sr = 44100
    ctx, bank = _context(sr, "both")
    ctx.set_logmel_rows_policy(*ALWAYS)
    ctx.set_overlap(2)
    msd, mwd = _mel(sr)
    T, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    steps = [[0, 1, 2, 3, 4], [5, 2, 0, 1, 4, 3, 2], [1, 1, 5]]
    outs = []
    for kinds in steps:
        lm, sg = _new(len(kinds), 64, T, 2), _new(len(kinds), 65, t4, 2)
        ctx.observe(spectrogram_out=sg, logmel_out=lm, mel_start=msd, mel_w=mwd, **_cols(sr, kinds))
        outs.append((lm, sg))
    ctx.join()
    torch.cuda.synchronize()
    for kinds, (lm, sg) in zip(steps, outs):
        _check_vs_oracle(sr, kinds, lm, sg)
    assert ctx.wave_scratch_bytes() == 0
    ctx.set_overlap(1)
    ctx.close()
