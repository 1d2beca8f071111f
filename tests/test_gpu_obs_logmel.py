"""Log-mel observations without a waveform buffer (ss_ctx_observe_features with audiogoal == NULL, ss_audio_obs_logmel_f32 /
ss_audio_obs_logmel_spec_f32): the one-launch fused kernels against the oracle and against the same context's accepted two-launch
call (an audiogoal buffer), on a both-forms, a time-domain-only and a spectral-only engine; the shapes the fused kernels do not
serve (44.1 kHz rows, cross-faded steps, unit counts outside the policy) through the context's own waveform scratch, bit-equal
to observe-then-features."""
import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 16000
TOL = 1e-4
EPS = 1e-6
ALWAYS = (1, 2 ** 31 - 1)              # set_logmel_policy: fused whenever the shape allows
NEVER = (1, 0)
_ENGINES = {}


def _mel(sr, n_mels=64):
    ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
    return torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)


def _check_mel(got, ref):
    got = np.asarray(got)
    assert got.shape == ref.shape and not np.isnan(got).any()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= TOL, err


def _engine(kind):
    """one engine per bank form for the module: {both, time, only} -> (engine, sources, RIRs in wav layout, bank slots)"""
    if kind not in _ENGINES:
        from ss_amd.renderer import AudioEngine
        rng = np.random.default_rng(5)
        src = O.synth_sources(rng, SR, k=3)
        rirs = [np.ascontiguousarray(O.synth_rir(rng, SR, length=int(rng.uniform(0.2, 1.0) * SR), n=1)[0].T) for _ in range(6)]
        rirs.append(np.zeros((0, 2), np.float32))                            # an empty file: the zero RIR
        eng = AudioEngine(SR, device=DEV, rir_spectral={"both": True, "time": False, "only": "only"}[kind], rir_slots=16)
        for i, s_ in enumerate(src):
            eng.source_id(f"s{i}", s_)
        slots = [eng.rir_slot(i, (lambda h=h: h)) for i, h in enumerate(rirs)]
        _ENGINES[kind] = (eng, src, rirs, slots)
    return _ENGINES[kind]


@pytest.mark.parametrize("overlap", [1, 2])
@pytest.mark.parametrize("dis", [False, True], ids=["plain", "distractor"])
@pytest.mark.parametrize("n_units", [1, 37, 300])
@pytest.mark.parametrize("kind", ["both", "time", "only"])
def test_fused_logmel_vs_oracle_and_two_launch_route(kind, n_units, dis, overlap):
    eng, src, rirs, slots = _engine(kind)
    rng = np.random.default_rng(1000 * n_units + 10 * dis + overlap)
    n = n_units
    sound, h = rng.integers(0, 3, n), rng.integers(0, len(rirs), n)
    rir = np.asarray([slots[i] for i in h], np.int64)
    silent = (np.arange(n) % 11 == 3)
    rir[silent] = -1
    cols = dict(sound=sound, t0=np.zeros(n, np.int64), rir=rir)
    dh = rng.integers(0, 6, n)
    if dis:
        cols.update(dis_sound=(sound + 1) % 3, dis_rir=np.where(np.arange(n) % 3 == 0, np.asarray([slots[i] for i in dh]), -1))
    ctx = eng._sync_context_bank(n, dis)
    ctx.set_overlap(1)
    msd, mwd = _mel(SR)
    T, t4 = 1 + SR // 160, P.spectrogram_shape(SR)[1]
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    sg_before = new(n, 65, t4, 2)
    ctx.observe(spectrogram_out=sg_before, **cols)
    ag_ref, sg_ref, lm_ref = new(n, 2, SR), new(n, 65, t4, 2), new(n, 64, T, 2)
    ctx.observe(spectrogram_out=sg_ref, audiogoal_out=ag_ref, logmel_out=lm_ref, mel_start=msd, mel_w=mwd, **cols)   # accepted today
    torch.cuda.synchronize()
    ctx.set_overlap(overlap)
    ctx.set_logmel_policy(*ALWAYS)
    lm1, lm2, sg2, lm3 = new(n, 64, T, 2), new(n, 64, T, 2), new(n, 65, t4, 2), new(n, 64, T, 2)
    ctx.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, **cols)                          # log-mel alone: no buffer at all
    ctx.observe(spectrogram_out=sg2, logmel_out=lm2, mel_start=msd, mel_w=mwd, **cols)     # log-mel + pooled spectrogram
    ctx.set_logmel_policy(*NEVER)                                                          # the scratch route on the same shape
    ctx.observe(logmel_out=lm3, mel_start=msd, mel_w=mwd, **cols)
    ctx.join()
    torch.cuda.synchronize()
    ctx.set_overlap(1)
    ctx.set_logmel_policy(*ALWAYS)
    from ss_amd import ops
    lm_two = new(n, 64, T, 2)                                         # scratch route = observe, then the feature kernel
    ops.audio_features_into(ag_ref, logmel_out=lm_two, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    torch.cuda.synchronize()
    assert torch.equal(lm3, lm_two)
    ref_max = float(lm_ref.abs().max())
    for lm in (lm1, lm2):
        assert not torch.isnan(lm).any()
        assert float((lm - lm_ref).abs().max()) <= TOL * ref_max
    assert not torch.isnan(sg2).any() and O.relerr(sg2.cpu().numpy(), sg_ref.cpu().numpy()) <= TOL
    lm1n, lm2n, sg2n = lm1.cpu().numpy(), lm2.cpu().numpy(), sg2.cpu().numpy()
    checked = 0
    for i in list(range(min(n, 8))) + [n - 1]:
        if silent[i] or not rirs[h[i]].size:                           # silent / zero RIR: log(eps) everywhere, pooled zeros
            if not (dis and cols["dis_rir"][i] >= 0):
                assert np.allclose(lm1n[i], np.log(EPS), rtol=1e-6) and np.allclose(lm2n[i], np.log(EPS), rtol=1e-6)
                assert not sg2n[i].any()
            continue
        d_on = dis and cols["dis_rir"][i] >= 0
        a = O.compute_audiogoal(src[sound[i]], rirs[h[i]], SR, distractor=src[(sound[i] + 1) % 3] if d_on else None,
                                distractor_rir=rirs[dh[i]] if d_on else None).astype(np.float32)
        ref = O.compute_logmel(a, SR, n_mels=64, eps=EPS)
        _check_mel(lm1n[i], ref)
        _check_mel(lm2n[i], ref)
        assert O.relerr(sg2n[i], O.compute_spectrogram(a)) <= TOL
        checked += 1
    assert checked or n == 1
    sg_after = new(n, 65, t4, 2)                                       # a plain step afterwards is what it was before
    ctx.observe(spectrogram_out=sg_after, **cols)
    torch.cuda.synchronize()
    assert torch.equal(sg_after, sg_before)


def test_gccphat_without_a_waveform_buffer_still_raises():
    eng, _, _, slots = _engine("both")
    n = 4
    cols = dict(sound=np.zeros(n, np.int64), t0=np.zeros(n, np.int64), rir=np.full(n, slots[0], np.int64))
    ctx = eng._sync_context_bank(n, False)
    ctx.set_overlap(1)
    msd, mwd = _mel(SR)
    T = 1 + SR // 160
    lm, gc, sg = torch.zeros((n, 64, T, 2), device=DEV), torch.zeros((n, 65, T), device=DEV), torch.zeros((n, 65, 26, 2), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(Exception):
        ctx.observe_prepared_features(ctx.prepare(**cols), sg.data_ptr(), None, stream, ctx.features(lm, msd, mwd, EPS, gc, 32, 1e-8))
    with pytest.raises(Exception):
        ctx.observe_prepared_features(ctx.prepare(**cols), None, None, stream, ctx.features(None, None, None, EPS, gc, 32, 1e-8))
    f = ctx.features(lm, msd, mwd, EPS)                                 # log-mel alone through the prepared entry: accepted
    ctx.observe_prepared_features(ctx.prepare(**cols), None, None, stream, f)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lm).all()) and float(lm.max()) > np.log(EPS) + 1.0


def test_scratch_route_at_44k_and_cross_faded_steps_bit_equal_to_observe_then_features():
    from ss_amd import ops
    from ss_amd.context import AudioContext
    from ss_amd.renderer import RirBank
    rng = np.random.default_rng(9)
    # 44.1 kHz: rows of three partition blocks
    sr = 44100
    s44 = O.synth_sources(rng, sr, k=1)[0]
    r44 = [np.ascontiguousarray(O.synth_rir(rng, sr, n=1)[0].T)]
    b44 = RirBank.from_arrays(r44, DEV)
    c3 = AudioContext(sr)
    c3.add_source("s", s44)
    c3.set_rir_bank(b44.data, b44.lengths)
    msd, mwd = _mel(sr)
    n, T, t4 = 3, 1 + sr // 160, P.spectrogram_shape(sr)[1]
    cols = dict(sound=np.zeros(n), t0=np.zeros(n), rir=np.array([0, -1, 0]))
    ag, sg0 = torch.empty((n, 2, sr), device=DEV), torch.empty((n, 65, t4, 2), device=DEV)
    c3.observe(spectrogram_out=sg0, audiogoal_out=ag, **cols)
    lm0 = torch.empty((n, 64, T, 2), device=DEV)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    ag1, lm1 = torch.empty_like(ag), torch.empty_like(lm0)               # (without a spectrogram the waveform comes from the
    c3.observe(audiogoal_out=ag1, **cols)                               #  convolution kernel alone)
    ops.audio_features_into(ag1, logmel_out=lm1, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    for want_sg in (True, False):
        lm, sg = torch.full_like(lm0, float("nan")), torch.full_like(sg0, float("nan"))
        c3.observe(spectrogram_out=sg if want_sg else None, logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
        torch.cuda.synchronize()
        assert torch.equal(lm, lm0 if want_sg else lm1) and (not want_sg or torch.equal(sg, sg0))
    lm44, cols44, mel44 = lm1, cols, (msd, mwd)
    _check_mel(lm0[0].cpu().numpy(), O.compute_logmel(O.compute_audiogoal(s44, r44[0], sr).astype(np.float32), sr, n_mels=64, eps=EPS))
    # SS2.0: 0.25-s steps at 16 kHz with a cross-fade from the previous RIR
    src3 = O.tile_short_source(O.synth_sources(rng, SR, k=1)[0], SR)
    rl = [np.ascontiguousarray(O.synth_rir(rng, SR, length=L, n=1)[0].T) for L in (9000, 12000, 20000)]
    bank2 = RirBank.from_arrays(rl, DEV)
    c2 = AudioContext(SR, step_time=0.25, wrap=True)
    c2.add_source("s", src3)
    c2.set_rir_bank(bank2.data, bank2.lengths)
    idx = np.array([100, 15000, 30000, 46000, 47000])
    cur, last = np.array([0, 1, 2, 0, 1]), np.array([1, 2, 0, -1, 2])
    Ls = np.array([9000, 12000, 20000])
    cols = dict(sound=np.zeros(5), t0=idx, rir=cur, last_rir=last, wrap=(idx >= Ls[cur]).astype(np.uint8),
                last_wrap=(idx >= Ls[np.maximum(last, 0)]).astype(np.uint8))
    msd, mwd = _mel(SR)
    T = 1 + SR // 160
    ag, sg0 = torch.empty((5, 2, SR), device=DEV), torch.empty((5, 65, 26, 2), device=DEV)
    c2.observe(spectrogram_out=sg0, audiogoal_out=ag, **cols)
    lm0 = torch.empty((5, 64, T, 2), device=DEV)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm, sg = torch.full_like(lm0, float("nan")), torch.full_like(sg0, float("nan"))
    c2.set_logmel_policy(*ALWAYS)                                       # (the step's cross-fade alone sends it to the scratch)
    c2.observe(spectrogram_out=sg, logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert torch.equal(lm, lm0) and torch.equal(sg, sg0)
    for i in range(5):
        ref = O.compute_audiogoal_continuous(src3, rl[cur[i]], SR, int(idx[i]), 0.25,
                                             last_rir=rl[last[i]] if last[i] >= 0 else None, use_crossfade=True).astype(np.float32)
        _check_mel(lm[i].cpu().numpy(), O.compute_logmel(ref, SR, n_mels=64, eps=EPS))
    # ... and the same context without a cross-fade in the step (no previous RIR anywhere): the fused launch, short step
    cols2 = dict(sound=np.zeros(5), t0=idx, rir=cur, wrap=cols["wrap"])
    c2.observe(spectrogram_out=sg0, audiogoal_out=ag, **cols2)
    lm1 = torch.full_like(lm0, float("nan"))
    c2.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, **cols2)
    torch.cuda.synchronize()
    for i in range(5):
        _check_mel(lm1[i].cpu().numpy(), O.compute_logmel(ag[i].cpu().numpy(), SR, n_mels=64, eps=EPS))
    # ss_release_scratch frees the contexts' waveform scratches as well; they grow again on demand
    from ss_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().ss_release_scratch() == 0
    lm = torch.full_like(lm44, float("nan"))
    c3.observe(logmel_out=lm, mel_start=mel44[0], mel_w=mel44[1], **cols44)
    torch.cuda.synchronize()
    assert torch.equal(lm, lm44)


@pytest.mark.parametrize("n_mels,pad_mode,n_valid", [(64, "reflect", SR), (40, "constant", SR), (64, "reflect", 4000)])
def test_stateless_entries_vs_two_launches(n_mels, pad_mode, n_valid):
    """ss_audio_obs_logmel_f32 / _spec_f32 against ops.audio_obs_* (waveform + spectrogram) + ops.logmel of that waveform; the
    waveform they write themselves when asked is the one ss_audio_obs_f32 writes"""
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    rng = np.random.default_rng(n_mels + n_valid)
    r = BatchedAudioRenderer(SR, device=DEV, pad_mode=pad_mode)
    for i, c in enumerate(O.synth_sources(rng, SR, k=4)):
        r.add_source(str(i), c)
    rirs = [np.ascontiguousarray(O.synth_rir(rng, SR, length=L, n=1)[0].T) for L in (16000, 9000, 12000, 16000, 5000)]
    r.set_rir_bank(RirBank.from_arrays(rirs, DEV))
    r.rirs.build_spectra()
    N = 21
    plan = r.plan_arrays(rng.integers(0, 4, N), np.zeros(N, np.int64), rng.integers(0, len(rirs), N))
    ms, mw, _ = P.mel_filterbank_sparse(SR, n_mels)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    T, t4 = 1 + SR // 160, P.spectrogram_shape(SR)[1]
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    for spectral in (False, True):
        ag0, sg0 = new(N, 2, SR), new(N, 65, t4, 2)
        if spectral:
            ops.audio_obs_spec_into(r._spec, r.rirs.spectra, r.rirs.lengths, plan.desc, ag0, sg0, n_valid, SR, pad_mode, flags=plan.flags)
        else:
            ops.audio_obs_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag0, sg0, n_valid, SR, pad_mode, flags=plan.flags)
        lm0 = ops.logmel(ag0, msd, mwd, EPS, pad_mode)
        for flags in (plan.flags, 0):                                   # loop-free kernel, and the loop form on the same units
            ag1, sg1, lm1, lm2 = new(N, 2, SR), new(N, 65, t4, 2), new(N, n_mels, T, 2), new(N, n_mels, T, 2)
            if spectral:
                ops.audio_obs_logmel_spec_into(r._spec, r.rirs.spectra, r.rirs.lengths, plan.desc, ag1, sg1, lm1, msd, mwd, n_valid,
                                               SR, EPS, pad_mode, flags=flags)
                ops.audio_obs_logmel_spec_into(r._spec, r.rirs.spectra, r.rirs.lengths, plan.desc, None, None, lm2, msd, mwd, n_valid,
                                               SR, EPS, pad_mode, flags=flags)
            else:
                ops.audio_obs_logmel_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag1, sg1, lm1, msd, mwd, n_valid, SR, EPS,
                                          pad_mode, flags=flags)
                ops.audio_obs_logmel_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, None, None, lm2, msd, mwd, n_valid, SR, EPS,
                                          pad_mode, flags=flags)
            torch.cuda.synchronize()
            if flags == plan.flags:
                assert torch.equal(ag1, ag0)                            # (same convolution code, same order: same bits)
            else:
                assert O.relerr(ag1.cpu().numpy(), ag0.cpu().numpy()) <= TOL
            assert O.relerr(sg1.cpu().numpy(), sg0.cpu().numpy()) <= TOL
            for lm in (lm1, lm2):
                assert not torch.isnan(lm).any()
                assert float((lm - lm0).abs().max()) <= TOL * float(lm0.abs().max())
    from ss_amd import _lib
    with pytest.raises(_lib.SsHipError):                                # two partition blocks: refused by this level
        ops.audio_obs_logmel_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, None, None, new(N, n_mels, 1 + 44100 // 160, 2),
                                  msd, mwd, 16000, 44100, EPS, pad_mode, flags=plan.flags)
