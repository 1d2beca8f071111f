"""Log-mel observations of SoundSpaces 2.0 steps (0.25 s of a 1-s row, cross-faded from the previous step's RIR) in one launch,
without a waveform buffer: ss_audio_obs_logmel_ss2_f32 (the cross-faded one-block row at 16 kHz; block 0 of a 44.1 kHz row with
and without the cross-fade) against today's two launches, and the context route behind ss_ctx_set_logmel_ss2_policy (default:
never - the scratch route, bit-equal to observe-then-features) against the oracle.  Tolerances: the project's log-mel rule
(1e-4 of the largest value per unit), relerr <= 1e-4 for the pooled spectrogram; the waveform is bit-equal to
ss_audio_obs_f32's.  Every output is pre-filled with NaN."""
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
LENS = (9000, 12000, 20000)            # RIR taps; the last spans two partition blocks.  Bank entry 3 is an empty RIR
_CACHE = {}


def _mel(sr, n_mels=64):
    ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
    return torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)


def _new(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _inputs(sr):
    """rng 31: a 1-s clip tiled x3 (as the reference loads it) and a second 1-s clip; RIRs of LENS taps (wav layout) + an empty one"""
    if sr not in _CACHE:
        rng = np.random.default_rng(31)
        a, b = O.synth_sources(rng, sr, k=2, seconds=1)
        rirs = [np.ascontiguousarray(O.synth_rir(rng, sr, length=L, n=1)[0].T) for L in LENS]
        rirs.append(np.zeros((0, 2), np.float32))
        _CACHE[sr] = ([O.tile_short_source(a, sr), b], rirs)
    return _CACHE[sr]


def _indices(sr):
    """sample indices in the early branch, around the RIR lengths and in the steady branch up to the wrap-around of the clip end"""
    return [100, 15000, 30000, 3 * sr - sr // 8, 3 * sr - sr // 16]


def _kind(sr, k, crossfade):
    """unit kinds of a step: four audible ones (three with a previous RIR when cross-faded), a silent unit, an empty RIR"""
    idx = _indices(sr)
    tab = [dict(index=idx[0], rir=0, last_rir=1), dict(index=idx[1], rir=1, last_rir=2), dict(index=idx[2], rir=2, last_rir=0),
           dict(index=idx[3], rir=0, last_rir=-1), dict(index=0, rir=-1, last_rir=-1), dict(index=idx[4], rir=3, last_rir=-1)]
    u = dict(tab[k % 6])
    if not crossfade:
        u["last_rir"] = -1
    return u


def _wrap(index, rir):
    return rir < 3 and index - LENS[rir] >= 0            # the reference's steady branch (continuous_simulator.py:433)


def _requests(sr, kinds, crossfade):
    from ss_amd.renderer import UnitRequest
    out = []
    for k in kinds:
        u = _kind(sr, k, crossfade)
        if u["rir"] < 0:
            out.append(UnitRequest(silent=True))
            continue
        out.append(UnitRequest(sound=0, t0=u["index"], rir=u["rir"], wrap=_wrap(u["index"], u["rir"]), last_rir=u["last_rir"],
                               last_wrap=_wrap(u["index"], u["last_rir"]) if u["last_rir"] >= 0 else None))
    return out


def _oracle_wave(sr, k, crossfade):
    key = ("wave", sr, k % 6, crossfade)
    if key not in _CACHE:
        srcs, rirs = _inputs(sr)
        u = _kind(sr, k, crossfade)
        a = None
        if u["rir"] >= 0 and rirs[u["rir"]].size:
            a = O.compute_audiogoal_continuous(srcs[0], rirs[u["rir"]], sr, u["index"], 0.25,
                                               last_rir=rirs[u["last_rir"]] if u["last_rir"] >= 0 else None,
                                               use_crossfade=crossfade).astype(np.float32)
        _CACHE[key] = a
    return _CACHE[key]


def _check_vs_oracle(sr, kinds, crossfade, lm, sg):
    """every unit of the step against the oracle of its kind (computed once per kind)"""
    lm = lm.cpu().numpy()
    sg = None if sg is None else sg.cpu().numpy()
    assert not np.isnan(lm).any() and (sg is None or not np.isnan(sg).any())
    live = P.live_pooled_blocks(sr // 4, sr)
    for i, k in enumerate(kinds):
        a = _oracle_wave(sr, k, crossfade)
        if a is None:                                    # silent / empty RIR: log(eps) everywhere, exact-zero spectrogram
            assert np.allclose(lm[i], np.log(EPS), rtol=1e-6), i
            assert sg is None or not sg[i].any(), i
            continue
        mkey, skey = ("mel", sr, k % 6, crossfade), ("sg", sr, k % 6, crossfade)
        if mkey not in _CACHE:
            _CACHE[mkey] = O.compute_logmel(a, sr, n_mels=64, eps=EPS)
            _CACHE[skey] = O.compute_spectrogram(a)
        ref = _CACHE[mkey]
        err = np.abs(lm[i] - ref).max() / np.abs(ref).max()
        assert err <= TOL, (i, k, err)
        assert np.allclose(lm[i][:, 4 * live:], np.log(EPS), rtol=1e-6), i
        if sg is not None:
            assert O.relerr(sg[i], _CACHE[skey]) <= TOL, (i, k)
            assert not sg[i][:, live:].any(), i


def _renderer(sr):
    key = ("renderer", sr)
    if key not in _CACHE:
        from ss_amd.renderer import BatchedAudioRenderer, RirBank
        srcs, rirs = _inputs(sr)
        r = BatchedAudioRenderer(sr, device=DEV, step_time=0.25, wrap=True)
        for i, c in enumerate(srcs):
            r.add_source(str(i), c)
        r.set_rir_bank(RirBank.from_arrays(rirs, DEV))
        _CACHE[key] = r
    return _CACHE[key]


@pytest.mark.parametrize("n_units", [1, 5, 150])
@pytest.mark.parametrize("sr,crossfade", [(16000, True), (44100, True), (44100, False)], ids=["16k-xfade", "44k-xfade", "44k-plain"])
def test_stateless_entry_vs_two_launches(sr, crossfade, n_units):
    """ss_audio_obs_logmel_ss2_f32 against ops.audio_obs_into (waveform + spectrogram) + ops.logmel of that waveform; 150 units =
    300 workgroups, more than one round of CUs"""
    from ss_amd import ops
    r = _renderer(sr)
    kinds = [(i + n_units) % 6 if n_units > 1 else 0 for i in range(n_units)]
    plan = r.plan(_requests(sr, kinds, crossfade))
    assert bool(plan.flags & ops.FLAG_CROSSFADE) == crossfade
    msd, mwd = _mel(sr)
    N, T, t4, nv = n_units, 1 + sr // 160, P.spectrogram_shape(sr)[1], r.n_valid
    assert nv == sr // 4
    ag0, sg0 = _new(N, 2, sr), _new(N, 65, t4, 2)
    ops.audio_obs_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag0, sg0, nv, sr, "reflect", flags=plan.flags)
    lm0 = ops.logmel(ag0, msd, mwd, EPS, "reflect")
    fused = lambda ag, sg, lm: ops.audio_obs_logmel_ss2_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag, sg, lm, msd, mwd,
                                                             nv, sr, EPS, "reflect", flags=plan.flags)
    ag1, sg1, lm1 = _new(N, 2, sr), _new(N, 65, t4, 2), _new(N, 64, T, 2)                # all three outputs: one launch
    fused(ag1, sg1, lm1)
    lm2 = _new(N, 64, T, 2)                                                              # log-mel alone: no buffer at all
    fused(None, None, lm2)
    sg3, lm3 = _new(N, 65, t4, 2), _new(N, 64, T, 2)                                     # log-mel + pooled spectrogram
    fused(None, sg3, lm3)
    torch.cuda.synchronize()
    assert torch.equal(ag1, ag0)                                         # (same convolution code, same order: same bits)
    assert not torch.isnan(sg1).any() and O.relerr(sg1.cpu().numpy(), sg0.cpu().numpy()) <= TOL
    assert torch.equal(sg3, sg1) and torch.equal(lm2, lm1) and torch.equal(lm3, lm1)
    err = ((lm1 - lm0).abs().amax(dim=(1, 2, 3)) / lm0.abs().amax(dim=(1, 2, 3))).max()  # per unit
    print(f"sr {sr} crossfade {crossfade} n {N}: worst log-mel error vs two launches {float(err):.3g}")
    assert not torch.isnan(lm1).any() and float(err) <= TOL, float(err)
    live = P.live_pooled_blocks(nv, sr)
    quiet = torch.full_like(lm1[:, :, 4 * live:], float(np.log(EPS)))
    assert torch.allclose(lm1[:, :, 4 * live:], quiet, rtol=1e-6, atol=0) and not sg1[:, :, live:].any()
    for i, k in enumerate(kinds):                                        # silent units and empty RIRs
        if k % 6 >= 4:
            assert torch.allclose(lm1[i], torch.full_like(lm1[i], float(np.log(EPS))), rtol=1e-6, atol=0) and not sg1[i].any()
    if n_units == 5:
        _check_vs_oracle(sr, kinds, crossfade, lm1, sg1)
    from ss_amd import _lib
    if crossfade and sr == 16000:
        with pytest.raises(_lib.SsHipError):                             # the plain one-block row belongs to the other entry
            ops.audio_obs_logmel_ss2_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, None, None, lm2, msd, mwd, nv, sr, EPS,
                                          "reflect", flags=0)


def _context(sr, binding="time", **kw):
    from ss_amd.context import AudioContext
    from ss_amd.renderer import BucketedRirBank, RirBank
    srcs, rirs = _inputs(sr)
    ctx = AudioContext(sr, step_time=0.25, wrap=True, **kw)
    for i, c in enumerate(srcs):
        ctx.add_source(str(i), c)
    if binding == "buckets":
        bank = BucketedRirBank.from_arrays(rirs, DEV, caps=[12000, 20000])
        ctx.set_rir_buckets(bank)
        return ctx, bank
    bank = RirBank.from_arrays(rirs, DEV)
    if binding == "only":
        ctx.set_rir_spectra_only(bank.build_spectra(), bank.lengths, bank.cap)
    else:
        ctx.set_rir_bank(bank.data, bank.lengths)
    return ctx, bank


def _cols(sr, kinds, crossfade, index_of=None):
    us = [_kind(sr, k, crossfade) for k in kinds]
    io = (lambda i: i) if index_of is None else (lambda i: index_of[i] if i >= 0 else -1)
    idx = np.array([u["index"] for u in us])
    cur, last = np.array([u["rir"] for u in us]), np.array([u["last_rir"] for u in us])
    cols = dict(sound=np.zeros(len(us)), t0=idx, rir=np.array([io(i) for i in cur]),
                wrap=np.array([_wrap(i, c) if c >= 0 else 0 for i, c in zip(idx, cur)], np.uint8))
    if crossfade:
        cols.update(last_rir=np.array([io(i) for i in last]),
                    last_wrap=np.array([_wrap(i, l) if l >= 0 else 0 for i, l in zip(idx, last)], np.uint8))
    return cols


def _observe_then_features(ctx, sr, cols, n, want_sg):
    from ss_amd import ops
    msd, mwd = _mel(sr)
    ag, sg = _new(n, 2, sr), (_new(n, 65, P.spectrogram_shape(sr)[1], 2) if want_sg else None)
    ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
    lm = _new(n, 64, 1 + sr // 160, 2)
    ops.audio_features_into(ag, logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    torch.cuda.synchronize()
    return lm, sg


def _context_route(sr, kinds, crossfade, overlap):
    msd, mwd = _mel(sr)
    n, T, t4 = len(kinds), 1 + sr // 160, P.spectrogram_shape(sr)[1]
    cols = _cols(sr, kinds, crossfade)
    # default policy: the scratch route, bit-equal to observe-then-features
    ctx, _ = _context(sr)
    sg_before = _new(n, 65, t4, 2)
    ctx.observe(spectrogram_out=sg_before, **cols)
    lm0, sg0 = _observe_then_features(ctx, sr, cols, n, True)
    lm0b, _ = _observe_then_features(ctx, sr, cols, n, False)
    assert ctx.wave_scratch_bytes() == 0
    ctx.set_overlap(overlap)
    lm_a, lm_b, sg_b = _new(n, 64, T, 2), _new(n, 64, T, 2), _new(n, 65, t4, 2)
    ctx.observe(logmel_out=lm_a, mel_start=msd, mel_w=mwd, **cols)
    ctx.observe(spectrogram_out=sg_b, logmel_out=lm_b, mel_start=msd, mel_w=mwd, **cols)
    ctx.join()
    torch.cuda.synchronize()
    ctx.set_overlap(1)
    assert torch.equal(lm_a, lm0b) and torch.equal(lm_b, lm0) and torch.equal(sg_b, sg0)
    assert ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    _check_vs_oracle(sr, kinds, crossfade, lm0, sg0)
    sg_after = _new(n, 65, t4, 2)
    ctx.observe(spectrogram_out=sg_after, **cols)
    torch.cuda.synchronize()
    assert torch.equal(sg_after, sg_before)
    ctx.close()
    # a fresh context that opts in: one fused launch per step, no waveform anywhere
    ctx, _ = _context(sr)
    ctx.set_logmel_ss2_policy(*ALWAYS)
    sg_pre = _new(n, 65, t4, 2)
    ctx.observe(spectrogram_out=sg_pre, **cols)
    ctx.set_overlap(overlap)
    lm1, lm2, sg2 = _new(n, 64, T, 2), _new(n, 64, T, 2), _new(n, 65, t4, 2)
    ctx.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, **cols)
    ctx.observe(spectrogram_out=sg2, logmel_out=lm2, mel_start=msd, mel_w=mwd, **cols)
    ctx.join()
    torch.cuda.synchronize()
    ctx.set_overlap(1)
    assert ctx.wave_scratch_bytes() == 0                                 # the fused launch really ran
    _check_vs_oracle(sr, kinds, crossfade, lm1, None)
    _check_vs_oracle(sr, kinds, crossfade, lm2, sg2)
    for lm in (lm1, lm2):                                                # ... and within the rule of the scratch route's result
        err = ((lm - lm0).abs().amax(dim=(1, 2, 3)) / lm0.abs().amax(dim=(1, 2, 3))).max()
        assert float(err) <= TOL, float(err)
    assert O.relerr(sg2.cpu().numpy(), sg0.cpu().numpy()) <= TOL
    sg_post = _new(n, 65, t4, 2)
    ctx.observe(spectrogram_out=sg_post, **cols)
    torch.cuda.synchronize()
    assert torch.equal(sg_post, sg_pre) and torch.equal(sg_pre, sg_before)
    ctx.set_logmel_ss2_policy(n + 1, 1000)                               # outside the range: the scratch route again
    lm3 = _new(n, 64, T, 2)
    ctx.observe(logmel_out=lm3, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert torch.equal(lm3, lm0b) and ctx.wave_scratch_bytes() > 0
    ctx.close()


@pytest.mark.parametrize("overlap", [1, 2])
def test_context_route_on_a_cross_faded_16k_step(overlap):
    """five units: RIRs of 9000 / 12000 / 20000 taps, early and (wrapped) steady branches, one unit without a previous RIR"""
    _context_route(16000, [0, 1, 2, 3, 0], True, overlap)


@pytest.mark.parametrize("crossfade", [True, False], ids=["crossfade", "first-step"])
def test_context_route_on_a_44k_step(crossfade):
    """three units of an SS2.0 step at 44.1 kHz, one of them silent; without a previous RIR anywhere (the first step of an
    episode) the step carries no cross-fade flag and takes the same entry"""
    _context_route(44100, [0, 4, 2], crossfade, 1)


def test_bucketed_and_spectral_only_contexts_keep_todays_route():
    """out of scope for the fused entry: with the policy set to always such a context still takes the scratch route (bit-equal to
    observe-then-features) - or refuses the step, where it refuses it today (a cross-faded step on a spectral-only bank)"""
    from ss_amd import _lib
    for sr, binding, crossfade in ((16000, "buckets", True), (44100, "buckets", False), (44100, "only", False), (16000, "only", True)):
        ctx, bank = _context(sr, binding)
        ctx.set_logmel_ss2_policy(*ALWAYS)
        kinds = [0, 1, 2, 4]
        cols = _cols(sr, kinds, crossfade, index_of=bank.index_of if binding == "buckets" else None)
        msd, mwd = _mel(sr)
        lm = _new(len(kinds), 64, 1 + sr // 160, 2)
        if binding == "only" and crossfade:                              # it would read rows: SS_EINVAL, with or without a buffer
            with pytest.raises(_lib.SsHipError):
                ctx.observe(audiogoal_out=_new(len(kinds), 2, sr), **cols)
            with pytest.raises(_lib.SsHipError):
                ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
            ctx.close()
            continue
        lm0, _ = _observe_then_features(ctx, sr, cols, len(kinds), False)
        ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
        torch.cuda.synchronize()
        assert not torch.isnan(lm).any() and torch.equal(lm, lm0) and ctx.wave_scratch_bytes() > 0, (sr, binding)
        ctx.close()
