"""The half-precision spectral RIR bank under the fused row kernels of 2 or 3 partition blocks on the GPU (44.1 / 48 kHz;
include/ss_hip.h "The half bank for rows of 2 or 3 partition blocks"): ss_audio_obs_rows_spec16_f32 /
ss_audio_obs_logmel_rows_spec16_f32 (k_obs_blocks / k_obs_rows <.., HALF>), ss_ctx_set_rir_spectra16_rows,
AudioEngine(rir_spectral="half", rir_half_rows=True).

  * stateless entries against ss_audio_obs_spec_f32 / ss_audio_obs_logmel_rows_spec_f32 fed float(q) * hscale, <= 2e-6 of peak
    (each fp32 path is held to <= 1e-6 of peak against float64 by the project's parity record, the inputs are identical; the host
    build measures 0.0); the waveform of the log-mel launch bit-equal to the spectrogram launch's;
  * producer: RirStore(spectral="half") at capacity 44 100 against the numpy quantisation of the fp32 store's spectra;
  * the engine end to end against the overlap-save model with the same quantiser (tests/spec_half_rows_ref.py), <= 1e-4 of peak
    (the project's budget) on waveform, pooled spectrogram and log-mel.  The model is fed the halves and scales the bank under
    test holds (the quantiser's decisions on the kernel's own fp32 spectra; the producer case ties them to the numpy rule value
    for value), after checking that they are the RIR's spectrum to within half an fp16 step.  The distance to the UNQUANTISED
    oracle is printed, not asserted: it is the format's loss.
Every output is pre-filled with NaN.  Nothing here captures a graph (a k_obs_blocks launch must not be replayed from one)."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_half_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 1e-4
AB = 2e-6
EPS = 1e-6
_CACHE = {}


def _new(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _mel(sr, n_mels=64):
    ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
    return torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)


def _world(sr):
    """per rate, computed once: a 1-s and a 3-s source; a planar bank of capacity 49 152 - entry 0 of 49 152 taps, 1 empty, 2 of
    9 000 taps, 3 of 40 000 taps scaled by 32 768 (every block audible) - a renderer over it, its half form and the
    dequantisation of that"""
    if sr not in _CACHE:
        from ss_amd import ops
        from ss_amd.renderer import BatchedAudioRenderer, RirBank
        rng = np.random.default_rng(sr)
        srcs = [O.synth_sources(rng, sr, k=1, seconds=1)[0], O.synth_sources(rng, sr, k=1, seconds=3)[0]]
        lens = np.asarray([49152, 0, 9000, 40000], np.int32)
        rows = np.zeros((4, 2, 49152), np.float32)
        for i, n in enumerate(lens):
            if n:
                rows[i, :, :n] = O.synth_rir_blocks(rng, sr, int(n), n=1)[0]
        rows[3] *= np.float32(32768.0)
        r = BatchedAudioRenderer(sr, device=DEV)
        for i, s in enumerate(srcs):
            r.add_source(f"s{i}", s)
        bank = torch.from_numpy(rows).to(DEV)
        r.set_rir_bank(RirBank(bank, torch.from_numpy(lens).to(DEV)))
        h16, hs = ops.rir_spectra16(bank)
        deq = (h16.float() * hs[..., None]).contiguous()                 # float(q) * hscale, exact in fp32
        _CACHE[sr] = types.SimpleNamespace(srcs=srcs, rows=rows, lens=lens, r=r, h16=h16, hs=hs, deq=deq)
    return _CACHE[sr]


def _perm():
    """natural component n of a block spectrum = stored component perm[n] (spec_half_rows_ref.kernel_order over ss_rir_spectra_f32)"""
    if "perm" not in _CACHE:
        from ss_amd import ops
        _CACHE["perm"] = R.kernel_order(lambda rows: ops.rir_spectra(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)).cpu().numpy())
    return _CACHE["perm"]


def _entry_spectra(q, scale, rir):
    """float(q) * scale of one bank entry (halves [2, hb, F], scales [2, hb]) in natural order - after checking that it IS the
    spectrum of `rir` [2, L]: every component within half an fp16 step of the scaled block maximum (8 / 2^14 of it) of the
    float64 transform"""
    got = R.bank_spectra(q, scale, _perm())
    for c in range(2):
        want = R.natural_components(rir[c])
        assert got.shape[1] >= want.shape[0] and not got[c, want.shape[0]:].any()
        for i in range(want.shape[0]):
            assert np.abs(got[c, i] - want[i]).max() <= 5e-4 * np.abs(want[i]).max(), (c, i)
    return got


def _bank_model(bank, clip, rir, t0, sr, slot=None):
    """the model of one row from the bank's own entry for `rir` [2, L] (wav layout accepted): `slot`, or the resident entry of that
    length whose spectra are the RIR's"""
    rir = np.asarray(rir, np.float32)
    rir = np.ascontiguousarray(rir.T) if rir.shape[0] != 2 else rir
    lens = bank.lengths.cpu().numpy()
    slots = [slot] if slot is not None else [int(k) for k in np.flatnonzero(lens == rir.shape[1])]
    last = None
    for k in slots:
        try:
            spectra = _entry_spectra(bank.spectra[k].cpu().numpy(), bank.scales[k].cpu().numpy(), rir)
        except AssertionError as e:
            last = e
            continue
        return R.model_audiogoal(clip, None, t0, sr, spectra=spectra)
    raise AssertionError(f"no resident entry holds this RIR's spectrum (length {rir.shape[1]}, candidates {slots}): {last}")


def _units(sr, n):
    """silent | empty RIR | the 3-s clip in its last second through the 3-block RIR, then live units over all three RIRs and both
    sounds, every fifth with a distractor term"""
    from ss_amd.renderer import UnitRequest
    t0 = P.window_start_sim(3 * sr, sr, 2)
    units = [UnitRequest(1, t0, 0), UnitRequest(silent=True), UnitRequest(0, 0, 1)][:max(n, 1)]
    for k in range(3, n):
        snd = k % 2
        units.append(UnitRequest(snd, t0 if snd else 0, (0, 2, 3)[k % 3], dis_sound=1 - snd if k % 5 == 0 else -1,
                                 dis_rir=2 if k % 5 == 0 else -1))
    return units[:n]


def _close(a, b, label):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any() and not np.isnan(b).any(), label
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()
    print(f"[gpu_spec_half_rows] {label}: max |half - fp32(dequantised)| / peak = {err:.3e}")
    assert err <= AB, (label, err)


# ---- 1. the dequantised A/B of the stateless entries -----------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n_units", [(44100, 1), (44100, 5), (44100, 43), (44100, 150), (48000, 5), (48000, 150), (20000, 5)])
def test_rows_spec16_entries_equal_fp32_entries_fed_dequantised_spectra(sr, n_units):
    """1 and 5 units: k_obs_blocks (with parts); 43: the first size k_obs_rows takes; 150: 300 rows on 256 CUs, the persistent
    walk; out_len 20 000: two output blocks"""
    from ss_amd import ops
    w = _world(sr)
    r = w.r
    plan = r.plan(_units(sr, n_units))
    lens = r.rirs.lengths
    n_mels = 64 if n_units % 2 else 40
    msd, mwd = _mel(sr, n_mels)
    N, T, sgs = n_units, 1 + sr // 160, r.spectrogram_shape
    res = {}
    for name, bank, scale in (("half", w.h16, w.hs), ("fp32", w.deq, None)):
        ag, sg = _new(N, 2, sr), _new(N, *sgs)                           # with the waveform buffer
        ops.audio_obs_spec_into(r._spec, bank, lens, plan.desc, ag, sg, sr, sr, flags=plan.flags, hscale=scale)
        sg_only = _new(N, *sgs)                                          # without
        ops.audio_obs_spec_into(r._spec, bank, lens, plan.desc, None, sg_only, sr, sr, flags=plan.flags, hscale=scale)
        kw = dict(flags=plan.flags) if scale is None else dict(flags=plan.flags, hscale=scale)
        ag2, sg2, lm = _new(N, 2, sr), _new(N, *sgs), _new(N, n_mels, T, 2)
        ops.audio_obs_logmel_rows_spec_into(r._spec, bank, lens, plan.desc, ag2, sg2, lm, msd, mwd, sr, sr, EPS, "reflect", **kw)
        lm_only = _new(N, n_mels, T, 2)                                  # log-mel alone: no buffer at all
        ops.audio_obs_logmel_rows_spec_into(r._spec, bank, lens, plan.desc, None, None, lm_only, msd, mwd, sr, sr, EPS, "reflect", **kw)
        res[name] = dict(ag=ag, sg=sg, sg_only=sg_only, mel_ag=ag2, mel_sg=sg2, logmel=lm, logmel_only=lm_only)
    torch.cuda.synchronize()
    h, f = res["half"], res["fp32"]
    for k in h:
        _close(h[k], f[k], f"sr {sr} n {n_units} {k}")
    assert torch.equal(h["mel_ag"], h["ag"])                             # the log-mel launch's waveform: the same bits
    assert torch.equal(h["sg_only"], h["sg"]) and torch.equal(h["logmel_only"], h["logmel"])
    assert bool(h["ag"][0].abs().max() > 0)
    for u in (1, 2):                                                     # silent / empty RIR: exact zeros, log(mel_eps)
        if u < N:
            for k in ("ag", "sg", "sg_only", "mel_ag", "mel_sg"):
                assert not h[k][u].any(), (k, u)
            assert np.allclose(h["logmel"][u].cpu().numpy(), np.log(EPS), rtol=1e-6)


def test_rows_spec16_entry_against_the_quantised_model():
    """the stateless launch at 44.1 kHz (k_obs_blocks) against the float64 model with the same quantiser: every RIR block of the
    3-block entries is audible, so a dropped or mis-scaled block would show as ~1e-1"""
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    sr = 44100
    w = _world(sr)
    r = w.r
    t0 = P.window_start_sim(3 * sr, sr, 2)
    units = [UnitRequest(1, t0, 0), UnitRequest(0, 0, 3), UnitRequest(0, 0, 2, dis_sound=1, dis_rir=3)]
    plan = r.plan(units)
    ag, sg = _new(3, 2, sr), _new(3, *r.spectrogram_shape)
    ops.audio_obs_spec_into(r._spec, w.h16, r.rirs.lengths, plan.desc, ag, sg, sr, sr, flags=plan.flags, hscale=w.hs)
    torch.cuda.synchronize()
    ag, sg = ag.cpu().numpy(), sg.cpu().numpy()

    h16, hs = w.h16.cpu().numpy(), w.hs.cpu().numpy()

    def model(sound, t, rir):
        return R.model_audiogoal(w.srcs[sound], None, t, sr, spectra=_entry_spectra(h16[rir], hs[rir], w.rows[rir][:, :w.lens[rir]]))
    refs = [model(1, t0, 0), model(0, 0, 3), model(0, 0, 2) + model(1, 0, 3)]
    for n, ref in enumerate(refs):
        _vs_model(ag[n], sg[n], ref, f"stateless unit {n}")


# ---- 2. producer -------------------------------------------------------------------------------------------------------------------
def test_half_store_at_44k_equals_numpy_quantisation_of_the_fp32_store():
    from ss_amd.renderer import RirStore
    sr = 44100
    rng = np.random.default_rng(9)
    wavs = [np.ascontiguousarray(O.synth_rir_blocks(rng, sr, n, n=1)[0].T) for n in (44100, 9000, 16385)]
    wavs[1] = wavs[1] * np.float32(1e-6)
    stores = {}
    for form in ("half", "only"):
        st = RirStore(4, sr, DEV, spectral=form)
        slots = [st.slot(f"k{i}", (lambda h=h: h)) for i, h in enumerate(wavs)]
        st.sync_spectra()
        stores[form] = (st, slots)
    torch.cuda.synchronize()
    half, hs_slots = stores["half"]
    only, on_slots = stores["only"]
    assert half.bank.spectra.dtype == torch.float16 and tuple(half.bank.spectra.shape) == (4, 2, 3, P.SPEC_FLOATS)
    assert only.bank.spectra.dtype == torch.float32
    want_q, want_s = R.quantise(only.bank.spectra.cpu().numpy())
    got_q, got_s = half.bank.spectra.cpu().numpy(), half.bank.scales.cpu().numpy()
    assert not np.isnan(got_q).any()
    for a, b in zip(hs_slots, on_slots):
        assert np.array_equal(got_q[a], want_q[b]) and got_s[a].tobytes() == want_s[b].tobytes(), (a, b)
        assert int(half.bank.lengths[a]) == int(only.bank.lengths[b])


# ---- 3. AudioEngine(rir_spectral="half", rir_half_rows=True) -------------------------------------------------------------------
def _vs_model(got_ag, got_sg, ref, label, oracle=None):
    """waveform and pooled spectrogram against the model's, <= 1e-4 of peak; prints the distance to `oracle` (unquantised)"""
    ea = O.relerr(got_ag, ref)
    es = O.relerr(got_sg, O.compute_spectrogram(ref.astype(np.float32))) if got_sg is not None else 0.0
    msg = f"[gpu_spec_half_rows] {label}: vs quantised model waveform {ea:.3e} spectrogram {es:.3e}"
    if oracle is not None:
        msg += f"; vs UNQUANTISED oracle waveform {O.relerr(got_ag, oracle):.3e}"
        if got_sg is not None:
            msg += f" spectrogram {O.relerr(got_sg, O.compute_spectrogram(oracle.astype(np.float32))):.3e}"
    print(msg)
    assert ea <= BUDGET and es <= BUDGET, (label, ea, es)


def _sim_world(sr, seed=3):
    """test_deferred.make_world at `sr`: a 1-s and a 3-s sound, 16 RIR files of 9 000 .. sr taps"""
    rng = np.random.default_rng(seed)
    sounds = {"telephone.wav": O.synth_sources(rng, sr, k=1)[0], "long.wav": O.synth_sources(rng, sr, k=1, seconds=3)[0]}
    files = {}
    for az in (0, 90, 180, 270):
        for rc in range(4):
            n = int(rng.integers(9000, sr + 1))
            files[f"rirs/replica/apartment_0/{az}/{rc}_7.wav"] = np.ascontiguousarray(O.synth_rir_blocks(rng, sr, n, n=1)[0].T)
    return sounds, files


def test_engine_vector_observer_step_with_evictions():
    """3 in-process envs wandering over 16 poses through a half store of 6 entries at 44.1 kHz (loads evict), 1-s and 3-s clips"""
    from fakes import FakeSim
    from ss_amd import sim_audio
    from ss_amd.renderer import AudioEngine
    from test_deferred import apply, trajectory
    sr = 44100
    sounds, files = _sim_world(sr)
    eng = AudioEngine(sr, device=DEV, rir_slots=6, rir_spectral="half", rir_half_rows=True)
    assert eng.store.spectral_half and eng.store.bank.spectra16 is not None and eng.store.bank.data.numel() == 0
    assert eng.store.bank.spectra.shape[2] == 3
    sims = [FakeSim(sr, sounds, files, False) for _ in range(3)]
    obs = sim_audio.VectorAudioObserver(eng, [sim_audio.attach(s, eng, rir_reader=files.get) for s in sims], want_audiogoal=True)
    trajs = [trajectory(rk, 4) for rk in range(3)]
    for k in range(4):
        for rk, s in enumerate(sims):
            apply(s, k, trajs[rk][k])
        idx = [s._audio_index for s in sims]
        out = obs.observe()
        torch.cuda.synchronize()
        ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
        for rk, s in enumerate(sims):
            wav = files[f"rirs/replica/apartment_0/{s.azimuth_angle}/{s._receiver_position_index}_{s._source_position_index}.wav"]
            clip = sounds[s._current_sound]
            t0 = 0 if len(clip) == sr else idx[rk] * sr
            oracle = np.asarray(O.compute_audiogoal(clip, wav, sr, audio_index=idx[rk]))
            _vs_model(ag[rk], sg[rk], _bank_model(eng.store.bank, clip, wav, t0, sr), f"vector step {k} env {rk}", oracle=oracle)
    assert eng.store.misses > 6 and len(eng.store._slot_of) <= 6
    assert eng.store.bank.spectra.dtype == torch.float16 and eng.store.bank.scales is not None


def test_engine_c_context_route_with_logmel_and_the_cross_fade_refusal():
    """a C-context step at 44.1 kHz: the log-mel rows entry inside set_logmel_rows_policy((1, 42)), the waveform-scratch route
    outside that range, spectrogram + waveform, waveform alone; a cross-faded request raises and leaves the outputs alone"""
    from ss_amd import _lib
    from ss_amd.renderer import AudioEngine
    sr = 44100
    w = _world(sr)
    eng = AudioEngine(sr, device=DEV, rir_slots=4, rir_cap=49152, rir_spectral="half", rir_half_rows=True)
    for i, s in enumerate(w.srcs):
        eng.source_id(f"s{i}", s)                                        # (the 3-s clip: whole RIRs)
    wavs = [np.ascontiguousarray(w.rows[i][:, :w.lens[i]].T) for i in range(4)]
    sl = [eng.rir_slot(i, (lambda h=h: h)) for i, h in enumerate(wavs)]
    n = 6
    t0 = P.window_start_sim(3 * sr, sr, 2)
    sound = np.arange(n, dtype=np.int32) % 2
    cols = dict(sound=sound, t0=np.where(sound == 1, t0, 0).astype(np.int32), rir=np.asarray([sl[(0, 1, 2, 3, 0, 2)[i]] for i in range(n)], np.int32))
    which = (0, 1, 2, 3, 0, 2)
    ctx = eng._sync_context_bank(n, False)
    msd, mwd = _mel(sr)
    T = 1 + sr // 160
    torch.cuda.synchronize()
    refs = [None if which[i] == 1 else _bank_model(eng.store.bank, w.srcs[sound[i]], w.rows[which[i]][:, :w.lens[which[i]]],
                                                   int(cols["t0"][i]), sr, slot=sl[which[i]]) for i in range(n)]
    outs = {}
    for route, policy in (("fused", (1, 42)), ("scratch", (1, 0))):
        ctx.set_logmel_rows_policy(*policy)
        lm, sg = _new(n, 64, T, 2), _new(n, *ctx.spectrogram_shape)
        ctx.observe(spectrogram_out=sg, logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)      # no waveform buffer
        torch.cuda.synchronize()
        outs[route] = (lm.cpu().numpy(), sg.cpu().numpy())
        # inside the policy's range the step is ONE launch of the log-mel rows entry (no waveform anywhere); outside it the
        # context renders into its own waveform scratch
        assert (ctx.wave_scratch_bytes() == 0) == (route == "fused"), (route, ctx.wave_scratch_bytes())
    for route, (lmn, sgn) in outs.items():
        assert not np.isnan(lmn).any() and not np.isnan(sgn).any(), route
        for i in range(n):
            if refs[i] is None:                                          # the empty RIR
                assert not sgn[i].any() and np.allclose(lmn[i], np.log(EPS), rtol=1e-6)
                continue
            want = O.compute_logmel(refs[i].astype(np.float32), sr, n_mels=64, eps=EPS)
            err = np.abs(lmn[i] - want).max() / np.abs(want).max()
            es = O.relerr(sgn[i], O.compute_spectrogram(refs[i].astype(np.float32)))
            print(f"[gpu_spec_half_rows] context log-mel ({route}) unit {i}: vs quantised model log-mel {err:.3e} spectrogram {es:.3e}")
            assert err <= BUDGET and es <= BUDGET, (route, i, err, es)
    sg, ag, ag1 = _new(n, *ctx.spectrogram_shape), _new(n, 2, sr), _new(n, 2, sr)
    ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
    ctx.observe(audiogoal_out=ag1, **cols)                               # waveform alone: the unfused half convolution
    torch.cuda.synchronize()
    for i in range(n):
        if refs[i] is None:
            assert not ag[i].any() and not ag1[i].any() and not sg[i].any()
            continue
        wav = wavs[which[i]]
        oracle = np.asarray(O.compute_audiogoal(w.srcs[sound[i]], wav, sr, audio_index=2 if sound[i] else 0))
        _vs_model(ag[i].cpu().numpy(), sg[i].cpu().numpy(), refs[i], f"context unit {i}", oracle=oracle)
        _vs_model(ag1[i].cpu().numpy(), None, refs[i], f"context unit {i}, waveform alone")
    sg0 = sg.clone()
    with pytest.raises(_lib.SsHipError):                                 # a cross-faded step would read rows: SS_EINVAL
        ctx.observe(cols["sound"], cols["t0"], cols["rir"], spectrogram_out=sg, last_rir=cols["rir"][::-1].copy())
    torch.cuda.synchronize()
    assert torch.equal(sg, sg0)
    sg1 = _new(n, *ctx.spectrogram_shape)                                # the failed step left no keys behind: the next one is right
    ctx.observe(spectrogram_out=sg1, **cols)
    torch.cuda.synchronize()
    assert torch.equal(sg1, sg0)


def test_engine_deferred_resolver_with_the_in_call_loader(tmp_path):
    """DeferredResolver over 44.1 kHz RIR files on disk, 10 entries for up to 8 new poses per step (every step evicts): the
    library's in-call loader serves the binding through ss_bank_scatter_spectra16_f32 (ss_miss_loader.bank = NULL)"""
    from scipy.io import wavfile
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    NS = types.SimpleNamespace
    sr, n_nodes, n_env = 44100, 5, 8
    root = tmp_path / "rirs"
    rirs = {}
    for az in (0, 90):
        (root / str(az)).mkdir(parents=True)
        for rc in range(n_nodes):
            for sc in range(n_nodes):
                n = int(np.random.default_rng(7 * rc + sc).integers(5000, sr + 1))
                h = np.ascontiguousarray(O.synth_rir_blocks(np.random.default_rng(100 * az + 10 * rc + sc), sr, n, n=1)[0].T)
                p = str(root / str(az) / f"{rc}_{sc}.wav")
                wavfile.write(p, sr, h)
                rirs[p] = h
    clip = O.synth_sources(np.random.default_rng(5), sr, k=1)[0]

    class Sim:
        config = NS(AUDIO=NS(RIR_SAMPLING_RATE=sr, HAS_DISTRACTOR_SOUND=False), USE_RENDERED_OBSERVATIONS=True)
        binaural_rir_dir = str(root)
        _source_sound_dict = {"s.wav": clip}
        _current_sound, _audio_index, _episode_step_count, _duration = "s.wav", 0, 0, 500
        _receiver_position_index = _source_position_index = 0
        azimuth_angle = 0
        current_source_sound = property(lambda self: clip)
        _audio_length = 1

    sims = [Sim() for _ in range(n_env)]
    for i, sm in enumerate(sims):
        attach_deferred(sm, env_rank=i)
    eng = AudioEngine(sr, device=DEV, rir_slots=10, rir_spectral="half", rir_half_rows=True)
    res = DeferredResolver(eng, fast=True, prefetch_azimuths=False)
    res.native_miss_path = True
    walk = np.random.default_rng(3)
    for step in range(3):
        for sm in sims:
            sm._receiver_position_index, sm._source_position_index = int(walk.integers(0, n_nodes)), int(walk.integers(0, n_nodes))
            sm.azimuth_angle = int(walk.choice([0, 90]))
            sm._episode_step_count += 1
        reqs = [pickle.loads(pickle.dumps(sm.get_current_spectrogram_observation(None))) for sm in sims]
        out = res.resolve(reqs, want_audiogoal=True)
        torch.cuda.synchronize()
        ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
        for i, sm in enumerate(sims):
            p = os.path.join(str(root), str(sm.azimuth_angle), f"{sm._receiver_position_index}_{sm._source_position_index}.wav")
            _vs_model(ag[i], sg[i], _bank_model(res.engine.store.bank, clip, rirs[p], 0, sr), f"deferred step {step} env {i}")
    st = res.engine.store
    assert st.spectral_half and st.misses > 10 and len(st._slot_of) <= 10 and res.library_loaded > 10
    assert st.bank.spectra.dtype == torch.float16 and st.bank.spectra.shape[2] == 3


def test_engine_bank_growth_from_two_blocks_to_three():
    """whole RIRs (a 3-s clip is registered) in a store of capacity 20 000 (two blocks per row): a 40 000-tap RIR grows the half
    bank to three - the old entries' halves and scales are unchanged bit for bit, their new block zero with a finite scale"""
    from ss_amd.renderer import AudioEngine, UnitRequest
    sr = 44100
    w = _world(sr)
    eng = AudioEngine(sr, device=DEV, rir_slots=4, rir_cap=20000, rir_spectral="half", rir_half_rows=True)
    for i, s in enumerate(w.srcs):
        eng.source_id(f"s{i}", s)                                        # (the 3-s clip: truncate_to = None from here on)
    t0 = P.window_start_sim(3 * sr, sr, 2)
    rows_a, rows_b = w.rows[0][:, :20000], w.rows[2][:, :9000]
    a = eng.rir_slot("a", lambda: np.ascontiguousarray(rows_a.T))
    b = eng.rir_slot("b", lambda: np.ascontiguousarray(rows_b.T))
    eng.begin_batch()
    out = eng.observe([UnitRequest(1, t0, a), UnitRequest(0, 0, b)], want_audiogoal=True)
    torch.cuda.synchronize()
    assert eng.store.bank.spectra.shape[2] == 2
    old_q, old_s = eng.store.bank.spectra.clone(), eng.store.bank.scales.clone()
    bank = eng.store.bank
    ref_a, ref_b = _bank_model(bank, w.srcs[1], rows_a, t0, sr, slot=a), _bank_model(bank, w.srcs[0], rows_b, 0, sr, slot=b)
    _vs_model(out["audiogoal"][0].cpu().numpy(), out["spectrogram"][0].cpu().numpy(), ref_a, "before growth")
    c = eng.rir_slot("c", lambda: np.ascontiguousarray(w.rows[3][:, :40000].T))
    eng.begin_batch()
    out = eng.observe([UnitRequest(1, t0, a), UnitRequest(0, 0, b), UnitRequest(1, t0, c)], want_audiogoal=True)
    torch.cuda.synchronize()
    q, s = eng.store.bank.spectra, eng.store.bank.scales
    assert eng.store.grown == 1 and q.shape[2] == 3 and s.shape[2] == 3 and eng.renderer.rirs is eng.store.bank
    for sl in (a, b):
        assert torch.equal(q[sl, :, :2].view(torch.int16), old_q[sl].view(torch.int16)) and torch.equal(s[sl, :, :2], old_s[sl])
        assert not q[sl, :, 2:].view(torch.int16).any() and bool(torch.isfinite(s[sl, :, 2:]).all())
    ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
    _vs_model(ag[0], sg[0], ref_a, "after growth, old entry a")
    _vs_model(ag[1], sg[1], ref_b, "after growth, old entry b")
    _vs_model(ag[0], sg[0], _bank_model(eng.store.bank, w.srcs[1], rows_a, t0, sr, slot=a), "after growth, old entry a from the grown bank")
    _vs_model(ag[2], sg[2], _bank_model(eng.store.bank, w.srcs[1], w.rows[3][:, :40000], t0, sr, slot=c), "after growth, the 3-block entry")


# ---- 4. HBM ---------------------------------------------------------------------------------------------------------------------
def test_half_engine_holds_twice_the_entries_of_only_at_44k():
    """1024 entries at 44.1 kHz: the half engine allocates entries * 2 * 3 * (64 KiB + 4 B) plus the length table - half of what
    the spectral-only engine allocates for its fp32 spectra (profiles/r7/NOTES.md has the figures)"""
    from ss_amd.renderer import AudioEngine
    sr, slots, hb = 44100, 1024, 3
    torch.zeros(1, device=DEV)
    deltas = {}
    for form, kw in (("half", dict(rir_half_rows=True)), ("only", {})):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(0)
        eng = AudioEngine(sr, device=DEV, rir_slots=slots, rir_spectral=form, **kw)
        torch.cuda.synchronize()
        deltas[form] = torch.cuda.memory_allocated(0) - before
        spectra_bytes = eng.store.bank.spectra.numel() * eng.store.bank.spectra.element_size()
        print(f"[gpu_spec_half_rows] 44.1 kHz, {slots} entries, rir_spectral={form!r}: engine allocates {deltas[form]} bytes "
              f"(spectra {spectra_bytes}); per entry {spectra_bytes // slots}")
        assert eng.store.bank.data.numel() == 0 and len(eng.store.bank) == slots
        if form == "half":
            assert spectra_bytes == slots * 2 * hb * (64 << 10) and eng.store.bank.scales.numel() == slots * 2 * hb
        else:
            assert spectra_bytes == slots * 2 * hb * (128 << 10)
        del eng
    ratio = deltas["only"] / deltas["half"]
    print(f"[gpu_spec_half_rows] HBM of 'only' / HBM of 'half' at {slots} entries = {ratio:.4f}")
    # next to the spectra (384 / 768 MiB) both engines allocate the same things - the renderer's window-spectra cache (64 slots of
    # 128 KiB = 8 MiB), the length table - and the half one 24 KiB of scales: under 16 MiB a side, (768 + 16) / (384 + 16) = 1.96
    assert 1.96 <= ratio <= 2.0, ratio
