"""The half-precision spectral RIR bank on the GPU (include/ss_hip.h "Half-precision spectral bank"): fp16 block spectra with one
power-of-two fp32 scale per (entry, ear, block), k_stage_spectra16 / k_conv_spec<.., HALF>, RirStore(spectral="half"),
AudioEngine(rir_spectral="half").  16 kHz, row capacities 16000 (one RIR block: the loop-free kernels) and 40000 (three blocks:
the loop kernels).

  * producers: bit-for-bit the numpy quantisation (tests/spec_half_ref.py) of ss_rir_spectra_f32's output;
  * consumers: each *_spec16_* entry against its _spec_f32 sibling fed float(q) * hscale, <= 2e-6 of peak (each fp32 path is held
    to <= 1e-6 of peak against float64 by the project's parity record, the inputs are identical; the host build measures 0.0);
  * end to end against the overlap-save model with the same quantiser, <= 1e-4 of peak (the project's budget; the model's own
    distance to the oracle, 2.4e-7, is checked on the CPU in tests/test_spec_half_host.py).  The distance to the UNQUANTISED
    oracle is printed, not asserted: it is the format's accuracy."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_half_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 16000
BUDGET = 1e-4
AB = 2e-6
EPS = 1e-6
CAPS = [16000, 40000]


def _same_halves(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape
    assert not np.isnan(got).any()
    return np.array_equal(got, want)                                     # (+0 == -0)


@pytest.fixture(scope="module")
def world():
    """sources (two 1-s clips, one 3-s clip) and, per capacity, a planar bank of 3 entries: 0 live (as long as the capacity,
    every block audible), 1 empty, 2 a 9000-tap RIR"""
    rng = np.random.default_rng(17)
    srcs = list(O.synth_sources(rng, SR, k=2, seconds=1)) + [O.synth_sources(rng, SR, k=1, seconds=3)[0]]
    short = O.synth_rir(rng, SR, length=9000, n=1)[0]
    banks = {}
    for cap in CAPS:
        rows = np.zeros((3, 2, cap), np.float32)
        rows[0] = O.synth_rir(rng, SR, length=cap, n=1)[0] if cap <= P.KB else O.synth_rir_blocks(rng, SR, cap, n=1)[0]
        rows[2, :, :9000] = short
        banks[cap] = (rows, np.asarray([cap, 0, 9000], np.int32))
    return types.SimpleNamespace(srcs=srcs, banks=banks)


def _model(w, cap, sound, t0, rir, quant=True):
    rows, lens = w.banks[cap]
    return R.model_audiogoal(w.srcs[sound], rows[rir][:, :lens[rir]], t0, SR, quant=quant)


def _renderer(w, cap):
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    rows, lens = w.banks[cap]
    r = BatchedAudioRenderer(SR, device=DEV)
    for i, s in enumerate(w.srcs):
        r.add_source(f"s{i}", s)
    bank = torch.from_numpy(rows).to(DEV)
    r.set_rir_bank(RirBank(bank, torch.from_numpy(lens).to(DEV)))
    h16, hs = ops.rir_spectra16(bank)
    deq = (h16.float() * hs[..., None]).contiguous()                     # float(q) * hscale, exact in fp32
    return r, h16, hs, deq


# ---- 1. producers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_producers_equal_numpy_quantisation(world, cap):
    from ss_amd import ops
    rows, lens = world.banks[cap]
    hb = P.ceil_div(cap, P.KB)
    bank = torch.from_numpy(rows).to(DEV)
    want_q, want_s = R.quantise(ops.rir_spectra(bank).cpu().numpy())     # ss_rir_spectra_f32's output through the numpy rule
    h16, hs = ops.rir_spectra16(bank)                                    # ss_rir_spectra16_f32
    torch.cuda.synchronize()
    assert _same_halves(h16.cpu().numpy(), want_q) and hs.cpu().numpy().tobytes() == want_s.tobytes()
    assert not h16[1].view(torch.int16).any() and bool((hs[1] == 1.0).all())             # the empty entry: halves +0, scale 1
    slots = np.asarray([5, 1, 3], np.int32)
    entries = 7
    garbage = rows.copy()
    for i, n in enumerate(lens):
        garbage[i, :, n:] = np.nan                                       # behind a row's length nothing is read
    for from_host in (True, False):                                      # ss_bank_scatter_spectra16_f32, both staging memories
        for layout in ("wav", "planar"):
            stage = torch.from_numpy(np.ascontiguousarray(garbage.transpose(0, 2, 1) if layout == "wav" else garbage))
            pidx, plen = torch.from_numpy(slots.copy()), torch.from_numpy(lens.copy())
            if from_host:
                stage, pidx, plen = stage.pin_memory(), pidx.pin_memory(), plen.pin_memory()
            else:
                stage, pidx, plen = stage.to(DEV), pidx.to(DEV), plen.to(DEV)
            q = torch.zeros((entries, 2, hb, P.SPEC_FLOATS), dtype=torch.float16, device=DEV)
            s = torch.zeros((entries, 2, hb), device=DEV)
            blen = torch.full((entries,), -5, dtype=torch.int32, device=DEV)
            ops.scatter_spectra_into(stage, layout == "planar", pidx, plen, 3, q, blen, hscale=s)
            torch.cuda.synchronize()
            qn, sn = q.cpu().numpy(), s.cpu().numpy()
            for i in range(3):
                assert _same_halves(qn[slots[i]], want_q[i]), (layout, from_host, i)
                assert sn[slots[i]].tobytes() == want_s[i].tobytes(), (layout, from_host, i)
            assert blen.cpu().numpy()[slots].tolist() == lens.tolist()
            others = np.setdiff1d(np.arange(entries), slots)
            assert not qn[others].view(np.uint16).any() and not sn[others].any() and (blen.cpu().numpy()[others] == -5).all()


# ---- 2. the dequantised A/B --------------------------------------------------------------------------------------------------
def _units(cap, n):
    """n = 3: one silent unit, one with the empty RIR, one live; n = 40: those three, then live units over both RIRs, all three
    sounds (the 3-s clip in its last second) and - every fifth - a distractor term"""
    from ss_amd.renderer import UnitRequest
    units = [UnitRequest(silent=True), UnitRequest(0, 0, 1), UnitRequest(0, 0, 0)]
    for k in range(3, n):
        snd = k % 3
        units.append(UnitRequest(snd, 2 * SR if snd == 2 else 0, 0 if k % 2 else 2, dis_sound=(k + 1) % 2 if k % 5 == 0 else -1,
                                 dis_rir=2 if k % 5 == 0 else -1))
    return units


def _close(a, b, label):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any() and not np.isnan(b).any(), label
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()
    print(f"[gpu_spec_half] {label}: max |half - fp32(dequantised)| / peak = {err:.3e}")
    assert err <= AB, (label, err)


@pytest.mark.parametrize("n_units", [3, 40])
@pytest.mark.parametrize("cap", CAPS)
def test_spec16_entries_equal_fp32_entries_fed_dequantised_spectra(world, cap, n_units):
    from ss_amd import ops
    r, h16, hs, deq = _renderer(world, cap)
    plan = r.plan(_units(cap, n_units))
    lens = r.rirs.lengths
    ms, mw, _ = P.mel_filterbank_sparse(SR, 64)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    T = 1 + SR // 160

    def nan(*shape):
        return torch.full(shape, float("nan"), device=DEV)
    res = {}
    for name, bank, scale in (("half", h16, hs), ("fp32", deq, None)):
        conv = nan(n_units, 2, SR)
        ops.fftconv_binaural_spec_into(r._spec, bank, lens, plan.desc, conv, r.n_valid, flags=plan.flags, hscale=scale)
        ag, sg = nan(n_units, 2, SR), nan(n_units, *r.spectrogram_shape)
        ops.audio_obs_spec_into(r._spec, bank, lens, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags, hscale=scale)
        ag2, sg2, lm = nan(n_units, 2, SR), nan(n_units, *r.spectrogram_shape), nan(n_units, 64, T, 2)
        ops.audio_obs_logmel_spec_into(r._spec, bank, lens, plan.desc, ag2, sg2, lm, msd, mwd, r.n_valid, r.out_len, mel_eps=EPS,
                                       flags=plan.flags, hscale=scale)
        res[name] = dict(conv=conv, ag=ag, sg=sg, mel_ag=ag2, mel_sg=sg2, logmel=lm)
    torch.cuda.synchronize()
    for k in res["half"]:
        _close(res["half"][k], res["fp32"][k], f"cap {cap} n {n_units} {k}")
    h = res["half"]
    for u in (0, 1):                                                     # silent / empty RIR: exact zeros, log(mel_eps)
        for k in ("conv", "ag", "sg", "mel_ag", "mel_sg"):
            assert not h[k][u].any(), (k, u)
        assert torch.equal(h["logmel"][u], res["fp32"]["logmel"][u])
        assert np.allclose(h["logmel"][u].cpu().numpy(), np.log(EPS), rtol=1e-6)
    assert bool(h["ag"][2].abs().max() > 0)


@pytest.mark.parametrize("cap", CAPS)
def test_context_steps_use_the_unit_table_and_equal_the_fp32_binding(world, cap):
    """40 units through two C contexts - one bound to the half bank (ss_ctx_set_rir_spectra16), one to the dequantised fp32
    spectra (the spectral-only binding): the context hands the launch its unit table (k_conv_spec<.., SIMPLE, TAB, .., HALF> on
    one-block rows); spectrogram + waveform, waveform alone, and the one-launch log-mel route."""
    from ss_amd.context import AudioContext
    r, h16, hs, deq = _renderer(world, cap)
    lens = r.rirs.lengths
    units = _units(cap, 40)
    cols = dict(sound=np.asarray([u.sound for u in units], np.int32), t0=np.asarray([u.t0 for u in units], np.int32),
                rir=np.asarray([-1 if u.silent else u.rir for u in units], np.int32))
    if cap > P.KB:                                                       # (one-block rows stay on the loop-free kernel)
        cols["dis_sound"] = np.asarray([u.dis_sound for u in units], np.int32)
        cols["dis_rir"] = np.asarray([u.dis_rir for u in units], np.int32)
    ms, mw, _ = P.mel_filterbank_sparse(SR, 64)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    outs = []
    for half in (True, False):
        ctx = AudioContext(SR)
        for i, s in enumerate(world.srcs):
            ctx.add_source(f"s{i}", s)
        if half:
            ctx.set_rir_spectra16(h16, hs, lens, cap)
        else:
            ctx.set_rir_spectra_only(deq, lens, cap)
        sg = torch.full((40,) + ctx.spectrogram_shape, float("nan"), device=DEV)
        ag, ag1 = torch.full((40, 2, SR), float("nan"), device=DEV), torch.full((40, 2, SR), float("nan"), device=DEV)
        lm = torch.full((40, 64, 1 + SR // 160, 2), float("nan"), device=DEV)
        ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
        ctx.observe(audiogoal_out=ag1, **cols)
        ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
        torch.cuda.synchronize()
        outs.append(dict(sg=sg, ag=ag, ag_only=ag1, logmel=lm))
        ctx.close()
    for k in outs[0]:
        _close(outs[0][k], outs[1][k], f"context cap {cap} {k}")
    for u in (0, 1):
        assert not outs[0]["ag"][u].any() and not outs[0]["sg"][u].any()
        assert np.allclose(outs[0]["logmel"][u].cpu().numpy(), np.log(EPS), rtol=1e-6)


# ---- 3. end to end against the quantised model ---------------------------------------------------------------------------------
def _vs_model(got_ag, got_sg, ref, label, oracle=None):
    """waveform and pooled spectrogram against the model's, <= 1e-4 of peak; prints the distance to `oracle` (unquantised)"""
    ea = O.relerr(got_ag, ref)
    es = O.relerr(got_sg, O.compute_spectrogram(ref.astype(np.float32))) if got_sg is not None else 0.0
    msg = f"[gpu_spec_half] {label}: vs quantised model waveform {ea:.3e} spectrogram {es:.3e}"
    if oracle is not None:
        msg += f"; vs UNQUANTISED oracle waveform {O.relerr(got_ag, oracle):.3e}"
        if got_sg is not None:
            msg += f" spectrogram {O.relerr(got_sg, O.compute_spectrogram(oracle.astype(np.float32))):.3e}"
    print(msg)
    assert ea <= BUDGET and es <= BUDGET, (label, ea, es)


@pytest.mark.parametrize("cap", CAPS)
def test_fused_launch_against_the_quantised_model(world, cap):
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    r, h16, hs, _ = _renderer(world, cap)
    rows, lens = world.banks[cap]
    units = [UnitRequest(silent=True), UnitRequest(0, 0, 1), UnitRequest(0, 0, 0), UnitRequest(2, 2 * SR, 0), UnitRequest(1, 0, 2)]
    plan = r.plan(units)
    ag, sg = torch.full((5, 2, SR), float("nan"), device=DEV), torch.full((5,) + r.spectrogram_shape, float("nan"), device=DEV)
    ops.audio_obs_spec_into(r._spec, h16, r.rirs.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags, hscale=hs)
    torch.cuda.synchronize()
    ag, sg = ag.cpu().numpy(), sg.cpu().numpy()
    assert not ag[:2].any() and not sg[:2].any()
    for n, u in enumerate(units[2:], start=2):
        wav = np.ascontiguousarray(rows[u.rir][:, :lens[u.rir]].T)
        oracle = O.compute_audiogoal(world.srcs[u.sound], wav, SR, audio_index=u.t0 // SR)
        _vs_model(ag[n], sg[n], _model(world, cap, u.sound, u.t0, u.rir), f"fused cap {cap} unit {n}", oracle=np.asarray(oracle))


# ---- 4. AudioEngine(rir_spectral="half") ----------------------------------------------------------------------------------------
def _model_of_file(clip, wav, t0):
    return R.model_audiogoal(clip, np.ascontiguousarray(np.asarray(wav, np.float32).T), t0, SR)


def test_engine_vector_observer_with_evictions(world):
    """4 in-process envs wandering over 32 poses through a half store of 8 entries (loads evict), 1-s and 3-s clips"""
    from fakes import FakeSim
    from ss_amd import sim_audio
    from ss_amd.renderer import AudioEngine
    from test_deferred import apply, make_world, trajectory
    sounds, files = make_world()
    eng = AudioEngine(SR, device=DEV, rir_slots=8, rir_spectral="half")
    assert eng.store.spectral_half and eng.store.bank.spectra16 is not None and eng.store.bank.data.numel() == 0
    sims = [FakeSim(SR, sounds, files, False) for _ in range(4)]
    obs = sim_audio.VectorAudioObserver(eng, [sim_audio.attach(s, eng, rir_reader=files.get) for s in sims], want_audiogoal=True)
    trajs = [trajectory(rk, 6) for rk in range(4)]
    for k in range(6):
        for rk, s in enumerate(sims):
            apply(s, k, trajs[rk][k])
        idx = [s._audio_index for s in sims]
        out = obs.observe()
        torch.cuda.synchronize()
        ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
        for rk, s in enumerate(sims):
            wav = files[f"rirs/replica/apartment_0/{s.azimuth_angle}/{s._receiver_position_index}_{s._source_position_index}.wav"]
            clip = sounds[s._current_sound]
            t0 = 0 if len(clip) == SR else idx[rk] * SR
            _vs_model(ag[rk], sg[rk], _model_of_file(clip, wav, t0), f"vector step {k} env {rk}")
    assert eng.store.misses > 8 and len(eng.store._slot_of) <= 8
    assert eng.store.bank.spectra.dtype == torch.float16 and eng.store.bank.scales is not None


def test_engine_deferred_resolver_with_the_in_call_loader(tmp_path):
    """DeferredResolver over RIR files on disk, 10 entries for up to 8 new poses per step: the library's in-call loader serves the
    half binding through ss_bank_scatter_spectra16_f32 (ss_miss_loader.bank = NULL)"""
    from scipy.io import wavfile
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    NS = types.SimpleNamespace
    n_nodes, n_env = 6, 8
    root = tmp_path / "rirs"
    rirs = {}
    for az in (0, 90):
        (root / str(az)).mkdir(parents=True)
        for rc in range(n_nodes):
            for sc in range(n_nodes):
                n = int(np.random.default_rng(7 * rc + sc).integers(2000, 16001))
                h = np.ascontiguousarray(O.synth_rir(np.random.default_rng(100 * az + 10 * rc + sc), SR, length=n, n=1)[0].T)
                p = str(root / str(az) / f"{rc}_{sc}.wav")
                wavfile.write(p, SR, h)
                rirs[p] = h
    clip = O.synth_sources(np.random.default_rng(5), SR, k=1)[0]

    class Sim:
        config = NS(AUDIO=NS(RIR_SAMPLING_RATE=SR, HAS_DISTRACTOR_SOUND=False), USE_RENDERED_OBSERVATIONS=True)
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
    res = DeferredResolver(AudioEngine(SR, device=DEV, rir_slots=10, rir_spectral="half"), fast=True, prefetch_azimuths=False)
    res.native_miss_path = True
    walk = np.random.default_rng(3)
    for step in range(4):
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
            _vs_model(ag[i], sg[i], _model_of_file(clip, rirs[p], 0), f"deferred step {step} env {i}")
    st = res.engine.store
    assert st.spectral_half and st.misses > 10 and len(st._slot_of) <= 10 and res.library_loaded > 10
    assert st.bank.spectra.dtype == torch.float16


def test_engine_c_context_route_with_logmel_and_the_cross_fade_refusal(world):
    from ss_amd import _lib
    from ss_amd.renderer import AudioEngine
    rows, lens = world.banks[16000]
    eng = AudioEngine(SR, device=DEV, rir_slots=4, rir_spectral="half")
    for i, s in enumerate(world.srcs[:2]):
        eng.source_id(f"s{i}", s)
    wavs = [np.ascontiguousarray(rows[i][:, :lens[i]].T) for i in range(3)]
    sl = [eng.rir_slot(i, (lambda h=h: h)) for i, h in enumerate(wavs)]
    n = 6
    cols = dict(sound=np.arange(n, dtype=np.int32) % 2, t0=np.zeros(n, np.int32), rir=np.asarray([sl[i % 3] for i in range(n)], np.int32))
    ctx = eng._sync_context_bank(n, False)
    ms, mw, _ = P.mel_filterbank_sparse(SR, 64)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    lm = torch.full((n, 64, 1 + SR // 160, 2), float("nan"), device=DEV)
    sg = torch.full((n,) + ctx.spectrogram_shape, float("nan"), device=DEV)
    ctx.observe(spectrogram_out=sg, logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)      # one launch, no waveform
    torch.cuda.synchronize()
    lmn, sgn = lm.cpu().numpy(), sg.cpu().numpy()
    assert not np.isnan(lmn).any() and not np.isnan(sgn).any()
    for i in range(n):
        if i % 3 == 1:                                                   # the empty RIR
            assert not sgn[i].any() and np.allclose(lmn[i], np.log(EPS), rtol=1e-6)
            continue
        ref = _model(world, 16000, i % 2, 0, i % 3)
        want = O.compute_logmel(ref.astype(np.float32), SR, n_mels=64, eps=EPS)
        err = np.abs(lmn[i] - want).max() / np.abs(want).max()
        es = O.relerr(sgn[i], O.compute_spectrogram(ref.astype(np.float32)))
        print(f"[gpu_spec_half] context log-mel unit {i}: vs quantised model log-mel {err:.3e} spectrogram {es:.3e}")
        assert err <= BUDGET and es <= BUDGET
    sg0 = sg.clone()
    with pytest.raises(_lib.SsHipError):                                 # a cross-faded step would read rows: SS_EINVAL
        ctx.observe(cols["sound"], cols["t0"], cols["rir"], spectrogram_out=sg, last_rir=cols["rir"][::-1].copy())
    torch.cuda.synchronize()
    assert torch.equal(sg, sg0)


def test_engine_bank_growth_from_one_block_to_three(world):
    """whole RIRs (a 3-s clip is registered): a 40000-tap RIR grows the half bank from one block per row to three - the old
    entries' halves and scales are unchanged bit for bit, their new blocks zero with finite scales"""
    from ss_amd.renderer import AudioEngine, UnitRequest
    rows16, lens16 = world.banks[16000]
    rows40, lens40 = world.banks[40000]
    eng = AudioEngine(SR, device=DEV, rir_slots=4, rir_spectral="half")
    for i, s in enumerate(world.srcs):
        eng.source_id(f"s{i}", s)                                        # (the 3-s clip: truncate_to = None from here on)
    a = eng.rir_slot("a", lambda: np.ascontiguousarray(rows16[0].T))
    b = eng.rir_slot("b", lambda: np.ascontiguousarray(rows16[2][:, :9000].T))
    eng.begin_batch()
    out = eng.observe([UnitRequest(2, 2 * SR, a), UnitRequest(0, 0, b)], want_audiogoal=True)
    torch.cuda.synchronize()
    assert eng.store.bank.spectra.shape[2] == 1
    old_q, old_s = eng.store.bank.spectra.clone(), eng.store.bank.scales.clone()
    _vs_model(out["audiogoal"][0].cpu().numpy(), out["spectrogram"][0].cpu().numpy(), _model(world, 16000, 2, 2 * SR, 0), "before growth")
    c = eng.rir_slot("c", lambda: np.ascontiguousarray(rows40[0].T))
    eng.begin_batch()
    out = eng.observe([UnitRequest(2, 2 * SR, a), UnitRequest(0, 0, b), UnitRequest(2, 2 * SR, c)], want_audiogoal=True)
    torch.cuda.synchronize()
    q, s = eng.store.bank.spectra, eng.store.bank.scales
    assert eng.store.grown == 1 and q.shape[2] == 3 and s.shape[2] == 3 and eng.renderer.rirs is eng.store.bank
    for sl in (a, b):
        assert torch.equal(q[sl, :, :1].view(torch.int16), old_q[sl].view(torch.int16)) and torch.equal(s[sl, :, :1], old_s[sl])
        assert not q[sl, :, 1:].view(torch.int16).any() and bool(torch.isfinite(s[sl, :, 1:]).all())
    ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
    _vs_model(ag[0], sg[0], _model(world, 16000, 2, 2 * SR, 0), "after growth, old entry a")
    _vs_model(ag[1], sg[1], _model(world, 16000, 0, 0, 2), "after growth, old entry b")
    _vs_model(ag[2], sg[2], _model(world, 40000, 2, 2 * SR, 0), "after growth, the 3-block entry")


# ---- 5. HBM ---------------------------------------------------------------------------------------------------------------------
def test_half_store_allocates_halves_scales_and_lengths_only():
    """entries * 2 * h_blocks * (64 KiB + 4 B) plus the length table: no rows, no fp32 spectra"""
    from ss_amd.renderer import RirStore
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    slots, cap = 64, 40000
    hb = P.ceil_div(cap, P.KB)
    before = torch.cuda.memory_allocated(0)
    st = RirStore(slots, cap, DEV, spectral="half")
    torch.cuda.synchronize()
    delta = torch.cuda.memory_allocated(0) - before

    def granule(nbytes):                                                 # (the caching allocator's 512-byte granule)
        return -(-nbytes // 512) * 512
    assert st.bank.data.numel() == 0 and len(st.bank) == slots and st.bank.cap == cap
    assert st.bank.spectra.dtype == torch.float16 and tuple(st.bank.spectra.shape) == (slots, 2, hb, P.SPEC_FLOATS)
    assert st.bank.spectra.element_size() * P.SPEC_FLOATS == 64 << 10
    assert delta == granule(slots * 2 * hb * (64 << 10)) + granule(slots * 2 * hb * 4) + granule(slots * 4), delta
