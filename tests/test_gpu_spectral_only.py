"""Spectral-only RIR banks (AudioEngine(rir_spectral="only"), RirStore(spectral="only")): the block spectra and the lengths,
no time-domain rows.  Staged rows are transformed on their way in (ss_bank_scatter_spectra_f32, k_stage_spectra); every step
reads the spectra.  Against ss_rir_spectra_f32 of the scattered rows (bit-identical), the oracle (<= 1e-4 of peak, exact
zeros for silent units) and a both-forms engine fed the same inputs (identical outputs)."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4


def check(got, ref, tol=TOL):
    got = np.asarray(got)
    assert not np.isnan(got).any()
    assert O.relerr(got, ref) <= tol, O.relerr(got, ref)


def _engines(sr, **kw):
    from ss_amd.renderer import AudioEngine
    return (AudioEngine(sr, device=DEV, rir_spectral="only", **kw), AudioEngine(sr, device=DEV, rir_spectral=True, **kw))


# ---- 1. the scatter against ss_rir_spectra_f32 of the scattered rows ------------------------------------------------------
@pytest.mark.parametrize("cap", [16000, 44100])
@pytest.mark.parametrize("from_host", [True, False])
def test_scatter_spectra_bit_identical_to_rir_spectra_of_the_rows(cap, from_host):
    from ss_amd import _lib, ops
    rng = np.random.default_rng(cap + from_host)
    lens = np.asarray([0, 1, cap - 1, cap, min(cap, 16385), cap // 3], np.int32)
    R, hb = len(lens), P.ceil_div(cap, P.KB)
    planar = rng.standard_normal((R, 2, cap)).astype(np.float32)
    for i, n in enumerate(lens):
        planar[i, :, n:] = 0.0
    rows = torch.from_numpy(planar).to(DEV)
    ref = ops.rir_spectra(rows)                                          # ss_rir_spectra_f32 of the planar rows
    slots = np.arange(R, dtype=np.int32)[::-1] * 2 + 1
    entries = int(slots.max()) + 2
    lib = _lib.load()
    for layout in ("wav", "planar"):
        host = planar.transpose(0, 2, 1) if layout == "wav" else planar
        stage = torch.from_numpy(np.ascontiguousarray(host))
        pidx, plen = torch.from_numpy(slots.copy()), torch.from_numpy(lens)
        if from_host:
            stage, pidx, plen = stage.pin_memory(), pidx.pin_memory(), plen.pin_memory()
        else:
            stage, pidx, plen = stage.to(DEV), pidx.to(DEV), plen.to(DEV)
        hspec = torch.full((entries, 2, hb, P.SPEC_FLOATS), 7.0, device=DEV)
        blen = torch.full((entries,), -5, dtype=torch.int32, device=DEV)
        ops.scatter_spectra_into(stage, layout == "planar", pidx, plen, R, hspec, blen)
        torch.cuda.synchronize()
        got = hspec[torch.from_numpy(slots).long().to(DEV)]
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), layout
        assert blen.cpu().numpy()[slots].tolist() == lens.tolist()
        others = torch.from_numpy(np.setdiff1d(np.arange(entries), slots)).to(DEV)
        assert bool((hspec[others] == 7.0).all()) and bool((blen[others] == -5).all())
    # pageable host memory is refused (the kernel would fault on it), before anything is launched
    page = torch.zeros((R, cap, 2))
    rc = lib.ss_bank_scatter_spectra_f32(page.data_ptr(), 2 * cap, 0, pidx.data_ptr(), plen.data_ptr(), R, hspec.data_ptr(), hb,
                                         blen.data_ptr(), None)
    assert rc == -1


# ---- 2. observations against the oracle and against a both-forms engine ---------------------------------------------------
def _observe_both(engs, units, **kw):
    outs = []
    for e in engs:
        e.begin_batch()
        o = e.observe(units, **kw)
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    return outs[0]


@pytest.mark.parametrize("sr,n_units", [(16000, 64), (44100, 5), (44100, 512)])
def test_engine_steps_vs_oracle_and_both_forms(sr, n_units):
    """1-s clips at 16 kHz (fused kernel, distractors, silent and zero-RIR units), 44.1 kHz at 5 units (k_obs_blocks) and 512
    units (k_obs_rows); audiogoal-only steps and the intensity of the waveform as well."""
    from ss_amd.renderer import UnitRequest
    rng = np.random.default_rng(sr + n_units)
    src = O.synth_sources(rng, sr, k=3)
    rirs = [np.ascontiguousarray(O.synth_rir(rng, sr, length=int(rng.uniform(0.2, 1.0) * sr), n=1)[0].T) for _ in range(6)]
    rirs.append(np.zeros((0, 2), np.float32))                            # an empty file: the zero RIR
    engs = _engines(sr, rir_slots=16)
    slots = [[e.rir_slot(i, (lambda h=h: h)) for i, h in enumerate(rirs)] for e in engs]
    assert slots[0] == slots[1]
    assert engs[0].store.bank.data.numel() == 0 and engs[0].store.bank.spectral_only
    units, refs = [], []
    dis = sr == 16000
    for n in range(n_units):
        if n % 11 == 3:
            units.append(UnitRequest(silent=True))
            refs.append(None)
            continue
        s_, h_ = int(rng.integers(0, 3)), int(rng.integers(0, len(rirs)))
        d_ = dis and n % 3 == 0
        units.append(UnitRequest(s_, 0, slots[0][h_], dis_sound=(s_ + 1) % 3 if d_ else -1, dis_rir=slots[0][(h_ + 1) % 6] if d_ else -1))
        refs.append(O.compute_audiogoal(src[s_], rirs[h_], sr, distractor=src[(s_ + 1) % 3] if d_ else None,
                                        distractor_rir=rirs[(h_ + 1) % 6] if d_ else None))
    for e in engs:
        for i, s_ in enumerate(src):
            e.source_id(f"s{i}", s_)
    out = _observe_both(engs, units, want_audiogoal=True)
    ag_only = _observe_both(engs, units, want_spectrogram=False)["audiogoal"]
    np.testing.assert_array_equal(ag_only, out["audiogoal"])
    for n, ref in enumerate(refs):
        if ref is None or not ref.size or not np.abs(ref).max():
            assert not out["audiogoal"][n].any() and not out["spectrogram"][n].any()
            continue
        check(out["audiogoal"][n], ref)
        check(out["spectrogram"][n], O.compute_spectrogram(ref.astype(np.float32)))
    from ss_amd import ops
    inten = ops.intensity(torch.from_numpy(out["audiogoal"]).to(DEV)).cpu().numpy()       # (VectorAudioObserver want_intensity)
    assert np.isfinite(inten).all()


def test_multisecond_clips_and_bank_growth_through_the_eager_adapter():
    """Multi-second clips (whole RIRs: truncate_to = None) through sim_audio.attach: a 1.5-s RIR grows the spectral-only bank
    (old blocks copied, new blocks zero) and rows clipped before reload; 12 files through 4 slots (evictions).  Against the oracle
    and against a both-forms engine walking the same poses."""
    from fakes import FakeSim, NS
    from ss_amd import sensors, sim_audio
    sr = 16000
    rng = np.random.default_rng(5)
    sounds = {"a.wav": O.synth_sources(rng, sr, k=1)[0], "long.wav": O.synth_sources(rng, sr, k=1, seconds=3)[0]}
    files = {f"rirs/replica/apartment_0/{az}/{r}_7.wav": np.ascontiguousarray(O.synth_rir(rng, sr, length=L, n=1)[0].T)
             for az in (0, 90, 180, 270) for r, L in ((1, 9000), (2, 16000), (3, 24000))}
    outs = []
    for eng in _engines(sr, rir_slots=4):
        sim = FakeSim(sr, sounds, files)
        sim_audio.attach(sim, eng, rir_reader=files.get)
        sensor = sensors.AudioGoalSensor(sim=sim, config=NS())
        got = []
        for step in range(14):
            sim._receiver_position_index = 1 + step % 3
            sim._rotation_angle = (step * 90) % 360
            sim._current_sound = "long.wav" if step >= 7 else "a.wav"
            sim._audiogoal_cache, sim._spectrogram_cache = {}, {}
            idx = sim._audio_index
            a = sensor.get_observation(observations=None, episode=None)
            path = f"rirs/replica/apartment_0/{sim.azimuth_angle}/{sim._receiver_position_index}_7.wav"
            check(a, O.compute_audiogoal(sim.current_source_sound, files[path], sr, audio_index=idx))
            got.append(np.asarray(a))
        assert eng.store.grown == 1 and eng.store.bank.spectra.shape[2] == 2 and eng.renderer.rirs is eng.store.bank
        outs.append(got)
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_growth_keeps_old_blocks_and_zero_fills_new_ones():
    """RirStore(spectral='only')._ensure_cap: the grown spectra equal ss_rir_spectra_f32 of the rows at the new capacity."""
    from ss_amd import ops
    from ss_amd.renderer import RirStore
    sr = 16000
    rng = np.random.default_rng(9)
    rows = [np.ascontiguousarray(O.synth_rir(rng, sr, length=L, n=1)[0].T) for L in (9000, 16000, 3000)]
    st = RirStore(4, sr, DEV, truncate_to=None, spectral="only")
    for i, h in enumerate(rows):
        st.slot(i, lambda h=h: h)
    st.slot(9, lambda: np.ascontiguousarray(O.synth_rir(rng, sr, length=24000, n=1)[0].T))     # grows to 2 blocks
    torch.cuda.synchronize()
    assert st.grown == 1 and st.bank.spectra.shape[2] == 2
    planar = torch.zeros((4, 2, st.cap), device=DEV)
    for i, h in enumerate(rows):
        planar[i, :, :h.shape[0]] = torch.from_numpy(h.T.copy()).to(DEV)
    ref = ops.rir_spectra(planar)
    assert torch.equal(st.bank.spectra[:3], ref[:3])                    # (+0 fill vs the zero block's spectrum: equal values)


def test_c_context_steps_and_features_on_the_spectral_only_binding():
    """AudioContext.set_rir_spectra_only (ss_ctx_set_rir_bank(NULL) + ss_ctx_set_rir_spectra): a savi-shaped step with log-mel +
    GCC-PHAT (ss_ctx_observe_features) equals the both-forms engine's context; a cross-faded step is refused (SS_EINVAL) with the
    output buffers untouched."""
    from ss_amd import _lib
    sr, n = 16000, 12
    rng = np.random.default_rng(21)
    src = O.synth_sources(rng, sr, k=2)
    rirs = [np.ascontiguousarray(O.synth_rir(rng, sr, length=12000, n=1)[0].T) for _ in range(4)]
    outs = []
    for eng in _engines(sr, rir_slots=8):
        for i, s_ in enumerate(src):
            eng.source_id(f"s{i}", s_)
        sl = [eng.rir_slot(i, (lambda h=h: h)) for i, h in enumerate(rirs)]
        cols = dict(sound=np.arange(n, dtype=np.int32) % 2, t0=np.zeros(n, np.int32), rir=np.asarray([sl[i % 4] for i in range(n)], np.int32),
                    dis_sound=np.asarray([(i + 1) % 2 for i in range(n)], np.int32), dis_rir=np.asarray([sl[(i + 1) % 4] if i % 2 else -1 for i in range(n)], np.int32))
        ctx = eng._sync_context_bank(n, True)
        ms, mw, _ = P.mel_filterbank_sparse(sr, 64)
        msd, mwd = torch.from_numpy(ms).to(DEV), torch.from_numpy(mw).to(DEV)
        T = 1 + sr // 160
        sg = torch.full((n,) + ctx.spectrogram_shape, 9.0, device=DEV)
        ag = torch.full((n, 2, sr), 9.0, device=DEV)
        lm, gc = torch.full((n, 64, T, 2), 9.0, device=DEV), torch.full((n, 65, T), 9.0, device=DEV)
        f = ctx.features(lm, msd, mwd, 1e-6, gc, 32, 1e-8)
        ctx.observe_prepared_features(ctx.prepare(**cols), sg.data_ptr(), ag.data_ptr(), torch.cuda.current_stream().cuda_stream, f)
        torch.cuda.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (ag, sg, lm, gc)))
        if eng.rir_spectral_only:
            for i in range(n):
                ref = O.compute_audiogoal(src[i % 2], rirs[i % 4], sr, distractor=src[(i + 1) % 2] if i % 2 else None,
                                          distractor_rir=rirs[(i + 1) % 4] if i % 2 else None)
                check(outs[-1][0][i], ref)
            ag0, sg0 = ag.clone(), sg.clone()
            with pytest.raises(_lib.SsHipError):                        # cross-fade: the route reads rows
                ctx.observe(cols["sound"], cols["t0"], cols["rir"], spectrogram_out=sg, audiogoal_out=ag,
                            last_rir=cols["rir"][::-1].copy())
            torch.cuda.synchronize()
            assert torch.equal(ag, ag0) and torch.equal(sg, sg0)
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


# ---- 3. more poses than slots: rir_file_slot, DeferredResolver with the in-call loader ---------------------------------------
def _write_rirs(root, sr, n_nodes):
    from scipy.io import wavfile
    rirs = {}
    for az in (0, 90):
        (root / str(az)).mkdir(parents=True)
        for r in range(n_nodes):
            for s_ in range(n_nodes):
                L = int(np.random.default_rng(7 * r + s_).integers(2000, 16001))
                h = O.synth_rir(np.random.default_rng(100 * az + 10 * r + s_), sr, length=L, n=1)[0]
                p = str(root / str(az) / f"{r}_{s_}.wav")
                wavfile.write(p, sr, np.ascontiguousarray(h.T))
                rirs[p] = np.ascontiguousarray(h.T)
    return rirs


def test_rir_file_slot_with_evictions(tmp_path):
    from ss_amd.renderer import UnitRequest
    from ss_amd.sim_audio import wav_rir_reader
    sr = 16000
    rirs = _write_rirs(tmp_path, sr, 4)
    paths = sorted(rirs)
    clip = O.synth_sources(np.random.default_rng(2), sr, k=1)[0]
    outs = []
    for eng in _engines(sr, rir_slots=6):
        eng.source_id("s", clip)
        got = []
        for k, p in enumerate(paths[:20]):
            eng.begin_batch()
            slot = eng.rir_file_slot(p, wav_rir_reader)
            got.append(eng.observe([UnitRequest(0, 0, slot)], want_audiogoal=True)["audiogoal"][0].cpu().numpy())
            check(got[-1], O.compute_audiogoal(clip, rirs[p], sr))
        assert eng.store.misses == 20 and len(eng.store._slot_of) == 6
        outs.append(got)
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_deferred_resolver_in_call_loader_with_evictions(tmp_path):
    """ss_ctx_observe_requests_load on a spectral-only context: the library reads the new poses' files and writes their block
    spectra with one k_stage_spectra launch (ss_miss_loader.bank = NULL); 10 entries for up to 8 new poses per step."""
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    NS = types.SimpleNamespace
    sr, n_nodes, n_env = 16000, 6, 8
    root = tmp_path / "rirs"
    rirs = _write_rirs(root, sr, n_nodes)
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

    def run(mode):
        sims = [Sim() for _ in range(n_env)]
        for i, sm in enumerate(sims):
            attach_deferred(sm, env_rank=i)
        res = DeferredResolver(AudioEngine(sr, device=DEV, rir_slots=10, rir_spectral=mode), fast=True, prefetch_azimuths=False)
        res.native_miss_path = True
        outs = []
        walk = np.random.default_rng(3)
        for _ in range(6):
            for sm in sims:
                sm._receiver_position_index, sm._source_position_index = int(walk.integers(0, n_nodes)), int(walk.integers(0, n_nodes))
                sm.azimuth_angle = int(walk.choice([0, 90]))
                sm._episode_step_count += 1
            reqs = [pickle.loads(pickle.dumps(sm.get_current_spectrogram_observation(None))) for sm in sims]
            out = res.resolve(reqs, want_audiogoal=True)
            torch.cuda.synchronize()
            outs.append((out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy(),
                         [os.path.join(str(root), str(sm.azimuth_angle), f"{sm._receiver_position_index}_{sm._source_position_index}.wav") for sm in sims]))
        return res, outs

    res_a, a = run("only")
    res_b, b = run(True)
    st = res_a.engine.store
    assert st.spectral_only and res_a.library_loaded > 10 and st.misses > 10 and len(st._slot_of) <= 10
    for (ag1, sg1, paths), (ag2, sg2, _) in zip(a, b):
        np.testing.assert_array_equal(ag1, ag2)
        np.testing.assert_array_equal(sg1, sg2)
        for i, pth in enumerate(paths):
            ref = O.compute_audiogoal(clip, rirs[pth], sr)
            check(ag1[i], ref)
            check(sg1[i], O.compute_spectrogram(ref.astype(np.float32)))


# ---- 4. HBM ----------------------------------------------------------------------------------------------------------------
def test_spectral_only_store_allocates_spectra_and_lengths_only():
    """In a fresh process (nothing else allocating): the store's torch.cuda.memory_allocated delta is its spectra plus its
    lengths - no [slots, 2, cap] rows."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (f"import sys; sys.path[:0] = [{root!r}, {os.path.join(root, 'sound-spaces_amd')!r}]\n"
            "import json, torch\n"
            "from ss_amd.renderer import RirStore\n"
            "torch.zeros(1, device='cuda:0'); torch.cuda.synchronize()\n"
            "before = torch.cuda.memory_allocated(0)\n"
            "st = RirStore(64, 16000, 'cuda:0', spectral='only'); torch.cuda.synchronize()\n"
            "print(json.dumps([torch.cuda.memory_allocated(0) - before, st.bank.data.numel(), len(st.bank), st.bank.cap]))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    delta, rows, n, cap = json.loads(r.stdout.strip().splitlines()[-1])
    slots, sr = 64, 16000
    spec_bytes = slots * 2 * P.ceil_div(sr, P.KB) * P.SPEC_FLOATS * 4
    len_bytes = -(-slots * 4 // 512) * 512                              # (the caching allocator's 512-byte granule)
    assert rows == 0 and n == slots and cap == sr
    assert delta == spec_bytes + len_bytes, (delta, spec_bytes, len_bytes)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ss_amd.renderer import AudioEngine, RirStore
    with pytest.raises(ValueError):
        AudioEngine(16000, device=DEV, rir_spectral="only", step_time=0.25)
    with pytest.raises(ValueError):
        AudioEngine(16000, device=DEV, rir_spectral="only", rir_buckets=[(8, 16000), (4, 2 * P.KB)])
    with pytest.raises(ValueError):
        AudioEngine(16000, device=DEV, rir_spectral="only", spectral_max_units=64)
    with pytest.raises(ValueError):
        RirStore(8, 16000, "cpu", spectral="only")
