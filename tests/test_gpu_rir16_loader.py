"""Pose misses served inside the step's call on half-precision time-domain rows (include/ss_hip.h: ss_miss_loader.stage_max,
``ss_bank_scatter_rows16_max_f32`` / k_scatter_rows16_max, ``ss_wav_read_rirs_max_f32``), on the GPU:

  a. the one-pass scatter against ``ss_bank_scatter_rows16_f32``, byte for byte, staging in pinned host and in device memory, 5 rows
     at cap 2000 and 3 rows at cap 44100, lengths on chunk seams;
  b. deferred steps with misses - the world of tests/test_wav_loader.py::test_pose_misses_are_served_inside_the_step_s_call (6 nodes,
     2 azimuths, 8 envs, 6 steps, one int16 file) on ``AudioEngine(16000, rir_rows="half")``: in-call against the three-call path
     bit-equal, the store's books, the entries' halves and scales against ``rir16_ref.quantise`` of their files, the outputs within
     the bound tests/test_gpu_time_rir16.py applies against the float64 model (1e-4), a 10-entry store that evicts inside the call;
  c. eager calls: ``AudioEngine.rir_file_slot`` goes through ``ss_ctx_load_rir_files`` (answer 0) and leaves ``load_files``' bytes;
  d. 44.1 kHz on the fused binding (``rir_rows16_fused=True``): one deferred step of 5 envs, all misses;
  e. overlap mode: the loader rewrites an entry that queued steps read - their outputs are unchanged (the half-store twin of
     tests/test_wav_loader.py::test_in_call_loader_orders_its_scatter_behind_steps_in_flight).

(The file's name sorts it behind tests/test_gpu_spec*.py: see tests/test_gpu_time_rir16.py.)"""
import os
import pickle
import types

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
from test_gpu_time_rir16 import BUDGET, _vs_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = types.SimpleNamespace


# ---- a. the scatter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,lens", [(2000, (2000, 0, 511, 512, 513)), (44100, (44100, 22016, 22017))])
def test_one_pass_scatter_equals_the_two_pass_scatter(cap, lens):
    from ss_amd import ops
    rng = np.random.default_rng(cap)
    n = len(lens)
    staged = np.full((n, cap, 2), np.nan, np.float32)                    # wav layout, NaN behind every row's length
    planar = np.zeros((n, 2, cap), np.float32)
    for i, ln in enumerate(lens):
        x = (rng.standard_normal((ln, 2)) * 10.0 ** (i - 2)).astype(np.float32)
        staged[i, :ln] = x
        planar[i, :, :ln] = x.T
    row_max = np.abs(planar).max(2).astype(np.float32)
    want_q, want_s = R.quantise(planar)
    slots = np.asarray([2 * i + 1 for i in range(n)], np.int32)[::-1].copy()
    entries = int(slots.max()) + 2
    lens_np = np.asarray(lens, np.int32)
    lens_np[0] = cap + 9                                                 # clamped
    for from_host in (True, False):
        arrs = [torch.from_numpy(a.copy()) for a in (staged, slots, lens_np, row_max)]
        arrs = [a.pin_memory() if from_host else a.to(DEV) for a in arrs]
        stage, pidx, plen, pmax = arrs
        banks = []
        for one_pass in (True, False):
            q = torch.full((entries, 2, cap), 3.0, dtype=torch.float16, device=DEV)
            s = torch.full((entries, 2), 9.0, device=DEV)
            bl = torch.full((entries,), -5, dtype=torch.int32, device=DEV)
            if one_pass:
                ops.scatter_rows16_max_into(stage, pidx, plen, pmax, n, q, s, bl)
            else:
                ops.scatter_rows16_into(stage, pidx, plen, n, q, s, bl)
            torch.cuda.synchronize()
            banks.append((q.cpu().numpy(), s.cpu().numpy(), bl.cpu().numpy()))
        for a, b in zip(*banks):
            assert a.tobytes() == b.tobytes(), from_host
        qn, sn, bn = banks[0]
        for i in range(n):
            assert qn[slots[i]].tobytes() == np.ascontiguousarray(want_q[i]).tobytes(), (from_host, i)
            assert sn[slots[i]].tobytes() == np.ascontiguousarray(want_s[i]).tobytes(), (from_host, i)
        assert bn[slots].tolist() == list(lens)
        others = np.setdiff1d(np.arange(entries), slots)
        assert (qn[others] == 3.0).all() and (sn[others] == 9.0).all() and (bn[others] == -5).all()
    with pytest.raises(ValueError, match="pinned"):                      # pageable maxima are refused like the other staged arrays
        ops.scatter_rows16_max_into(stage, pidx, plen, torch.from_numpy(row_max.copy()), n, q, s, bl)


# ---- the deferred world -------------------------------------------------------------------------------------------------------------
def _sim_class(sr, root, clip):
    class Sim:
        config = NS(AUDIO=NS(RIR_SAMPLING_RATE=sr, HAS_DISTRACTOR_SOUND=False), USE_RENDERED_OBSERVATIONS=True)
        binaural_rir_dir = str(root)
        _source_sound_dict = {"s.wav": clip}
        _current_sound, _audio_index, _episode_step_count, _duration = "s.wav", 0, 0, 500
        _receiver_position_index = _source_position_index = 0
        azimuth_angle = 0
        current_source_sound = property(lambda self: clip)
        _audio_length = 1
    return Sim


def _path_of(root, sm):
    return os.path.join(str(root), str(sm.azimuth_angle), f"{sm._receiver_position_index}_{sm._source_position_index}.wav")


@pytest.fixture(scope="module")
def world16(tmp_path_factory):
    """6 nodes x 6 nodes x 2 azimuths of float32 wav files (one of them int16) at 16 kHz and a 1-s clip; the float64 model of a
    file's observation is computed once per file and kept"""
    sr, n_nodes = 16000, 6
    rng = np.random.default_rng(11)
    root = tmp_path_factory.mktemp("rir16_loader") / "rirs"
    rirs = {}
    for az in (0, 90):
        (root / str(az)).mkdir(parents=True)
        for r in range(n_nodes):
            for s_ in range(n_nodes):
                L = int(rng.integers(2000, 16001))
                h = O.synth_rir(np.random.default_rng(100 * az + 10 * r + s_), sr, length=L, n=1)[0]
                p = str(root / str(az) / f"{r}_{s_}.wav")
                if (az, r, s_) == (90, 5, 5):                    # one file scipy reads but the library's reader hands back
                    wavfile.write(p, sr, (h.T * 20000).astype(np.int16))
                    rirs[p] = (h.T * 20000).astype(np.int16).astype(np.float32)
                else:
                    wavfile.write(p, sr, np.ascontiguousarray(h.T))
                    rirs[p] = np.ascontiguousarray(h.T)
    clip = O.synth_sources(np.random.default_rng(5), sr, k=1)[0]
    models = {}

    def model(path):
        if path not in models:
            models[path] = R.model_audiogoal(clip, np.ascontiguousarray(rirs[path].T), 0, sr)
        return models[path]
    return NS(sr=sr, n_nodes=n_nodes, root=root, rirs=rirs, clip=clip, model=model)


def _run16(w, in_call, slots, n_env=8, steps=6):
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    Sim = _sim_class(w.sr, w.root, w.clip)
    sims = [Sim() for _ in range(n_env)]
    for i, sm in enumerate(sims):
        attach_deferred(sm, env_rank=i)
    res = DeferredResolver(AudioEngine(w.sr, device=DEV, rir_slots=slots, rir_rows="half"), fast=True, prefetch_azimuths=False)
    res.native_miss_path = in_call
    outs = []
    walk = np.random.default_rng(3)
    for k in range(steps):
        for sm in sims:
            sm._receiver_position_index, sm._source_position_index = int(walk.integers(0, w.n_nodes)), int(walk.integers(0, w.n_nodes))
            sm.azimuth_angle = int(walk.choice([0, 90]))
            sm._episode_step_count += 1
        if k == 4:
            sims[0]._receiver_position_index = sims[0]._source_position_index = 5
            sims[0].azimuth_angle = 90                           # the int16 file
        reqs = [pickle.loads(pickle.dumps(sm.get_current_spectrogram_observation(None))) for sm in sims]
        out = res.resolve(reqs, want_audiogoal=True)
        torch.cuda.synchronize()
        outs.append((out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy(), [_path_of(w.root, sm) for sm in sims]))
    return res, outs


def test_deferred_pose_misses_are_served_inside_the_call_on_half_rows(world16):
    w = world16
    res_a, a = _run16(w, True, 256)
    res_b, b = _run16(w, False, 256)
    assert res_a.library_loaded >= 20 and res_b.library_loaded == 0
    store = res_a.engine.store
    assert store.rows_half and store.bank.data.dtype == torch.float16
    assert len(store._slot_of) == store.misses and len(store._free) == store.slots - len(store._slot_of)
    qd, sd, ld = store.bank.data.cpu().numpy(), store.bank.scales.cpu().numpy(), store.bank.lengths.cpu().numpy()
    for (key, slot) in store._slot_of.items():                   # the store's books agree with what the library wrote
        assert key[0] == "ix" and store._key_at[slot] == key and store._used[slot]
        k = key[1]
        path = os.path.join(res_a._table_dirs[k >> 40], f"{(k >> 20) & 0xFFFFF}_{k & 0xFFFFF}.wav")
        n = min(w.rirs[path].shape[0], 16000)
        assert int(store.host_len[slot]) == n == int(ld[slot])
        assert int(res_a._pair_slots[np.searchsorted(res_a._pair_keys, k)]) == slot
        row = np.zeros((2, store.cap), np.float32)               # halves and scales: the numpy rule on the file's samples
        row[:, :n] = w.rirs[path][:n].T
        q, s = R.quantise(row)
        assert qd[slot].tobytes() == np.ascontiguousarray(q).tobytes(), path
        assert sd[slot].tobytes() == np.ascontiguousarray(s).tobytes(), path
    assert np.all(np.diff(res_a._pair_keys) > 0)
    qb, sb = res_b.engine.store.bank.data.cpu().numpy(), res_b.engine.store.bank.scales.cpu().numpy()
    for key, slot in store._slot_of.items():                     # ... and equal to what load_files left on the three-call path
        sl_b = res_b.engine.store._slot_of[key]
        assert qd[slot].tobytes() == qb[sl_b].tobytes() and sd[slot].tobytes() == sb[sl_b].tobytes()
    for (ag1, sg1, _), (ag2, sg2, _) in zip(a, b):
        np.testing.assert_array_equal(ag1, ag2)
        np.testing.assert_array_equal(sg1, sg2)
    for step, env in [(0, i) for i in range(4)] + [(4, 0), (5, 3)]:   # envs of the first step, the int16 file, a late step
        ag, sg, paths = a[step]
        _vs_model(ag[env], sg[env], w.model(paths[env]), f"half rows in-call step {step} env {env}")
    assert a[4][2][0].endswith(os.path.join("90", "5_5.wav"))
    res_c, c = _run16(w, True, 10)                               # 10 entries for up to 8 new poses per step: the library evicts
    st_c = res_c.engine.store
    assert st_c.misses > 10 and res_c.library_loaded > 10 and len(st_c._slot_of) <= 10
    assert sorted(st_c._slot_of.values()) == sorted(np.flatnonzero(st_c._used).tolist())
    assert sorted(int(v) for v in res_c._pair_slots) == sorted(st_c._slot_of[k_] for k_ in st_c._slot_of if k_[0] == "ix")
    for (ag1, sg1, _), (ag3, sg3, _) in zip(a, c):
        np.testing.assert_array_equal(ag1, ag3)
        np.testing.assert_array_equal(sg1, sg3)
    res_d, d = _run16(w, False, 10)                              # ... exactly like the store's own eviction path
    assert res_d.library_loaded == 0
    for (ag1, _, _), (ag4, _, _) in zip(a, d):
        np.testing.assert_array_equal(ag1, ag4)


# ---- c. eager calls -----------------------------------------------------------------------------------------------------------------
def test_eager_file_slot_goes_through_the_library_on_half_rows(world16, monkeypatch):
    from ss_amd import _lib
    from ss_amd.renderer import AudioEngine
    from ss_amd.sim_audio import wav_rir_reader
    w = world16
    lib = _lib.load()
    real = lib.ss_ctx_load_rir_files
    answers = []

    def counted(*args):
        rc = real(*args)
        answers.append(rc)
        return rc
    monkeypatch.setattr(lib, "ss_ctx_load_rir_files", counted)
    paths = [str(w.root / "0" / "1_2.wav"), str(w.root / "90" / "3_4.wav"), str(w.root / "90" / "5_5.wav")]     # the last: int16
    eng = AudioEngine(w.sr, device=DEV, rir_slots=8, rir_rows="half")
    slots = []
    for p in paths:
        eng.begin_batch()
        slots.append(eng.rir_file_slot(p, wav_rir_reader))
    torch.cuda.synchronize()
    assert answers.count(0) >= 1 and answers == [0, 0, 1]               # served, served, handed back (scipy's semantics)
    monkeypatch.undo()
    eng2 = AudioEngine(w.sr, device=DEV, rir_slots=8, rir_rows="half")
    ref = eng2.store.load_files(paths, paths, reader=wav_rir_reader)
    torch.cuda.synchronize()
    for p, a, b in zip(paths, slots, ref):
        assert eng.store.bank.data[a].cpu().numpy().tobytes() == eng2.store.bank.data[b].cpu().numpy().tobytes(), p
        assert eng.store.bank.scales[a].cpu().numpy().tobytes() == eng2.store.bank.scales[b].cpu().numpy().tobytes(), p
        assert int(eng.store.bank.lengths[a]) == int(eng2.store.bank.lengths[b]) == eng.store.host_len[a] == min(len(w.rirs[p]), 16000)
    assert eng.store.misses == 3 and eng.rir_file_slot(paths[0], wav_rir_reader) == slots[0]      # a hit: no further call
    assert len(answers) == 3


# ---- d. 44.1 kHz, the fused binding ----------------------------------------------------------------------------------------------------
def test_deferred_step_44100_fused_binding_all_misses(tmp_path):
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    sr, n_env = 44100, 5
    root = tmp_path / "rirs"
    (root / "0").mkdir(parents=True)
    files = {}
    # source 7: the step under test; source 6: a first step (a resolver's first step registers the sound and the directory in
    # Python and loads its files there, whatever the store)
    for sc, all_taps in ((7, (44100, 20000, 9000, 30001, 44100)), (6, (3000,) * 5)):
        for rc, taps in enumerate(all_taps):
            rng = np.random.default_rng(2000 + 10 * sc + rc)
            h = (O.synth_rir(rng, sr, length=taps, n=1) if taps <= P.KB else O.synth_rir_blocks(rng, sr, taps, n=1))[0]
            h = np.ascontiguousarray(h.T.astype(np.float32))
            p = str(root / "0" / f"{rc}_{sc}.wav")
            wavfile.write(p, sr, h)
            files[p] = h
    clip = O.synth_sources(np.random.default_rng(6), sr, k=1)[0]
    Sim = _sim_class(sr, root, clip)

    def run(in_call):
        sims = [Sim() for _ in range(n_env)]
        for i, sm in enumerate(sims):
            attach_deferred(sm, env_rank=i)
        eng = AudioEngine(sr, device=DEV, rir_slots=16, rir_rows="half", rir_rows16_fused=True)
        res = DeferredResolver(eng, fast=True, prefetch_azimuths=False)
        res.native_miss_path = in_call
        for sc in (6, 7):
            for i, sm in enumerate(sims):
                sm._receiver_position_index, sm._source_position_index = i, sc
                sm._episode_step_count += 1
            reqs = [pickle.loads(pickle.dumps(sm.get_current_spectrogram_observation(None))) for sm in sims]
            out = res.resolve(reqs, want_audiogoal=True)
            torch.cuda.synchronize()
            assert res.library_loaded == (n_env if in_call and sc == 7 else 0)      # the second step: ONE call, all five poses
        return res, out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()

    res_a, ag_a, sg_a = run(True)
    res_b, ag_b, sg_b = run(False)
    assert res_a.library_loaded == n_env and res_b.library_loaded == 0
    assert tuple(sg_a.shape[1:]) == (65, 69, 2)
    np.testing.assert_array_equal(ag_a, ag_b)
    np.testing.assert_array_equal(sg_a, sg_b)
    sa, sb = res_a.engine.store, res_b.engine.store
    assert sa.cap == sb.cap == sr
    for key, slot in sa._slot_of.items():
        assert sa.bank.data[slot].cpu().numpy().tobytes() == sb.bank.data[sb._slot_of[key]].cpu().numpy().tobytes()
        assert sa.bank.scales[slot].cpu().numpy().tobytes() == sb.bank.scales[sb._slot_of[key]].cpu().numpy().tobytes()
    for env in (0, 3):                                                   # a full row and one that ends inside a chunk
        wav = files[str(root / "0" / f"{env}_7.wav")]
        _vs_model(ag_a[env], sg_a[env], R.model_audiogoal(clip, np.ascontiguousarray(wav.T), 0, sr), f"44100 fused in-call env {env}")


# ---- e. overlap mode ------------------------------------------------------------------------------------------------------------------
def test_in_call_loader_orders_its_scatter_behind_steps_in_flight_on_half_rows(tmp_path):
    """Overlap mode + a half-rows store of three entries: thirty large steps that read entry A are queued on the lanes, then a new
    pose is loaded by the library's loader (ss_ctx_load_rir_files), which evicts the least recently used entry - A - while those
    steps are still in flight.  The one-pass scatter goes on the caller's stream: it has to wait for the lanes."""
    from ss_amd import _lib
    from ss_amd.renderer import AudioEngine
    from ss_amd.sim_audio import wav_rir_reader
    sr, n_units, n_steps = 16000, 512, 30
    rng = np.random.default_rng(21)
    paths = []
    for k in range(4):
        p = str(tmp_path / f"{k}_0.wav")
        wavfile.write(p, sr, np.ascontiguousarray(O.synth_rir(rng, sr, length=16000, n=1)[0].T))
        paths.append(p)
    clip = O.synth_sources(rng, sr, k=1)[0]
    eng = AudioEngine(sr, device=DEV, rir_slots=3, rir_rows="half")
    sid = eng.source_id("s", clip)
    slots = []
    for p in paths[:3]:
        eng.begin_batch()
        slots.append(eng.rir_file_slot(p, wav_rir_reader))
    ctx = eng.context()
    cols = dict(sound=np.full(n_units, sid), t0=np.zeros(n_units, np.int64), rir=np.full(n_units, slots[0]))
    ref = torch.empty((n_units, 65, 26, 2), device=DEV)
    eng.observe_columns(cols, spectrogram_out=ref)
    torch.cuda.synchronize()
    ctx.set_overlap(2)
    out = torch.zeros((n_steps, n_units, 65, 26, 2), device=DEV)
    torch.cuda.synchronize()
    lib = _lib.load()
    real, answers = lib.ss_ctx_load_rir_files, []

    def counted(*args):
        answers.append(real(*args))
        return answers[-1]
    for k in range(n_steps):
        eng.observe_columns(cols, spectrogram_out=out[k])
    eng.begin_batch()
    lib.ss_ctx_load_rir_files = counted
    try:
        new = eng.rir_file_slot(paths[3], wav_rir_reader)           # evicts A (= slots[0]) inside ONE C call, steps still queued
    finally:
        lib.ss_ctx_load_rir_files = real
    assert answers == [0] and new == slots[0] and eng.store.misses == 4
    ctx.join()
    torch.cuda.synchronize()
    for k in range(n_steps):
        assert torch.equal(out[k], ref), k
    sg = torch.empty((1, 65, 26, 2), device=DEV)                    # ... and the new pose renders from the rewritten entry
    eng.observe_columns(dict(sound=np.array([sid]), t0=np.zeros(1, np.int64), rir=np.array([new])), spectrogram_out=sg)
    ctx.join()
    torch.cuda.synchronize()
    model = R.model_audiogoal(clip, np.ascontiguousarray(wav_rir_reader(paths[3]).T), 0, sr)
    err = O.relerr(sg[0].cpu().numpy(), R.model_spectrogram(model))
    print(f"[gpu_rir16_loader] overlap: the new pose against the quantised float64 model {err:.3e}")
    assert err <= BUDGET, err
