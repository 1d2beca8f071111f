"""Half-precision time-domain RIR rows on the GPU (include/ss_hip.h "Half-precision time-domain rows"): fp16 rows with one
power-of-two fp32 scale per (entry, ear), k_rows_half / k_scatter_rows16 / k_conv<.., HALF>, ss_ctx_set_rir_bank16,
RirStore(rows="half"), AudioEngine(rir_rows="half").  The two banks of tests/test_rir16_host.py.

  * producers: bit for bit the numpy rule (tests/rir16_ref.py), from a device bank and from staged rows in pinned host and in
    device memory, NaN behind every row's length;
  * consumers: each *_rir16_* entry, and a context bound to the half rows, against the fp32 sibling fed float(q) * scale on
    identical parameters, <= 2e-6 of peak (each fp32 path is held to <= 1e-6 of peak against float64 by the project's parity
    record, the inputs are identical; the host build measures 0.0) - at 5 units (rows split over CUs), 130 (the unit table,
    through a context) and 260 (past the table); silent units and the empty entry are exact zeros;
  * against the float64 model on the dequantised rows, <= 1e-4 of peak (the project's budget; the model's own distance to the
    oracle is checked on the CPU in tests/test_rir16_host.py);
  * end to end: AudioEngine(rir_rows="half") at 16 kHz (two wav files, eager and vector observations, the store's bytes) and at
    44.1 kHz (one vector step of 5 envs).

(The file's name sorts it behind tests/test_gpu_spec*.py: their allocation checks compare torch.cuda.memory_allocated with exact
byte counts, which holds only for the allocator cache the files in front of them leave behind.)"""
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
from test_rir16_host import make_banks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 16000
BUDGET = 1e-4
AB = 2e-6
EPS = 1e-6


@pytest.fixture(scope="module")
def world():
    """the two banks (numpy, read-only) and per sampling rate two 1-s clips and one 3-s clip; computed once"""
    srcs = {}
    for sr in (16000, 44100):
        rng = np.random.default_rng(sr)
        srcs[sr] = list(O.synth_sources(rng, sr, k=2, seconds=1)) + [O.synth_sources(rng, sr, k=1, seconds=3)[0]]
    return types.SimpleNamespace(banks=make_banks(), srcs=srcs)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _renderer(w, name, sr=SR, **kw):
    """a planner over the fp32 rows of bank `name`, its half form from the device (ss_rir_rows16_f32) and float(q) * scale"""
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    b = w.banks[name]
    r = BatchedAudioRenderer(sr, device=DEV, **kw)
    for i, s in enumerate(w.srcs[sr]):
        r.add_source(f"s{i}", s)
    rows = torch.from_numpy(b["rows"].copy()).to(DEV)                    # (the fixture's arrays are read-only)
    r.set_rir_bank(RirBank(rows, torch.from_numpy(b["lens"].copy()).to(DEV)))
    q, s = ops.rir_rows16(rows)
    deq = (q.float() * s[..., None]).contiguous()                        # float(q) * scale, exact in fp32
    return r, q, s, deq


# ---- 1. producers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "long"])
def test_producers_equal_the_numpy_rule(world, name):
    from ss_amd import ops
    b = world.banks[name]
    n, cap = b["rows"].shape[0], b["cap"]
    q, s = ops.rir_rows16(torch.from_numpy(b["rows"].copy()).to(DEV))    # ss_rir_rows16_f32
    torch.cuda.synchronize()
    assert q.cpu().numpy().tobytes() == b["q"].tobytes() and s.cpu().numpy().tobytes() == b["s"].tobytes()
    if name == "small":
        assert not q[1].view(torch.int16).any() and bool((s[1] == 1.0).all())       # the empty entry: +0 halves, scale 1
    staged = np.full((n, cap, 2), np.nan, np.float32)                    # wav layout, NaN behind every row's length
    for i, ln in enumerate(b["lens"]):
        staged[i, :ln] = b["rows"][i, :, :ln].T
    slots = np.asarray([2 * i + 1 for i in range(n)], np.int32)[::-1].copy()
    entries = int(slots.max()) + 2
    for from_host in (True, False):                                      # ss_bank_scatter_rows16_f32, both staging memories
        stage, pidx, plen = torch.from_numpy(staged), torch.from_numpy(slots.copy()), torch.from_numpy(b["lens"].copy())
        if from_host:
            stage, pidx, plen = stage.pin_memory(), pidx.pin_memory(), plen.pin_memory()
        else:
            stage, pidx, plen = stage.to(DEV), pidx.to(DEV), plen.to(DEV)
        q2 = torch.zeros((entries, 2, cap), dtype=torch.float16, device=DEV)
        s2 = torch.zeros((entries, 2), device=DEV)
        blen = torch.full((entries,), -5, dtype=torch.int32, device=DEV)
        ops.scatter_rows16_into(stage, pidx, plen, n, q2, s2, blen)
        torch.cuda.synchronize()
        qn, sn, bl = q2.cpu().numpy(), s2.cpu().numpy(), blen.cpu().numpy()
        for i in range(n):
            assert qn[slots[i]].tobytes() == b["q"][i].tobytes(), (from_host, i)
            assert sn[slots[i]].tobytes() == b["s"][i].tobytes(), (from_host, i)
        assert bl[slots].tolist() == b["lens"].tolist()
        others = np.setdiff1d(np.arange(entries), slots)
        assert not qn[others].view(np.uint16).any() and not sn[others].any() and (bl[others] == -5).all()
    with pytest.raises(ValueError, match="pinned"):                      # pageable host memory is refused
        ops.scatter_rows16_into(torch.from_numpy(staged), torch.from_numpy(slots.copy()).pin_memory(),
                                torch.from_numpy(b["lens"].copy()).pin_memory(), n, q2, s2, blen)


# ---- 2. the dequantised A/B through the C ABI ------------------------------------------------------------------------------------
def _units(name, n, sr=SR, distractor=False):
    """unit 0 silent, then live units over every entry of the bank (the empty one included) and all three sounds (the 3-s clip
    in its last second); distractor: every third live unit carries a term of ANOTHER entry"""
    from ss_amd.renderer import UnitRequest
    entries = 4 if name == "small" else 2
    units = [UnitRequest(silent=True)]
    for k in range(1, n):
        snd = k % 3
        dis = distractor and k % 3 == 0
        units.append(UnitRequest(snd, 2 * sr if snd == 2 else 0, k % entries, dis_sound=(k + 1) % 2 if dis else -1,
                                 dis_rir=(k + 1) % entries if dis else -1))
    return units


def _model_unit(w, name, u, sr, n_valid=None):
    b = w.banks[name]

    def term(sound, t0, rir):
        ln = int(b["lens"][rir])
        return R.model_audiogoal(w.srcs[sr][sound], b["rows"][rir][:, :ln], t0, sr, True, n_valid)
    ref = term(u.sound, u.t0, u.rir)
    if u.dis_rir is not None and u.dis_rir >= 0:
        ref = ref + term(u.dis_sound, 0, u.dis_rir)
    return ref


def _close(a, b, label):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any() and not np.isnan(b).any(), label
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()
    print(f"[gpu_rir16] {label}: max |half - fp32(dequantised)| / peak = {err:.3e}")
    assert err <= AB, (label, err)
    return a


def _vs_model(got_ag, got_sg, ref, label):
    ea = O.relerr(got_ag, ref)
    es = O.relerr(got_sg, R.model_spectrogram(ref)) if got_sg is not None else 0.0
    print(f"[gpu_rir16] {label}: vs quantised float64 model waveform {ea:.3e} spectrogram {es:.3e}")
    assert ea <= BUDGET and es <= BUDGET, (label, ea, es)


CASES = {                      # bank, distractor terms, renderer keywords
    "loop_free": ("small", False, {}),                                   # one RIR block, one term: the loop-free kernels
    "loop_distractor": ("small", True, {}),                              # a second term of another entry: the loop kernels
    "loop_three_rir_blocks": ("long", True, {}),
    "n_valid_4000": ("small", False, dict(step_time=0.25)),              # 4 000 of 16 000 samples rendered
}


@pytest.mark.parametrize("n_units", [5, 260])
@pytest.mark.parametrize("case", list(CASES))
def test_rir16_entries_equal_fp32_entries_fed_dequantised_rows(world, case, n_units):
    from ss_amd import ops
    name, dis, kw = CASES[case]
    r, q, s, deq = _renderer(world, name, **kw)
    units = _units(name, n_units, distractor=dis)
    plan = r.plan(units)
    lens = r.rirs.lengths
    assert bool(plan.flags & ops.FLAG_NO_DISTRACTOR) == (not dis)
    res = {}
    for form in ("half", "fp32"):
        conv, ag, sg, sg_only = _nan(n_units, 2, SR), _nan(n_units, 2, SR), _nan(n_units, *r.spectrogram_shape), _nan(n_units, *r.spectrogram_shape)
        if form == "half":
            ops.fftconv_binaural_rir16_into(r._spec, q, s, lens, plan.desc, conv, r.n_valid, flags=plan.flags)
            ops.audio_obs_rir16_into(r._spec, q, s, lens, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
            ops.audio_obs_rir16_into(r._spec, q, s, lens, plan.desc, None, sg_only, r.n_valid, r.out_len, flags=plan.flags)
        else:
            ops.fftconv_binaural_into(r._spec, deq, lens, plan.desc, conv, r.n_valid, flags=plan.flags)
            ops.audio_obs_into(r._spec, deq, lens, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
            ops.audio_obs_into(r._spec, deq, lens, plan.desc, None, sg_only, r.n_valid, r.out_len, flags=plan.flags)
        res[form] = dict(conv=conv, ag=ag, sg=sg, sg_only=sg_only)
    torch.cuda.synchronize()
    h = {k: _close(res["half"][k], res["fp32"][k], f"{case} n {n_units} {k}") for k in res["half"]}
    zero = [0] + ([k for k in range(1, n_units) if k % 4 == 1 and not units[k].dis_rir >= 0] if name == "small" else [])
    for u in zero[:8]:                                                   # silent / the empty entry: bit-exact zeros
        for k in h:
            assert not h[k][u].view(np.uint32).any(), (k, u)
    assert np.abs(h["ag"][2]).max() > 0 and np.array_equal(h["conv"], h["ag"])
    if r.n_valid < SR:
        assert not h["ag"][:, :, r.n_valid:].any()
    for u in range(2, 5):                                                # the first live units against the float64 model
        _vs_model(h["ag"][u], h["sg"][u], _model_unit(world, name, units[u], SR, r.n_valid), f"{case} n {n_units} unit {u}")


@pytest.mark.parametrize("n_units", [5, 130])
def test_rir16_unfused_44100_three_output_blocks(world, n_units):
    from ss_amd import ops
    sr = 44100
    r, q, s, deq = _renderer(world, "long", sr=sr)
    units = _units("long", n_units, sr=sr, distractor=True)
    plan = r.plan(units)
    lens = r.rirs.lengths
    a, b = _nan(n_units, 2, sr), _nan(n_units, 2, sr)
    ops.fftconv_binaural_rir16_into(r._spec, q, s, lens, plan.desc, a, r.n_valid, flags=plan.flags)
    ops.fftconv_binaural_into(r._spec, deq, lens, plan.desc, b, r.n_valid, flags=plan.flags)
    torch.cuda.synchronize()
    h = _close(a, b, f"44100 unfused n {n_units}")
    assert not h[0].view(np.uint32).any() and np.abs(h[2]).max() > 0
    for u in (2, 3):
        _vs_model(h[u], None, _model_unit(world, "long", units[u], sr), f"44100 unfused n {n_units} unit {u}")
    with pytest.raises(Exception):                                       # the fused entry serves one-block rows only
        ops.audio_obs_rir16_into(r._spec, q, s, lens, plan.desc, a, _nan(n_units, *r.spectrogram_shape), r.n_valid, r.out_len,
                                 flags=plan.flags)


def _cols(units):
    cols = dict(sound=np.asarray([max(u.sound, 0) for u in units], np.int32), t0=np.asarray([u.t0 for u in units], np.int32),
                rir=np.asarray([-1 if u.silent else u.rir for u in units], np.int32))
    if any(u.dis_rir is not None and u.dis_rir >= 0 for u in units):
        cols["dis_sound"] = np.asarray([u.dis_sound for u in units], np.int32)
        cols["dis_rir"] = np.asarray([u.dis_rir for u in units], np.int32)
    return cols


@pytest.mark.parametrize("n_units", [5, 130, 260])
def test_context_on_half_rows_equals_the_fp32_binding_16k(world, n_units):
    """two C contexts - one bound by ss_ctx_set_rir_bank16, one to the dequantised fp32 rows: the fused launch (the unit table up
    to 256 units), waveform alone, spectrogram alone, log-mel through the waveform scratch (the fp32 context takes its one-launch
    log-mel form there: equal to rounding, 1.6e-7 measured, everything else 0.0); a cross-fade is refused"""
    from ss_amd import _lib
    from ss_amd.context import AudioContext
    r, q, s, deq = _renderer(world, "small")
    lens = r.rirs.lengths
    units = _units("small", n_units)
    cols = _cols(units)
    ms, mw, _ = P.mel_filterbank_sparse(SR, 64)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    outs = []
    for half in (True, False):
        ctx = AudioContext(SR)
        for i, src in enumerate(world.srcs[SR]):
            ctx.add_source(f"s{i}", src)
        if half:
            ctx.set_rir_bank16(q, s, lens)
        else:
            ctx.set_rir_bank(deq, lens)
        sg, sg1 = _nan(n_units, *ctx.spectrogram_shape), _nan(n_units, *ctx.spectrogram_shape)
        ag, ag1 = _nan(n_units, 2, SR), _nan(n_units, 2, SR)
        lm = _nan(n_units, 64, 1 + SR // 160, 2)
        ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
        ctx.observe(audiogoal_out=ag1, **cols)
        ctx.observe(spectrogram_out=sg1, **cols)
        ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
        torch.cuda.synchronize()
        if half:
            sg0 = sg.clone()
            with pytest.raises(_lib.SsHipError):                         # a cross-faded step: SS_EINVAL, nothing written
                ctx.observe(cols["sound"], cols["t0"], cols["rir"], spectrogram_out=sg, last_rir=cols["rir"][::-1].copy())
            torch.cuda.synchronize()
            assert torch.equal(sg, sg0)
            again = _nan(n_units, *ctx.spectrogram_shape)                # ... and no keys left behind: the next step is intact
            ctx.observe(spectrogram_out=again, **cols)
            torch.cuda.synchronize()
            assert torch.equal(again, sg1)
        outs.append(dict(sg=sg, ag=ag, ag_only=ag1, sg_only=sg1, logmel=lm))
        ctx.close()
    h = {k: _close(outs[0][k], outs[1][k], f"context 16k n {n_units} {k}") for k in outs[0]}
    for u in (0, 1):                                                     # silent / the empty entry
        assert not h["ag"][u].view(np.uint32).any() and not h["sg"][u].view(np.uint32).any()
        assert np.allclose(h["logmel"][u], np.log(EPS), rtol=1e-6)
    _vs_model(h["ag"][2], h["sg"][2], _model_unit(world, "small", units[2], SR), f"context 16k n {n_units} unit 2")


def test_context_on_half_rows_44100_takes_two_launches(world):
    """rows of three blocks: the half convolution into the caller's buffer - or, without one, the context's hand-over buffer -
    and the spectrogram kernel; against a context on the dequantised fp32 rows given a waveform buffer (the same two launches)"""
    from ss_amd.context import AudioContext
    sr, n = 44100, 5
    r, q, s, deq = _renderer(world, "long", sr=sr)
    lens = r.rirs.lengths
    units = _units("long", n, sr=sr, distractor=True)
    cols = _cols(units)
    outs = []
    for half in (True, False):
        ctx = AudioContext(sr)
        for i, src in enumerate(world.srcs[sr]):
            ctx.add_source(f"s{i}", src)
        if half:
            ctx.set_rir_bank16(q, s, lens)
        else:
            ctx.set_rir_bank(deq, lens)
        sg, sg1, ag = _nan(n, *ctx.spectrogram_shape), _nan(n, *ctx.spectrogram_shape), _nan(n, 2, sr)
        ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
        if half:
            ctx.observe(spectrogram_out=sg1, **cols)                     # no waveform buffer: the hand-over buffer
        torch.cuda.synchronize()
        outs.append(dict(sg=sg, ag=ag, sg_only=sg1 if half else sg))
        ctx.close()
    h = {k: _close(outs[0][k], outs[1][k], f"context 44100 {k}") for k in outs[0]}
    assert np.array_equal(h["sg"], h["sg_only"])
    for u in (2, 3):
        _vs_model(h["ag"][u], h["sg"][u], _model_unit(world, "long", units[u], sr), f"context 44100 unit {u}")


# ---- 3. AudioEngine(rir_rows="half") ---------------------------------------------------------------------------------------------
def _write_rirs(root, sr, spec):
    """spec: {(azimuth, receiver, source): taps} -> {path: wav-layout array}, float32 stereo wav files under root"""
    from scipy.io import wavfile
    files = {}
    for k, ((az, rc, sc), taps) in enumerate(spec.items()):
        d = root / str(az)
        d.mkdir(parents=True, exist_ok=True)
        rng = np.random.default_rng(1000 + k)
        h = (O.synth_rir(rng, sr, length=taps, n=1) if taps <= P.KB else O.synth_rir_blocks(rng, sr, taps, n=1))[0]
        h = np.ascontiguousarray(h.T.astype(np.float32))
        p = str(d / f"{rc}_{sc}.wav")
        wavfile.write(p, sr, h)
        files[p] = h
    return files


def _file_model(clip, wav, t0, sr):
    return R.model_audiogoal(clip, np.ascontiguousarray(wav.T), t0, sr)


def test_engine_16k_two_wav_files_eager_and_vector(world, tmp_path):
    from fakes import FakeSim
    from ss_amd import sim_audio
    from ss_amd.renderer import AudioEngine, RirStore, UnitRequest
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    # (every tensor of this store is at most 1 MiB and a multiple of 512 B: such requests are always cut to size by the caching
    #  allocator, whatever earlier tests left in its cache - a larger one may be handed a cached block up to 1 MiB too big)
    slots, cap = 128, 2000
    before = torch.cuda.memory_allocated(0)
    st = RirStore(slots, cap, DEV, rows="half")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(0) - before == slots * (4 * cap + 8 + 4)       # halves of both ears + two scales + a length
    assert st.bank.data.dtype == torch.float16 and tuple(st.bank.data.shape) == (slots, 2, cap)
    assert st.bank.scales.dtype == torch.float32 and tuple(st.bank.scales.shape) == (slots, 2) and st.bank.spectra is None
    del st

    files = _write_rirs(tmp_path, SR, {(90, 3, 7): 16000, (0, 1, 7): 9000})
    paths = list(files)
    clips = {"one.wav": world.srcs[SR][0], "three.wav": world.srcs[SR][2]}
    slots, cap = 128, SR
    eng = AudioEngine(SR, device=DEV, rir_slots=slots, rir_rows="half")
    assert eng.store.rows_half and eng.store.bank.rows_half and not eng.rir_spectral
    bank = eng.store.bank
    assert bank.data.numel() * 2 + bank.scales.numel() * 4 + bank.lengths.numel() * 4 == slots * (4 * cap + 8 + 4)
    # eager: the files through the store's own reader and the new scatter, then one observation per call
    sl = eng.store.load_files(paths, paths)
    ids = [eng.source_id(nm, c) for nm, c in clips.items()]
    for k, (p, t0, snd) in enumerate(((paths[0], 0, 0), (paths[1], 2 * SR, 1))):
        eng.begin_batch()
        out = eng.observe([UnitRequest(ids[snd], t0, sl[k])], want_audiogoal=True)
        torch.cuda.synchronize()
        _vs_model(out["audiogoal"][0].cpu().numpy(), out["spectrogram"][0].cpu().numpy(),
                  _file_model(list(clips.values())[snd], files[p], t0, SR), f"engine 16k eager {k}")
    q, s = R.quantise(np.stack([np.pad(files[p].T, ((0, 0), (0, cap - len(files[p])))) for p in paths]))
    assert eng.store.bank.data[sl].cpu().numpy().tobytes() == q.tobytes()
    assert eng.store.bank.scales[sl].cpu().numpy().tobytes() == s.tobytes()
    # vector: two in-process envs on the same files - the record path reports its misses, load_files serves them, the call runs again
    eng2 = AudioEngine(SR, device=DEV, rir_slots=8, rir_rows="half")
    sims = [FakeSim(SR, clips, {}, False) for _ in range(2)]
    for sm in sims:
        sm.binaural_rir_dir = str(tmp_path)
    sims[1]._receiver_position_index, sims[1]._rotation_angle, sims[1]._current_sound = 1, 0, "three.wav"
    obs = sim_audio.VectorAudioObserver(eng2, [sim_audio.attach(sm, eng2) for sm in sims], want_audiogoal=True)
    for step in range(3):
        idx = [sm._audio_index for sm in sims]
        out = obs.observe()
        torch.cuda.synchronize()
        ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
        _vs_model(ag[0], sg[0], _file_model(clips["one.wav"], files[paths[0]], 0, SR), f"engine 16k vector step {step} env 0")
        _vs_model(ag[1], sg[1], _file_model(clips["three.wav"], files[paths[1]], idx[1] * SR, SR), f"engine 16k vector step {step} env 1")
    assert eng2.store.misses == 2 and eng2.store.rows_half


def test_engine_44100_one_vector_step_of_5_envs(world, tmp_path):
    from fakes import FakeSim
    from ss_amd import sim_audio
    from ss_amd.renderer import AudioEngine
    sr = 44100
    spec = {(0, rc, 7): taps for rc, taps in enumerate((44100, 20000, 9000, 30001, 44100))}
    files = _write_rirs(tmp_path, sr, spec)
    clips = {"one.wav": world.srcs[sr][0], "three.wav": world.srcs[sr][2]}
    eng = AudioEngine(sr, device=DEV, rir_slots=8, rir_rows="half")
    sims = [FakeSim(sr, clips, {}, False) for _ in range(5)]
    for rc, sm in enumerate(sims):
        sm.binaural_rir_dir, sm._receiver_position_index, sm._rotation_angle = str(tmp_path), rc, 0
        sm._current_sound = "three.wav" if rc % 2 else "one.wav"
        sm._audio_index = 2 if rc % 2 else 0
    obs = sim_audio.VectorAudioObserver(eng, [sim_audio.attach(sm, eng) for sm in sims], want_audiogoal=True)
    out = obs.observe()
    torch.cuda.synchronize()
    ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
    assert tuple(sg.shape[1:]) == (65, 69, 2) and eng.store.bank.data.dtype == torch.float16
    for rc, sm in enumerate(sims):
        wav = files[str(tmp_path / "0" / f"{rc}_7.wav")]
        clip = clips[sm._current_sound]
        _vs_model(ag[rc], sg[rc], _file_model(clip, wav, 2 * sr if rc % 2 else 0, sr), f"engine 44100 env {rc}")
