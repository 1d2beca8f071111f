"""Half-precision time-domain RIR rows under the fused 44.1 / 48 kHz row kernels on the GPU (include/ss_hip.h "Half-precision
time-domain rows"): k_obs_blocks / k_obs_rows <.., ROWS16>, ss_audio_obs_rows_rir16_f32, ss_ctx_set_rir_bank16_rows,
AudioEngine(rir_rows="half", rir_rows16_fused=True).  The banks and helpers of tests/test_gpu_time_rir16.py.

  * stateless: ops.audio_obs_rows_rir16_into against ops.audio_obs_into on float(q) * scale, identical parameters, <= 2e-6 of peak
    (each fp32 path is held to <= 1e-6 of peak against float64 by the project's parity record, the inputs are identical; the host
    build measures 0.0) - 1 and 5 units (k_obs_blocks with parts), 43 (the first size past its budget of one workgroup per CU),
    150 (k_obs_rows' persistent loop: more rows than CUs), at 44.1 kHz, 48 kHz and 20 kHz (two blocks), distractor terms of another
    entry, with and without a waveform buffer; silent units bit-exact +0; two live units against the quantised float64 model,
    <= 1e-4 of peak (the project's budget);
  * context: ss_ctx_set_rir_bank16_rows against ss_ctx_set_rir_bank16 at 44.1 kHz, 5 units - waveform + spectrogram, spectrogram
    alone (no hand-over buffer on the new binding: tests/test_rir16_rows_host.py pins the routes, values are compared here),
    log-mel + spectrogram, n_valid = 11 025 with and without a waveform buffer; a cross-fade is refused and leaves outputs and
    keys untouched;
  * engine: AudioEngine(44100, rir_rows="half", rir_rows16_fused=True) over wav files - one vector step of 5 envs and one eager
    call, against the same engine without the keyword (the A/B bound) and against the file model (1e-4).

(The file's name sorts it behind tests/test_gpu_spec*.py: see tests/test_gpu_time_rir16.py.)"""
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

from test_rir16_host import make_banks
from test_gpu_time_rir16 import (AB, DEV, EPS, _close, _cols, _file_model, _model_unit, _nan, _renderer, _units, _vs_model,
                                 _write_rirs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    """the two banks (numpy, read-only) and per sampling rate two 1-s clips and one 3-s clip; computed once"""
    srcs = {}
    for sr in (20000, 44100, 48000):
        rng = np.random.default_rng(sr)
        srcs[sr] = list(O.synth_sources(rng, sr, k=2, seconds=1)) + [O.synth_sources(rng, sr, k=1, seconds=3)[0]]
    return types.SimpleNamespace(banks=make_banks(), srcs=srcs, models={})


def _model(w, name, u, sr, n_valid=None):
    """the quantised float64 model of one unit, computed once per (bank, rate, unit) and shared"""
    key = (name, sr, n_valid, u.sound, u.t0, u.rir, u.dis_sound, u.dis_rir)
    if key not in w.models:
        w.models[key] = _model_unit(w, name, u, sr, n_valid)
        w.models[key].setflags(write=False)
    return w.models[key]


# ---- 1. stateless -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n_units", [(44100, 1), (44100, 5), (44100, 43), (44100, 150), (48000, 5), (48000, 150), (20000, 5)])
def test_rows_rir16_entry_equals_fp32_entry_fed_dequantised_rows(world, sr, n_units):
    from ss_amd import ops
    name = "small" if sr == 20000 else "long"                            # (20 kHz: two output blocks over one RIR block)
    r, q, s, deq = _renderer(world, name, sr=sr)
    units = _units(name, max(n_units, 4), sr=sr, distractor=True)
    if n_units == 1:
        units = units[3:4]                                               # one live unit, with its distractor term
    plan = r.plan(units)
    lens = r.rirs.lengths
    assert not (plan.flags & ops.FLAG_NO_DISTRACTOR) and len(units) == n_units
    res = {}
    for form in ("half", "fp32"):
        ag, sg, sg_only = _nan(n_units, 2, sr), _nan(n_units, *r.spectrogram_shape), _nan(n_units, *r.spectrogram_shape)
        if form == "half":
            ops.audio_obs_rows_rir16_into(r._spec, q, s, lens, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
            ops.audio_obs_rows_rir16_into(r._spec, q, s, lens, plan.desc, None, sg_only, r.n_valid, r.out_len, flags=plan.flags)
        else:
            ops.audio_obs_into(r._spec, deq, lens, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
            ops.audio_obs_into(r._spec, deq, lens, plan.desc, None, sg_only, r.n_valid, r.out_len, flags=plan.flags)
        res[form] = dict(ag=ag, sg=sg, sg_only=sg_only)
    torch.cuda.synchronize()
    h = {k: _close(res["half"][k], res["fp32"][k], f"rows {sr} n {n_units} {k}") for k in res["half"]}
    assert np.array_equal(h["sg"], h["sg_only"])                         # the same launch with and without the waveform written
    live = [0] if n_units == 1 else [2, 3]
    if n_units > 1:                                                      # the silent unit: bit-exact +0
        for k in h:
            assert not h[k][0].view(np.uint32).any(), k
    for u in live:
        assert np.abs(h["ag"][u]).max() > 0
        _vs_model(h["ag"][u], h["sg"][u], _model(world, name, units[u], sr), f"rows {sr} n {n_units} unit {u}")


def test_rows_rir16_entry_without_distractor_terms_and_one_rendered_block(world):
    """SS_FLAG_NO_DISTRACTOR (half the stash) at 5 and 43 units; and n_valid = 11 025 of 44 100: one launch without a waveform
    buffer, the half convolution + k_spectrogram with one - both against the fp32 entry on the dequantised rows"""
    from ss_amd import ops
    sr = 44100
    r, q, s, deq = _renderer(world, "long", sr=sr)
    lens = r.rirs.lengths
    for n in (5, 43):
        units = _units("long", n, sr=sr)
        plan = r.plan(units)
        assert plan.flags & ops.FLAG_NO_DISTRACTOR
        a, b = dict(ag=_nan(n, 2, sr), sg=_nan(n, *r.spectrogram_shape)), dict(ag=_nan(n, 2, sr), sg=_nan(n, *r.spectrogram_shape))
        ops.audio_obs_rows_rir16_into(r._spec, q, s, lens, plan.desc, a["ag"], a["sg"], sr, sr, flags=plan.flags)
        ops.audio_obs_into(r._spec, deq, lens, plan.desc, b["ag"], b["sg"], sr, sr, flags=plan.flags)
        torch.cuda.synchronize()
        h = {k: _close(a[k], b[k], f"rows no-distractor n {n} {k}") for k in a}
        assert not h["ag"][0].view(np.uint32).any() and not h["sg"][0].view(np.uint32).any()
        _vs_model(h["ag"][2], h["sg"][2], _model(world, "long", units[2], sr), f"rows no-distractor n {n} unit 2")
    nv, n = 11025, 5
    r2, q2, s2, deq2 = _renderer(world, "long", sr=sr, step_time=0.25)
    assert r2.n_valid == nv
    units = _units("long", n, sr=sr, distractor=True)
    plan = r2.plan(units)
    lens = r2.rirs.lengths
    a = dict(ag=_nan(n, 2, sr), sg=_nan(n, *r2.spectrogram_shape), sg_only=_nan(n, *r2.spectrogram_shape))
    b = dict(ag=_nan(n, 2, sr), sg=_nan(n, *r2.spectrogram_shape), sg_only=_nan(n, *r2.spectrogram_shape))
    ops.audio_obs_rows_rir16_into(r2._spec, q2, s2, lens, plan.desc, a["ag"], a["sg"], nv, sr, flags=plan.flags)
    ops.audio_obs_rows_rir16_into(r2._spec, q2, s2, lens, plan.desc, None, a["sg_only"], nv, sr, flags=plan.flags)
    ops.audio_obs_into(r2._spec, deq2, lens, plan.desc, b["ag"], b["sg"], nv, sr, flags=plan.flags)
    ops.audio_obs_into(r2._spec, deq2, lens, plan.desc, None, b["sg_only"], nv, sr, flags=plan.flags)
    torch.cuda.synchronize()
    h = {k: _close(a[k], b[k], f"rows n_valid {nv} {k}") for k in a}
    assert not h["ag"][:, :, nv:].any() and np.abs(h["ag"][2][:, :nv]).max() > 0
    _vs_model(h["ag"][2], h["sg"][2], _model(world, "long", units[2], sr, nv), f"rows n_valid {nv} unit 2")
    err = np.abs(h["sg"].astype(np.float64) - h["sg_only"]).max() / np.abs(h["sg"]).max()      # (two launches against one)
    print(f"[gpu_rir16_rows] n_valid {nv}: spectrogram of the two-launch route vs the one-launch route: {err:.3e}")
    assert err <= AB


def test_rows_rir16_entry_refusals_on_the_device(world):
    from ss_amd import _lib, ops
    r, q, s, deq = _renderer(world, "small", sr=20000)
    plan = r.plan(_units("small", 3, sr=20000))
    sg = _nan(3, *r.spectrogram_shape)
    with pytest.raises(_lib.SsHipError):                                 # a cross-fade
        ops.audio_obs_rows_rir16_into(r._spec, q, s, r.rirs.lengths, plan.desc, None, sg, 20000, 20000, flags=ops.FLAG_CROSSFADE)
    torch.cuda.synchronize()
    assert bool(torch.isnan(sg).all())


# ---- 2. the context binding -------------------------------------------------------------------------------------------------
def _contexts(world, sr, q, s, lens, n_valid=None):
    from ss_amd.context import AudioContext
    out = []
    for rows in (True, False):
        ctx = AudioContext(sr, n_valid=n_valid)
        for i, src in enumerate(world.srcs[sr]):
            ctx.add_source(f"s{i}", src)
        ctx.set_rir_bank16(q, s, lens, rows=rows)
        out.append(ctx)
    return out


def test_context_bound_for_the_row_kernels_equals_the_plain_binding_44100(world):
    from ss_amd import _lib
    sr, n = 44100, 5
    r, q, s, deq = _renderer(world, "long", sr=sr)
    lens = r.rirs.lengths
    units = _units("long", n, sr=sr, distractor=True)
    cols = _cols(units)
    ms, mw, _ = P.mel_filterbank_sparse(sr, 64)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    outs = []
    for rows, ctx in zip((True, False), _contexts(world, sr, q, s, lens)):
        shp = ctx.spectrogram_shape
        sg, sg1, sg2, ag = _nan(n, *shp), _nan(n, *shp), _nan(n, *shp), _nan(n, 2, sr)
        lm, lm1 = _nan(n, 64, 1 + sr // 160, 2), _nan(n, 64, 1 + sr // 160, 2)
        ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
        ctx.observe(spectrogram_out=sg1, **cols)                         # (rows=False: the hand-over buffer; rows=True: none)
        ctx.observe(spectrogram_out=sg2, logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
        ctx.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
        torch.cuda.synchronize()
        if rows:
            sg0 = sg.clone()
            with pytest.raises(_lib.SsHipError):                         # a cross-faded step: SS_EINVAL, nothing written
                ctx.observe(cols["sound"], cols["t0"], cols["rir"], spectrogram_out=sg, last_rir=cols["rir"][::-1].copy())
            torch.cuda.synchronize()
            assert torch.equal(sg, sg0)
            again = _nan(n, *shp)                                        # ... and no keys left behind: the next step is intact
            ctx.observe(spectrogram_out=again, **cols)
            torch.cuda.synchronize()
            assert torch.equal(again, sg1)
        outs.append(dict(sg=sg, ag=ag, sg_only=sg1, sg_mel=sg2, logmel=lm, logmel_only=lm1))
        ctx.close()
    h = {k: _close(outs[0][k], outs[1][k], f"context 44100 rows=True vs rows=False {k}") for k in outs[0]}
    assert np.array_equal(h["sg"], h["sg_only"]) and np.array_equal(h["sg"], h["sg_mel"])
    assert not h["ag"][0].view(np.uint32).any() and not h["sg"][0].view(np.uint32).any()
    assert np.allclose(h["logmel"][0], np.log(EPS), rtol=1e-6)
    for u in (2, 3):
        _vs_model(h["ag"][u], h["sg"][u], _model(world, "long", units[u], sr), f"context 44100 rows=True unit {u}")


def test_context_bound_for_the_row_kernels_one_rendered_block(world):
    """n_valid = 11 025 of 44 100: with a waveform buffer both bindings take two launches, without one the new binding takes
    k_obs_rows and the plain one its hand-over buffer"""
    sr, n, nv = 44100, 5, 11025
    r, q, s, deq = _renderer(world, "long", sr=sr, step_time=0.25)
    lens = r.rirs.lengths
    units = _units("long", n, sr=sr, distractor=True)
    cols = _cols(units)
    outs = []
    for ctx in _contexts(world, sr, q, s, lens, n_valid=nv):
        sg, sg1, ag = _nan(n, *ctx.spectrogram_shape), _nan(n, *ctx.spectrogram_shape), _nan(n, 2, sr)
        ctx.observe(spectrogram_out=sg, audiogoal_out=ag, **cols)
        ctx.observe(spectrogram_out=sg1, **cols)
        torch.cuda.synchronize()
        outs.append(dict(sg=sg, ag=ag, sg_only=sg1))
        ctx.close()
    h = {k: _close(outs[0][k], outs[1][k], f"context 44100 n_valid {nv} {k}") for k in outs[0]}
    assert not h["ag"][:, :, nv:].any()
    _vs_model(h["ag"][2], h["sg_only"][2], _model(world, "long", units[2], sr, nv), f"context 44100 n_valid {nv} unit 2")


# ---- 3. AudioEngine(rir_rows="half", rir_rows16_fused=True) -----------------------------------------------------------------
def test_engine_44100_fused_rows_vector_step_and_eager_call(world, tmp_path):
    from fakes import FakeSim
    from ss_amd import sim_audio
    from ss_amd.renderer import AudioEngine, UnitRequest
    sr = 44100
    spec = {(0, rc, 7): taps for rc, taps in enumerate((44100, 20000, 9000, 30001, 44100))}
    files = _write_rirs(tmp_path, sr, spec)
    paths = list(files)
    clips = {"one.wav": world.srcs[sr][0], "three.wav": world.srcs[sr][2]}
    got = []
    for fused in (True, False):
        eng = AudioEngine(sr, device=DEV, rir_slots=8, rir_rows="half", **(dict(rir_rows16_fused=True) if fused else {}))
        assert eng.rir_rows16_fused == fused and eng.renderer.rows16_fused == fused and eng.store.bank.rows_half
        sims = [FakeSim(sr, clips, {}, False) for _ in range(5)]
        for rc, sm in enumerate(sims):
            sm.binaural_rir_dir, sm._receiver_position_index, sm._rotation_angle = str(tmp_path), rc, 0
            sm._current_sound = "three.wav" if rc % 2 else "one.wav"
            sm._audio_index = 2 if rc % 2 else 0
        obs = sim_audio.VectorAudioObserver(eng, [sim_audio.attach(sm, eng) for sm in sims], want_audiogoal=True)
        out = obs.observe()                                              # one vector step of 5 envs (the context's binding)
        torch.cuda.synchronize()
        vec = dict(ag=out["audiogoal"].clone(), sg=out["spectrogram"].clone())
        assert tuple(vec["sg"].shape[1:]) == (65, 69, 2) and eng.store.bank.data.dtype == torch.float16
        # one eager call on a second engine of the same kind (the renderer's path: ops.audio_obs_rows_rir16_into)
        eng2 = AudioEngine(sr, device=DEV, rir_slots=8, rir_rows="half", **(dict(rir_rows16_fused=True) if fused else {}))
        sl = eng2.store.load_files(paths[:2], paths[:2])
        ids = [eng2.source_id(nm, c) for nm, c in clips.items()]
        eng2.begin_batch()
        e1 = eng2.observe([UnitRequest(ids[0], 0, sl[0]), UnitRequest(ids[1], 2 * sr, sl[1])], want_audiogoal=True)
        torch.cuda.synchronize()
        e1 = {k: v.clone() for k, v in e1.items() if k in ("audiogoal", "spectrogram")}
        eng2.begin_batch()
        e2 = eng2.observe([UnitRequest(ids[0], 0, sl[0]), UnitRequest(ids[1], 2 * sr, sl[1])])      # spectrogram only
        torch.cuda.synchronize()
        got.append(dict(vec_ag=vec["ag"], vec_sg=vec["sg"], eager_ag=e1["audiogoal"].clone(), eager_sg=e1["spectrogram"].clone(),
                        eager_sg_only=e2["spectrogram"].clone()))
    h = {k: _close(got[0][k], got[1][k], f"engine 44100 fused vs two launches {k}") for k in got[0]}
    assert np.array_equal(h["eager_sg"], h["eager_sg_only"])
    for rc in range(5):
        wav = files[str(tmp_path / "0" / f"{rc}_7.wav")]
        clip = clips["three.wav" if rc % 2 else "one.wav"]
        _vs_model(h["vec_ag"][rc], h["vec_sg"][rc], _file_model(clip, wav, 2 * sr if rc % 2 else 0, sr), f"engine 44100 fused env {rc}")
    for k, (snd, t0) in enumerate((("one.wav", 0), ("three.wav", 2 * sr))):
        _vs_model(h["eager_ag"][k], h["eager_sg"][k], _file_model(clips[snd], files[paths[k]], t0, sr), f"engine 44100 fused eager {k}")
