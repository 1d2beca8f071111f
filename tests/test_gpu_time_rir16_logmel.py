"""One-launch log-mel from half-precision time-domain RIR rows on the GPU (include/ss_hip.h: ss_audio_obs_logmel_rir16_f32,
ss_audio_obs_logmel_rows_rir16_f32, ss_audio_obs_logmel_rir16_buckets_f32, ss_ctx_set_logmel_rir16_policy).

  * stateless: each new entry against two launches on the same half bank - the existing rir16 observation entry with a waveform,
    then ss_audio_features_f32: the waveform bit-equal, the pooled spectrogram within 1e-4, the log-mel within the log-mel rule
    (1e-4 of the unit's largest value); all three outputs and log-mel alone.  And A/B against the fp32 log-mel entry on
    float(q) * scale: waveform and pooled spectrogram <= 2e-6 of peak, log-mel under the rule (the host build measures 0.0).
    16 kHz: the five kinds of unit of tests/test_rir16_host.py (loop-free) and the distractor case (loop); buckets: the 12-unit
    scene of tests/spec_buckets_ref.py and the first-bucket identity; 44.1 kHz: 5 units (k_obs_blocks) and 44 units (264
    workgroups > 256 CUs: k_obs_rows); 48 kHz: 5 units.
  * context, the three bindings: under set_logmel_rir16_policy(1, 2**31 - 1) the log-mel within the rule of the quantised float64
    model and no waveform scratch; under the default bit-equal to observe + audio_features_into, with scratch; a step outside the
    range takes the scratch route; a cross-faded step is SS_EINVAL and leaves no keys; two overlap lanes.
  * engine: AudioEngine(rir_rows="half") at 16 kHz, with rir_buckets, and at 44.1 kHz with rir_rows16_fused: one step of 5 envs,
    policy on against policy off; rebinding the bank keeps the policy.

No launch is captured into a graph, and no test forces k_obs_blocks outside its plan.  (The file's name sorts it behind
tests/test_gpu_spec*.py, and it allocates from a memory pool of its own: see tests/test_gpu_rir16_buckets.py.)"""
import gc
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
import spec_buckets_ref as B
from test_logmel import TOL as MEL_TOL
from test_rir16_host import SIMPLE_UNITS, make_banks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, SR44, SR48 = 16000, 44100, 48000
AB = 2e-6
BUDGET = 1e-4
EPS = 1e-6
ALWAYS = (1, 2 ** 31 - 1)
ENGINE_BUCKETS = [(3, 16000), (4, 40000)]


@pytest.fixture(scope="module", autouse=True)
def _private_pool():
    """Every torch allocation of this module comes from a memory pool of the module's own and goes back to the driver with it:
    later modules of the suite hold torch.cuda.memory_allocated deltas of a store to the byte."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        gc.collect()
        torch.cuda.synchronize()
    del pool


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


_MEL = {}


def _mel(sr, n_mels=64):
    if (sr, n_mels) not in _MEL:
        ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
        _MEL[(sr, n_mels)] = (torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV),
                              torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV))
    return _MEL[(sr, n_mels)]


@pytest.fixture(scope="module")
def world(_private_pool):
    """the two banks of tests/test_rir16_host.py (numpy, read-only) and per sampling rate two 1-s clips and one 3-s clip"""
    srcs = {}
    for sr in (SR, SR44, SR48):
        rng = np.random.default_rng(sr)
        srcs[sr] = list(O.synth_sources(rng, sr, k=2, seconds=1)) + [O.synth_sources(rng, sr, k=1, seconds=3)[0]]
    w = types.SimpleNamespace(banks=make_banks(), srcs=srcs)
    yield w
    w.__dict__.clear()
    _MEL.clear()
    gc.collect()


def _requests(units):
    from ss_amd.renderer import UnitRequest
    return [UnitRequest(silent=True) if u.get("rir", -1) < 0 else
            UnitRequest(u["sound"], u["t0"], u["rir"], dis_sound=u.get("dis_sound", -1), dis_rir=u.get("dis_rir", -1)) for u in units]


def _cycle(name, n, sr):
    """unit 0 silent, then live units over every entry of the bank and all three sounds (the 3-s clip in its last second); every
    third live unit carries a term of ANOTHER entry"""
    entries = 4 if name == "small" else 2
    units = [dict(rir=-1)]
    for k in range(1, n):
        u = dict(sound=k % 3, t0=2 * sr if k % 3 == 2 else 0, rir=k % entries)
        if k % 3 == 0:
            u.update(dis_sound=(k + 1) % 2, dis_rir=(k + 1) % entries)
        units.append(u)
    return units


def _renderer(w, name, sr):
    """a planner over the fp32 rows of bank `name`, its half form from the device (ss_rir_rows16_f32) and float(q) * scale"""
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    b = w.banks[name]
    r = BatchedAudioRenderer(sr, device=DEV)
    for i, s in enumerate(w.srcs[sr]):
        r.add_source(f"s{i}", s)
    rows = torch.from_numpy(b["rows"].copy()).to(DEV)
    r.set_rir_bank(RirBank(rows, torch.from_numpy(b["lens"].copy()).to(DEV)))
    q, s = ops.rir_rows16(rows)
    return r, q, s, (q.float() * s[..., None]).contiguous()


def _model_wave(w, name, u, sr):
    """float64 waveform of the quantised model of one unit (both terms); None: a silent unit or the empty entry alone"""
    b = w.banks[name]
    if u.get("rir", -1) < 0:
        return None
    out, live = np.zeros((2, sr)), False
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        ln = int(b["lens"][g])
        live = live or ln > 0
        out += R.model_audiogoal(w.srcs[sr][snd], b["rows"][g][:, :ln], t0, sr, True)
    return out if live else None


def _rule(got, ref, label):
    """the log-mel rule, per unit: 1e-4 of the unit's largest value"""
    got, ref = got.cpu().numpy(), ref.cpu().numpy() if torch.is_tensor(ref) else ref
    assert not np.isnan(got).any(), label
    worst = 0.0
    for k in range(len(got)):
        err = np.abs(got[k].astype(np.float64) - ref[k]).max() / np.abs(ref[k]).max()
        worst = max(worst, err)
        assert err <= MEL_TOL, (label, k, err)
    print(f"[gpu_rir16_logmel] {label}: worst log-mel error / unit's largest value = {worst:.3e}")


def _peak(got, ref, bound, label):
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    assert not np.isnan(got).any(), label
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max()
    print(f"[gpu_rir16_logmel] {label}: max error / peak = {err:.3e}")
    assert err <= bound, (label, err)


def _compare(n, sr, two, one, fp32, quiet, label, n_mels=64):
    """two(ag, sg): today's observation with a waveform; one(ag, sg, lm): the new entry; fp32(ag, sg, lm): its fp32 sibling on the
    dequantised rows"""
    from ss_amd import ops
    msd, mwd = _mel(sr, n_mels)
    T, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    ag0, sg0, lm0 = _nan(n, 2, sr), _nan(n, 65, t4, 2), _nan(n, n_mels, T, 2)
    two(ag0, sg0)
    ops.audio_features_into(ag0, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    ag1, sg1, lm1 = _nan(n, 2, sr), _nan(n, 65, t4, 2), _nan(n, n_mels, T, 2)             # all three outputs: one launch
    one(ag1, sg1, lm1)
    lm2 = _nan(n, n_mels, T, 2)                                                            # log-mel alone: no buffer at all
    one(None, None, lm2)
    ag3, sg3, lm3 = _nan(n, 2, sr), _nan(n, 65, t4, 2), _nan(n, n_mels, T, 2)
    fp32(ag3, sg3, lm3)
    torch.cuda.synchronize()
    for t in (ag0, sg0, lm0, ag1, sg1, lm1, lm2, ag3, sg3, lm3):
        assert not torch.isnan(t).any(), label
    assert torch.equal(ag1, ag0), label                                  # (same convolution code, same order: same bits)
    _peak(sg1, sg0, BUDGET, f"{label}: pooled spectrogram, one launch vs two")
    _rule(lm1, lm0, f"{label}: log-mel (all three outputs), one launch vs two")
    _rule(lm2, lm0, f"{label}: log-mel alone, one launch vs two")
    _peak(ag1, ag3, AB, f"{label}: waveform, half vs fp32(dequantised)")
    _peak(sg1, sg3, AB, f"{label}: pooled spectrogram, half vs fp32(dequantised)")
    _rule(lm1, lm3, f"{label}: log-mel, half vs fp32(dequantised)")
    for k in quiet:                                                      # silent units and the empty entry
        assert torch.allclose(lm2[k], torch.full_like(lm2[k], float(np.log(EPS))), rtol=1e-6, atol=0), (label, k)
        assert torch.allclose(lm1[k], torch.full_like(lm1[k], float(np.log(EPS))), rtol=1e-6, atol=0), (label, k)
        assert not sg1[k].any() and not ag1[k].any(), (label, k)
    return lm1, sg1


def _vs_model(w, name, units, sr, lm, sg, label, only=None):
    lm = lm.cpu().numpy()
    sg = None if sg is None else sg.cpu().numpy()
    for k, u in enumerate(units):
        if only is not None and k not in only:
            continue
        wave = _model_wave(w, name, u, sr)
        if wave is None:
            assert np.allclose(lm[k], np.log(EPS), rtol=1e-6, atol=0), (label, k)
            continue
        ref = O.compute_logmel(wave, sr, lm.shape[1], EPS)
        err = np.abs(lm[k] - ref).max() / np.abs(ref).max()
        print(f"[gpu_rir16_logmel] {label} unit {k}: log-mel vs quantised float64 model = {err:.3e}")
        assert err <= MEL_TOL, (label, k, err)
        if sg is not None:
            e = O.relerr(sg[k], O.compute_spectrogram(wave))
            assert e <= BUDGET, (label, k, e)


# ---- 1. stateless ------------------------------------------------------------------------------------------------------------
def _single_case(w, name, sr, units, label, quiet, model_units):
    from ss_amd import ops
    r, q, s, deq = _renderer(w, name, sr)
    plan = r.plan(_requests(units))
    lens = r.rirs.lengths
    long_rows = sr > P.KB
    two_f = ops.audio_obs_rows_rir16_into if long_rows else ops.audio_obs_rir16_into
    one_f = ops.audio_obs_logmel_rows_rir16_into if long_rows else ops.audio_obs_logmel_rir16_into
    fp32_f = ops.audio_obs_logmel_rows_into if long_rows else ops.audio_obs_logmel_into
    msd, mwd = _mel(sr)
    lm1, sg1 = _compare(
        len(units), sr,
        lambda ag, sg: two_f(r._spec, q, s, lens, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags),
        lambda ag, sg, lm: one_f(r._spec, q, s, lens, plan.desc, ag, sg, lm, msd, mwd, r.n_valid, r.out_len, EPS, "reflect", flags=plan.flags),
        lambda ag, sg, lm: fp32_f(r._spec, deq, lens, plan.desc, ag, sg, lm, msd, mwd, r.n_valid, r.out_len, EPS, "reflect", flags=plan.flags),
        quiet, label)
    _vs_model(w, name, units, sr, lm1, sg1, label, only=model_units)
    return plan


def test_stateless_16k_loop_free(world):
    from ss_amd import ops
    plan = _single_case(world, "small", SR, SIMPLE_UNITS, "16 kHz, 5 units, loop-free", quiet=[1, 2], model_units=[0, 3, 4])
    assert plan.flags & ops.FLAG_NO_DISTRACTOR


def test_stateless_16k_loop_with_a_distractor(world):
    from ss_amd import ops
    units = [dict(sound=0, t0=0, rir=3, dis_sound=1, dis_rir=2), dict(rir=-1), dict(sound=1, t0=0, rir=0)]
    plan = _single_case(world, "small", SR, units, "16 kHz, 3 units, loop + distractor", quiet=[1], model_units=[0, 2])
    assert not (plan.flags & ops.FLAG_NO_DISTRACTOR)


@pytest.mark.parametrize("sr,n_units", [(SR44, 5), (SR44, 44), (SR48, 5)],
                         ids=["44100-5-units-blocks-kernel", "44100-44-units-rows-kernel", "48000-5-units"])
def test_stateless_rows_of_three_blocks(world, sr, n_units):
    units = _cycle("long", n_units, sr)
    _single_case(world, "long", sr, units, f"{sr} Hz, {n_units} units", quiet=[0], model_units=[1, 3])


@pytest.fixture(scope="module")
def scene(_private_pool):
    """the 12-unit, four-bucket scene: the half bucketed bank, the fp32 one of float(q) * scale, a planner"""
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank
    sc = B.scene()
    lengths = torch.from_numpy(np.ascontiguousarray(sc["lens"], np.int32)).to(DEV)
    rows = [torch.from_numpy(np.ascontiguousarray(r)).to(DEV) for r in sc["rows"]]
    qs = [ops.rir_rows16(r) for r in rows]
    deq = [(q.float() * s[..., None]).contiguous() for q, s in qs]
    views = [lengths[f:f + n] for f, n in zip(B.FIRST, B.COUNTS)]
    half = BucketedRirBank([RirBank(q, v, scales=s) for (q, s), v in zip(qs, views)], lengths, list(B.FIRST))
    fp32 = BucketedRirBank([RirBank(d, v) for d, v in zip(deq, views)], lengths, list(B.FIRST))
    r = BatchedAudioRenderer(B.SR, device=DEV)
    for i, src in enumerate(sc["srcs"]):
        r.add_source(f"s{i}", src)
    r.set_rir_bank(half)
    torch.cuda.synchronize()
    w = types.SimpleNamespace(sc=sc, half=half, fp32=fp32, deq=[d.cpu().numpy() for d in deq], lengths=lengths, r=r)
    yield w
    w.__dict__.clear()
    gc.collect()


def _scene_model(w, u):
    if u.get("rir", -1) < 0 or u["rir"] == B.EMPTY:
        return None
    out = np.zeros((2, SR))
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        b = B.bucket_of(g)
        out += R.model_audiogoal(w.sc["srcs"][snd], w.deq[b][g - B.FIRST[b]][:, :int(w.sc["lens"][g])], t0, SR, quant=False)
    return out


def _scene_vs_model(w, units, lm, sg, label):
    lm = lm.cpu().numpy()
    sg = None if sg is None else sg.cpu().numpy()
    assert not np.isnan(lm).any(), label
    for k, u in enumerate(units):
        wave = _scene_model(w, u)
        if wave is None:
            assert np.allclose(lm[k], np.log(EPS), rtol=1e-6, atol=0) and (sg is None or not sg[k].any()), (label, k)
            continue
        ref = O.compute_logmel(wave, SR, 64, EPS)
        err = np.abs(lm[k] - ref).max() / np.abs(ref).max()
        print(f"[gpu_rir16_logmel] {label} unit {k}: log-mel vs float64 model fed the bank's halves = {err:.3e}")
        assert err <= MEL_TOL, (label, k, err)
        if sg is not None:
            assert O.relerr(sg[k], O.compute_spectrogram(wave)) <= BUDGET, (label, k)


def test_stateless_buckets_twelve_unit_scene(scene):
    from ss_amd import ops
    w, r = scene, scene.r
    units = w.sc["units"]
    plan = r.plan(_requests(units))
    assert not (plan.flags & 7)                                          # distractor terms, no cross-fade, not bucket 0 alone
    arr, arr32 = w.half.rir16_c_array(), w.fp32.c_array(False)
    msd, mwd = _mel(SR)
    quiet = [k for k, u in enumerate(units) if u.get("rir", -1) < 0 or u["rir"] == B.EMPTY]
    lm1, sg1 = _compare(
        len(units), SR,
        lambda ag, sg: ops.audio_obs_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags),
        lambda ag, sg, lm: ops.audio_obs_logmel_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, ag, sg, lm, msd, mwd, r.n_valid,
                                                                   r.out_len, EPS, "reflect", flags=plan.flags),
        lambda ag, sg, lm: ops.audio_obs_logmel_buckets_into(r._spec, arr32, 4, w.lengths, plan.desc, ag, sg, lm, msd, mwd, r.n_valid,
                                                             r.out_len, EPS, "reflect", flags=plan.flags),
        quiet, "16 kHz buckets, 12 units")
    _scene_vs_model(w, units, lm1, sg1, "16 kHz buckets, 12 units")


def test_first_bucket_launch_bit_equals_the_single_allocation_entry_on_bucket_0(scene):
    from ss_amd import _lib, ops
    from ss_amd.renderer import UnitRequest
    w, r = scene, scene.r
    units = [UnitRequest(0, 0, 0), UnitRequest(1, 0, 2), UnitRequest(0, 0, B.EMPTY), UnitRequest(silent=True), UnitRequest(1, 4000, 0)]
    plan = r.plan(units)
    assert plan.flags & ops.FLAG_NO_DISTRACTOR
    b0, arr = w.half.banks[0], w.half.rir16_c_array()
    msd, mwd = _mel(SR)
    n, T, t4 = len(units), 1 + SR // 160, P.spectrogram_shape(SR)[1]
    for flags in (plan.flags | ops.FLAG_FIRST_BUCKET, ops.FLAG_FIRST_BUCKET):           # loop-free, and the loop kernel on bucket 0
        got = [_nan(n, 2, SR), _nan(n, 65, t4, 2), _nan(n, 64, T, 2)]
        ops.audio_obs_logmel_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, *got, msd, mwd, r.n_valid, r.out_len, EPS,
                                                "reflect", flags=flags)
        want = [_nan(n, 2, SR), _nan(n, 65, t4, 2), _nan(n, 64, T, 2)]
        ops.audio_obs_logmel_rir16_into(r._spec, b0.data, b0.scales, w.lengths, plan.desc, *want, msd, mwd, r.n_valid, r.out_len, EPS,
                                        "reflect", flags=flags & ~ops.FLAG_FIRST_BUCKET)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert not torch.isnan(a).any() and torch.equal(a, b), flags
        assert got[0][0].any() and not got[0][2].any() and not got[0][3].any()
    with pytest.raises(_lib.SsHipError):                                 # rows longer than kB: never on the buckets entry
        ops.audio_obs_logmel_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, None, None, _nan(n, 64, 1 + SR44 // 160, 2),
                                                *_mel(SR44), SR44, SR44, EPS, "reflect", flags=plan.flags)


# ---- 2. the context: ss_ctx_set_logmel_rir16_policy --------------------------------------------------------------------------
def _cols(units):
    cols = dict(sound=np.asarray([u.get("sound", 0) for u in units], np.int32), t0=np.asarray([u.get("t0", 0) for u in units], np.int32),
                rir=np.asarray([u.get("rir", -1) for u in units], np.int32))
    if any(u.get("dis_rir", -1) >= 0 for u in units):
        cols["dis_sound"] = np.asarray([u.get("dis_sound", 0) for u in units], np.int32)
        cols["dis_rir"] = np.asarray([u.get("dis_rir", -1) for u in units], np.int32)
    return cols


BINDINGS = {"bank16": (SR, "small"), "bank16_rows": (SR44, "long"), "rir16_buckets": (SR, None)}


def _bound_context(world, scene, binding, **kw):
    """-> (context, units, check(lm, sg, label, kinds=None) against the quantised float64 model, tensors to keep alive)"""
    from ss_amd.context import AudioContext
    sr, name = BINDINGS[binding]
    ctx = AudioContext(sr, **kw)
    if binding == "rir16_buckets":
        for i, c in enumerate(scene.sc["srcs"]):
            ctx.add_source(str(i), c)
        ctx.set_rir16_buckets(scene.half)
        units = scene.sc["units"]
        return ctx, units, (lambda lm, sg, label, us=units: _scene_vs_model(scene, us, lm, sg, label)), None
    r, q, s, _ = _renderer(world, name, sr)
    for i, c in enumerate(world.srcs[sr]):
        ctx.add_source(str(i), c)
    ctx.set_rir_bank16(q, s, r.rirs.lengths, rows=binding == "bank16_rows")
    units = SIMPLE_UNITS + [dict(sound=0, t0=0, rir=3, dis_sound=1, dis_rir=2)] if sr == SR else _cycle("long", 5, sr)
    return ctx, units, (lambda lm, sg, label, us=units: _vs_model(world, name, us, sr, lm, sg, label)), (q, s, r)


@pytest.mark.parametrize("binding", list(BINDINGS))
def test_context_default_is_the_scratch_route_and_the_policy_opts_in(world, scene, binding):
    from ss_amd import _lib, ops
    sr = BINDINGS[binding][0]
    msd, mwd = _mel(sr)
    T, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    # default policy - and the four older ranges set to always, which never apply here: the scratch route, bit-equal to
    # observe-then-features
    ctx, units, check, keep = _bound_context(world, scene, binding)
    cols, n = _cols(units), len(units)
    for setter in (ctx.set_logmel_policy, ctx.set_logmel_rows_policy, ctx.set_logmel_ss2_policy, ctx.set_logmel_buckets_policy):
        setter(*ALWAYS)
    assert ctx.wave_scratch_bytes() == 0
    ag = _nan(n, 2, sr)
    ctx.observe(audiogoal_out=ag, **cols)
    lm0 = _nan(n, 64, T, 2)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm = _nan(n, 64, T, 2)
    ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert not torch.isnan(lm).any() and torch.equal(lm, lm0) and ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    ctx.close()
    # a fresh context that opts in: one fused launch per step, no waveform anywhere
    ctx, units, check, keep = _bound_context(world, scene, binding)
    ctx.set_logmel_rir16_policy(*ALWAYS)
    lm1, lm2, sg2 = _nan(n, 64, T, 2), _nan(n, 64, T, 2), _nan(n, 65, t4, 2)
    ctx.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    ctx.observe(spectrogram_out=sg2, logmel_out=lm2, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert ctx.wave_scratch_bytes() == 0                                 # the fused launch really ran
    check(lm1, None, f"context {binding} log-mel alone")
    check(lm2, sg2, f"context {binding} with the spectrogram")
    _rule(lm1, lm0, f"context {binding}: one launch vs the scratch route")
    # a cross-faded step: SS_EINVAL, nothing written, no keys left behind - the next step is intact
    with pytest.raises(_lib.SsHipError):
        ctx.observe(cols["sound"], cols["t0"], cols["rir"], logmel_out=lm2, mel_start=msd, mel_w=mwd, mel_eps=EPS,
                    last_rir=cols["rir"][::-1].copy())
    again = _nan(n, 64, T, 2)
    ctx.observe(logmel_out=again, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert torch.equal(again, lm1) and ctx.wave_scratch_bytes() == 0
    ctx.set_logmel_rir16_policy(n + 1, 1000)                             # outside the range: the scratch route
    lm3 = _nan(n, 64, T, 2)
    ctx.observe(logmel_out=lm3, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert torch.equal(lm3, lm0) and ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    ctx.close()


def test_overlap_lanes_under_the_always_policy(world, scene):
    """two internal lanes, four consecutive steps of different units: each within the rule, no waveform scratch"""
    ctx, units, _, keep = _bound_context(world, scene, "bank16")
    ctx.set_logmel_rir16_policy(*ALWAYS)
    ctx.set_overlap(2)
    msd, mwd = _mel(SR)
    T, t4 = 1 + SR // 160, P.spectrogram_shape(SR)[1]
    steps = [[0, 1, 2, 3, 4, 5], [5, 4, 0], [3, 3, 1, 2], [4, 0, 5, 1, 3]]
    outs = []
    for kinds in steps:
        lm, sg = _nan(len(kinds), 64, T, 2), _nan(len(kinds), 65, t4, 2)
        ctx.observe(spectrogram_out=sg, logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **_cols([units[k] for k in kinds]))
        outs.append((lm, sg))
    ctx.join()
    torch.cuda.synchronize()
    for kinds, (lm, sg) in zip(steps, outs):
        _vs_model(world, "small", [units[k] for k in kinds], SR, lm, sg, f"overlap {kinds}")
    assert ctx.wave_scratch_bytes() == 0
    ctx.set_overlap(1)
    ctx.close()


# ---- 3. the engine -----------------------------------------------------------------------------------------------------------
def _write_rirs(root, sr, taps):
    """float32 stereo wav files -> [(path, wav-layout array)]"""
    from scipy.io import wavfile
    files = []
    for k, n in enumerate(taps):
        rng = np.random.default_rng(2000 + k)
        h = (O.synth_rir(rng, sr, length=n, n=1) if n <= P.KB else O.synth_rir_blocks(rng, sr, n, n=1))[0]
        h = np.ascontiguousarray(h.T.astype(np.float32))
        p = str(root / f"{k}_{n}.wav")
        wavfile.write(p, sr, h)
        files.append((p, h))
    return files


@pytest.mark.parametrize("kind,sr,taps", [("plain", SR, (16000, 9000, 3000, 15999, 12000)),
                                          ("buckets", SR, (16000, 9000, 30000, 40000, 20000)),
                                          ("fused-rows", SR44, (44100, 20000, 9000, 30001, 44100))])
def test_engine_one_step_of_5_envs_policy_on_against_policy_off(world, tmp_path, kind, sr, taps):
    from ss_amd.renderer import AudioEngine
    files = _write_rirs(tmp_path, sr, taps)
    kw = dict(plain={}, buckets=dict(rir_buckets=ENGINE_BUCKETS), **{"fused-rows": dict(rir_rows16_fused=True)})[kind]
    eng = AudioEngine(sr, device=DEV, rir_slots=8, rir_rows="half", **kw)
    clips = [world.srcs[sr][0], world.srcs[sr][2]]
    sid = [eng.source_id(f"clip{i}", c) for i, c in enumerate(clips)]
    paths = [p for p, _ in files]
    slots = eng.store.load_files(paths, paths)
    n = len(files)
    cols = dict(sound=np.asarray([sid[k % 2] for k in range(n)], np.int32), t0=np.asarray([2 * sr if k % 2 else 0 for k in range(n)], np.int32),
                rir=np.asarray(slots, np.int32))
    msd, mwd = _mel(sr)
    T = 1 + sr // 160
    eng.context().set_logmel_rir16_policy(*ALWAYS)                       # callers set the policy on the engine's context
    ctx = eng._sync_context_bank(n, False)
    lm_on = _nan(n, 64, T, 2)
    ctx.observe(logmel_out=lm_on, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert ctx.wave_scratch_bytes() == 0
    eng._ctx_bank = None                                                 # the engine binds its bank again: the policy stays
    ctx = eng._sync_context_bank(n, False)
    lm_again = _nan(n, 64, T, 2)
    ctx.observe(logmel_out=lm_again, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert ctx.wave_scratch_bytes() == 0 and torch.equal(lm_again, lm_on)
    ctx.set_logmel_rir16_policy(1, 0)
    lm_off = _nan(n, 64, T, 2)
    ctx.observe(logmel_out=lm_off, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    assert ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    _rule(lm_on, lm_off, f"engine {kind}: policy on against policy off")
    got = lm_on.cpu().numpy()
    for k, (p, wav) in enumerate(files):                                 # ... and each env against the quantised model of its file
        ref = O.compute_logmel(R.model_audiogoal(clips[k % 2], np.ascontiguousarray(wav.T), 2 * sr if k % 2 else 0, sr), sr, 64, EPS)
        err = np.abs(got[k] - ref).max() / np.abs(ref).max()
        print(f"[gpu_rir16_logmel] engine {kind} env {k}: log-mel vs quantised float64 model of the file = {err:.3e}")
        assert err <= MEL_TOL, (kind, k, err)
