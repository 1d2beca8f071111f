"""Half spectral length buckets under rows of 2 or 3 partition blocks on the GPU: ss_audio_obs_rows_spec16_buckets_f32,
ss_audio_obs_logmel_rows_spec16_buckets_f32 (k_obs_blocks<true, MEL, HALF, HBK> while the grid fits the chip, k_obs_rows<true, false,
BUCKETS, MEL, HALF> beyond), ss_ctx_set_rir_spec_buckets_rows and AudioEngine(rir_half_bucket_rows=True).  The scene is
tests/spec_half_bucket_rows_world.py: buckets of 1 / 3 / 5 blocks, RIR lengths below, at and clamped by their bucket's depth, entries
scaled by 32 768 and 1e-6 in different buckets, a unit whose terms sit in buckets of different depth, a silent unit, the empty RIR,
the 3-s clip at t0 = 1 s.  Every output is pre-filled with NaN; none may survive.

  * against ss_audio_obs_spec_buckets_f32 / ss_audio_obs_logmel_spec_buckets_f32 on fp32 buckets holding float(q) * hscale:
    <= 2e-6 of peak, the project's A/B bound (log-mel: 1e-4 of the unit's largest value);
  * against the float64 overlap-save model fed the bank's own halves and scales: <= 1e-4 of peak on waveform and pooled spectrogram;
  * SS_FLAG_FIRST_BUCKET launches: bit for bit ss_audio_obs_rows_spec16_f32 / ss_audio_obs_logmel_rows_spec16_f32 on bucket 0's arrays;
  * the engine at 44.1 kHz: eager, a context step, the vector observer, log-mel inside and outside the buckets policy, and the
    cross-fade refusal.
Nothing here captures a graph (a k_obs_blocks launch must not be replayed from one)."""
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_half_bucket_rows_world as W
import spec_half_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUDGET = 1e-4
AB = 2e-6
MEL_TOL = 1e-4
EPS = 1e-6
N_MELS = 64


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _unit_requests(units):
    from ss_amd.renderer import UnitRequest
    return [UnitRequest(silent=True) if u.get("rir", -1) < 0 else
            UnitRequest(u["sound"], u["t0"], u["rir"], dis_sound=u.get("dis_sound", -1), dis_rir=u.get("dis_rir", -1)) for u in units]


@pytest.fixture(scope="module")
def world():
    """the scene on the device: per bucket the fp32 spectra of its rows, their half form and the dequantised halves; the half
    bucketed bank and the fp32 one holding the dequantised spectra; the kernel's component order.  Built once, never written to."""
    from ss_amd import ops
    from ss_amd.renderer import BucketedRirBank, RirBank
    sc = W.scene()
    lengths = torch.from_numpy(np.array(sc["lens"])).to(DEV)
    rows = [torch.from_numpy(np.array(r)).to(DEV) for r in sc["rows"]]
    half = [ops.rir_spectra16(r) for r in rows]
    q, s = [h[0] for h in half], [h[1] for h in half]
    deq = [(a.float() * b[..., None]).contiguous() for a, b in half]          # float(q) * hscale, exact in fp32

    def only(spectra, scales=None):
        banks = []
        for b, sp in enumerate(spectra):
            bank = RirBank(torch.zeros((W.COUNTS[b], 2, 0), dtype=torch.float32, device=DEV),
                           lengths[W.FIRST[b]:W.FIRST[b] + W.COUNTS[b]], cap=W.CAPS[b])
            bank.spectra = sp
            bank.scales = scales[b] if scales is not None else None
            banks.append(bank)
        return BucketedRirBank(banks, lengths, W.FIRST)

    perm = R.kernel_order(lambda x: ops.rir_spectra(torch.from_numpy(np.ascontiguousarray(x)).to(DEV)).cpu().numpy())
    torch.cuda.synchronize()
    return types.SimpleNamespace(lengths=lengths, banks=dict(half=only(q, s), deq=only(deq)), perm=perm,
                                 q=[a.cpu().numpy() for a in q], s=[a.cpu().numpy() for a in s], qd=q, sd=s, plans={})


def _planned(w, sr, units):
    """a renderer at rate sr with the scene's sources, and the plan of `units` (cached per rate and unit list)"""
    from ss_amd.renderer import BatchedAudioRenderer
    key = (sr, len(units), tuple(u.get("rir", -1) for u in units))
    if key not in w.plans:
        r = BatchedAudioRenderer(sr, device=DEV)
        for i, src in enumerate(W.sources(sr)):
            r.add_source(f"s{i}", src)
        r.set_rir_bank(w.banks["deq"])
        w.plans[key] = (r, r.plan(_unit_requests(units)))
    return w.plans[key]


def _mel(sr):
    ms, mw, _ = P.mel_filterbank_sparse(sr, N_MELS)
    return (torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV))


def _launch(w, sr, units, which, n_valid=None, flags=None):
    """both entries of bank `which` (half: the new ones; deq: the fp32 spectral-bucket entries) over `units` ->
    dict(sg0 = spectrogram without a waveform buffer, ag / sg = both outputs, lm0 = log-mel alone, lag / lsg / lm = all three)"""
    from ss_amd import ops
    r, plan = _planned(w, sr, units)
    n_valid = sr if n_valid is None else n_valid
    flags = plan.flags if flags is None else flags
    n = len(units)
    ms, mw = _mel(sr)
    arr = w.banks[which].spec_c_array()
    shape, frames = r.spectrogram_shape, 1 + sr // 160
    o = dict(sg0=_nan(n, *shape), ag=_nan(n, 2, sr), sg=_nan(n, *shape), lm0=_nan(n, N_MELS, frames, 2), lag=_nan(n, 2, sr),
             lsg=_nan(n, *shape), lm=_nan(n, N_MELS, frames, 2))
    obs = ops.audio_obs_rows_spec16_buckets_into if which == "half" else ops.audio_obs_spec_buckets_into
    mel = ops.audio_obs_logmel_rows_spec16_buckets_into if which == "half" else ops.audio_obs_logmel_spec_buckets_into
    obs(r._spec, arr, 3, w.lengths, plan.desc, None, o["sg0"], n_valid, sr, flags=flags)
    mel(r._spec, arr, 3, w.lengths, plan.desc, None, None, o["lm0"], ms, mw, n_valid, sr, mel_eps=EPS, flags=flags)
    mel(r._spec, arr, 3, w.lengths, plan.desc, o["lag"], o["lsg"], o["lm"], ms, mw, n_valid, sr, mel_eps=EPS, flags=flags)
    if n_valid > P.KB:                                   # (with a waveform buffer, one rendered block goes to the unfused route)
        obs(r._spec, arr, 3, w.lengths, plan.desc, o["ag"], o["sg"], n_valid, sr, flags=flags)
    else:
        del o["ag"], o["sg"]
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    for k, a in out.items():
        assert not np.isnan(a[:, :, :n_valid] if k in ("ag", "lag") else a).any(), (which, k)
    return out


def _check_ab(units, got, ref, label, n_valid=None):
    for k in ref:
        a, b = got[k], ref[k]
        if k in ("ag", "lag") and n_valid is not None:
            a, b = a[:, :, :n_valid], b[:, :, :n_valid]
        if k.startswith("lm"):
            worst = 0.0
            for n in range(len(units)):                   # the project's log-mel rule: 1e-4 of the unit's largest value
                e = np.abs(a[n] - b[n]).max() / np.abs(b[n]).max()
                worst = max(worst, e)
                assert e <= MEL_TOL, (label, k, n, e)
                if not W.terms(units[n]) or units[n]["rir"] == W.EMPTY:
                    assert np.allclose(a[n], np.log(EPS), rtol=1e-6), (label, k, n)
            print(f"[gpu_spec_half_bucket_rows] {label} {k}: max |half - fp32(dequantised)| / unit max = {worst:.3e}")
            continue
        err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()
        print(f"[gpu_spec_half_bucket_rows] {label} {k}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        assert err <= AB, (label, k, err)
        for n, u in enumerate(units):                     # the silent unit and the empty RIR: exact zeros
            dead = not W.terms(u) or u["rir"] == W.EMPTY
            assert bool(a[n].any()) != dead, (label, k, n)


_REFS = {}


def _model(w, sr, u):
    """float64 overlap-save of unit u from the halves and scales the bank holds, cut where the kernels stop reading"""
    key = (sr, u["rir"], u.get("dis_rir", -1), u["t0"])
    if key not in _REFS:
        srcs = W.sources(sr)
        out = np.zeros((2, sr))
        for snd, t0, g in W.terms(u):
            b = W.bucket_of(g)
            nbh = min(P.ceil_div(W.LENS[g], P.KB), P.ceil_div(W.CAPS[b], P.KB))
            if nbh:
                spectra = R.bank_spectra(w.q[b][g - W.FIRST[b]], w.s[b][g - W.FIRST[b]], w.perm)[:, :nbh]
                out += R.model_audiogoal(srcs[snd], None, t0, sr, spectra=spectra)
        _REFS[key] = out
    return _REFS[key]


def _check_model(w, sr, units, got, label, n_valid=None, only=None):
    for n, u in enumerate(units):
        if not W.terms(u) or u["rir"] == W.EMPTY or (only is not None and n not in only):
            continue
        ref = _model(w, sr, u)
        for ag, sg in (("ag", "sg"), ("lag", "lsg")):
            if ag not in got:
                continue
            if n_valid is None:
                ea, es = O.relerr(got[ag][n], ref), O.relerr(got[sg][n], O.compute_spectrogram(ref.astype(np.float32)))
            else:
                ea, es = O.relerr(got[ag][n][:, :n_valid], ref[:, :n_valid]), 0.0
            print(f"[gpu_spec_half_bucket_rows] {label} unit {n} ({ag}): vs model fed the bank's halves waveform {ea:.3e} spectrogram {es:.3e}")
            assert ea <= BUDGET and es <= BUDGET, (label, n, ea, es)
        if n_valid is None:
            es = O.relerr(got["sg0"][n], O.compute_spectrogram(ref.astype(np.float32)))
            assert es <= BUDGET, (label, n, "sg0", es)


@pytest.mark.parametrize("case", ["44100-7", "44100-5", "22050-7"])
def test_blocks_route_against_fp32_buckets_and_the_model(world, case):
    """n_valid == out_len and few units: one workgroup per output block (k_obs_blocks); three blocks with a partial last one, and two"""
    sr, n = (int(x) for x in case.split("-"))
    units = W.units(sr)[:n]
    got, ref = _launch(world, sr, units, "half"), _launch(world, sr, units, "deq")
    _check_ab(units, got, ref, f"blocks {case}")
    _check_model(world, sr, units, got, f"blocks {case}")


def test_rows_route_forced_by_a_short_step(world):
    """n_valid = 40 000 < out_len: k_obs_blocks declines, k_obs_rows renders; the pooled blocks behind n_valid are written"""
    sr, n_valid = 44100, 40000
    units = W.units(sr)
    got, ref = _launch(world, sr, units, "half", n_valid=n_valid), _launch(world, sr, units, "deq", n_valid=n_valid)
    _check_ab(units, got, ref, "rows n_valid 40000", n_valid=n_valid)
    _check_model(world, sr, units, got, "rows n_valid 40000", n_valid=n_valid)


def test_rows_route_with_more_rows_than_cus(world):
    """130 units drawn from the same entries: 260 rows on the persistent k_obs_rows, whose row loop runs twice on some workgroups"""
    sr = 44100
    base = W.units(sr)
    units = [base[k % len(base)] for k in range(130)]
    got, ref = _launch(world, sr, units, "half"), _launch(world, sr, units, "deq")
    _check_ab(units, got, ref, "rows 130 units")
    _check_model(world, sr, units, got, "rows 130 units", only=range(123, 130))
    for k in ("sg0", "ag", "lm0"):                        # a unit's result depends on that unit alone
        for n in range(len(base), 130):
            assert got[k][n].tobytes() == got[k][n % len(base)].tobytes(), (k, n)


def test_first_bucket_launch_equals_the_single_allocation_entries_bit_for_bit(world):
    """every index in bucket 0: SS_FLAG_FIRST_BUCKET makes the launch a single-allocation one on bucket 0's arrays"""
    from ss_amd import ops
    sr = 44100
    units = [dict(sound=1, t0=sr, rir=1), dict(sound=0, t0=0, rir=2, dis_sound=1, dis_rir=1), dict(rir=-1), dict(sound=0, t0=0, rir=W.EMPTY)]
    r, plan = _planned(world, sr, units)
    assert plan.flags & ops.FLAG_FIRST_BUCKET and not plan.flags & ops.FLAG_NO_DISTRACTOR
    got = _launch(world, sr, units, "half")
    n, ms, mw = len(units), *_mel(sr)
    q0, s0, lens0 = world.qd[0], world.sd[0], world.lengths[:W.COUNTS[0]].contiguous()
    sg0, ag, sg = _nan(n, *r.spectrogram_shape), _nan(n, 2, sr), _nan(n, *r.spectrogram_shape)
    lm0, lag, lsg, lm = (_nan(n, N_MELS, 1 + sr // 160, 2), _nan(n, 2, sr), _nan(n, *r.spectrogram_shape), _nan(n, N_MELS, 1 + sr // 160, 2))
    ops.audio_obs_spec_into(r._spec, q0, lens0, plan.desc, None, sg0, sr, sr, flags=plan.flags, hscale=s0)
    ops.audio_obs_spec_into(r._spec, q0, lens0, plan.desc, ag, sg, sr, sr, flags=plan.flags, hscale=s0)
    ops.audio_obs_logmel_rows_spec_into(r._spec, q0, lens0, plan.desc, None, None, lm0, ms, mw, sr, sr, mel_eps=EPS, flags=plan.flags, hscale=s0)
    ops.audio_obs_logmel_rows_spec_into(r._spec, q0, lens0, plan.desc, lag, lsg, lm, ms, mw, sr, sr, mel_eps=EPS, flags=plan.flags, hscale=s0)
    torch.cuda.synchronize()
    for k, t in dict(sg0=sg0, ag=ag, sg=sg, lm0=lm0, lag=lag, lsg=lsg, lm=lm).items():
        assert got[k].tobytes() == t.cpu().numpy().tobytes(), k
    assert got["ag"][0].any() and got["ag"][1].any() and not got["ag"][2].any() and not got["ag"][3].any()
    # ... and the same launch without the promise resolves the buckets: equal to rounding
    loop = _launch(world, sr, units, "half", flags=plan.flags & ~ops.FLAG_FIRST_BUCKET)
    _check_ab(units, loop, got, "first-bucket launch vs bucket-resolving launch")


def test_stateless_cross_fade_is_refused(world):
    from ss_amd import _lib, ops
    sr = 44100
    units = W.units(sr)[:3]
    r, plan = _planned(world, sr, units)
    arr = world.banks["half"].spec_c_array()
    sg = _nan(len(units), *r.spectrogram_shape)
    with pytest.raises(_lib.SsHipError):
        ops.audio_obs_rows_spec16_buckets_into(r._spec, arr, 3, world.lengths, plan.desc, None, sg, sr, sr, flags=plan.flags | ops.FLAG_CROSSFADE)
    with pytest.raises(_lib.SsHipError):                  # the entries that refused half buckets at this length still do
        ops.audio_obs_spec_buckets_into(r._spec, arr, 3, world.lengths, plan.desc, None, sg, sr, sr, flags=plan.flags)
    torch.cuda.synchronize()
    assert bool(torch.isnan(sg).all())


# ---- AudioEngine(rir_buckets=..., rir_spectral="half", rir_spectral_buckets=True, rir_half_bucket_rows=True) --------------------
SR = 44100
ENGINE_BUCKETS = [(3, 16384), (2, 49152)]


def _rirs(seed, lens):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray((O.synth_rir_blocks(rng, SR, L, n=1) if L > P.KB else O.synth_rir(rng, SR, length=L, n=1))[0].T)
            for L in lens]


def _model_of_slot(eng, perm, clip, slot, t0):
    """the float64 model of one unit from the halves and scales the store holds in global entry `slot`"""
    st = eng.store
    b = st.bank.bucket_of(slot)
    sub, k, n = st.stores[b].bank, slot - st.first[b], int(st.host_len[slot])
    if n == 0:
        return np.zeros((2, SR))
    spectra = R.bank_spectra(sub.spectra[k].cpu().numpy(), sub.scales[k].cpu().numpy(), perm)
    return R.model_audiogoal(clip, None, t0, SR, spectra=spectra[:, :max(1, P.ceil_div(n, P.KB))])


def _check_unit(eng, perm, ag, sg, clip, wav, slot, t0, label):
    """against the model fed the entry's own halves and scales (1e-4), and - the entry holds THIS file - within 1e-3 of the
    unquantised model of the file (the format's loss is 2.0 - 2.6e-4 of peak; another file's RIR is ~1)"""
    ref = _model_of_slot(eng, perm, clip, slot, t0)
    ea, es = O.relerr(ag, ref), O.relerr(sg, O.compute_spectrogram(ref.astype(np.float32)))
    exact = R.model_audiogoal(clip, np.ascontiguousarray(np.asarray(wav, np.float32).T), t0, SR, quant=False)
    loss = O.relerr(ag, exact)
    print(f"[gpu_spec_half_bucket_rows] {label}: vs model waveform {ea:.3e} spectrogram {es:.3e}; vs UNQUANTISED model of the file {loss:.3e}")
    assert ea <= BUDGET and es <= BUDGET and loss <= 1e-3, (label, ea, es, loss)


def _engine():
    from ss_amd.renderer import AudioEngine
    return AudioEngine(SR, device=DEV, rir_buckets=ENGINE_BUCKETS, rir_spectral="half", rir_spectral_buckets=True, rir_half_bucket_rows=True)


def test_engine_eager_context_logmel_and_cross_fade_refusal(world):
    from ss_amd import _lib, ops
    from ss_amd.renderer import UnitRequest
    srcs = W.sources(SR)
    eng = _engine()
    st = eng.store
    assert st.bank.spectral_only and st.bank.half
    sid = [eng.source_id(f"s{i}", s) for i, s in enumerate(srcs)]          # (the 3-s clip: whole RIRs)
    lens = [9000, 16384, 30000, 49152]
    rirs = _rirs(5, lens)
    cases = [(0, 0, 0), (1, SR, 1), (1, SR, 2), (0, 0, 3)]                 # (sound, t0, rir): both buckets, the 3-s clip at 1 s
    eng.begin_batch()
    slots = [eng.rir_slot(("r", h), lambda h=h: rirs[h]) for _, _, h in cases]
    assert [st.bank.bucket_of(s) for s in slots] == [0, 0, 1, 1]
    units = [UnitRequest(sid[a], t0, s) for (a, t0, _), s in zip(cases, slots)] + [UnitRequest(silent=True)]
    units.append(UnitRequest(sid[0], 0, slots[0], dis_sound=sid[1], dis_rir=slots[3]))   # two terms, two buckets
    out = eng.observe(units, want_audiogoal=True)
    sg_only = eng.observe(units)["spectrogram"]                          # no waveform buffer: one launch of the row kernels
    n = len(units)
    sg2, ag2 = _nan(n, *eng.renderer.spectrogram_shape), _nan(n, 2, SR)
    cols = dict(sound=np.asarray([u.sound for u in units], np.int32), t0=np.asarray([u.t0 for u in units], np.int32),
                rir=np.asarray([-1 if u.silent else u.rir for u in units], np.int32),
                dis_sound=np.asarray([max(u.dis_sound, 0) for u in units], np.int32), dis_rir=np.asarray([u.dis_rir for u in units], np.int32))
    eng.observe_columns(cols, spectrogram_out=sg2, audiogoal_out=ag2)        # the C context (ss_ctx_set_rir_spec_buckets_rows)
    torch.cuda.synchronize()
    assert torch.equal(sg_only, out["spectrogram"])
    for label, ag, sg in (("eager", out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()),
                          ("context", ag2.cpu().numpy(), sg2.cpu().numpy())):
        assert not np.isnan(ag).any() and not np.isnan(sg).any()
        for k, (a, t0, h) in enumerate(cases):
            _check_unit(eng, world.perm, ag[k], sg[k], srcs[a], rirs[h], slots[k], t0, f"{label} unit {k}")
        assert not ag[4].any() and not sg[4].any()
        ref = _model_of_slot(eng, world.perm, srcs[0], slots[0], 0) + _model_of_slot(eng, world.perm, srcs[1], slots[3], 0)
        assert O.relerr(ag[5], ref) <= BUDGET and O.relerr(sg[5], O.compute_spectrogram(ref.astype(np.float32))) <= BUDGET, label
    # a cross-faded step is refused (it would read rows) and leaves no keys behind: the next step is correct
    ctx = eng._sync_context_bank(n, True)
    sg0 = sg2.clone()
    with pytest.raises(_lib.SsHipError):
        ctx.observe(cols["sound"], cols["t0"], cols["rir"], spectrogram_out=sg2, last_rir=cols["rir"][::-1].copy())
    torch.cuda.synchronize()
    assert torch.equal(sg2, sg0)
    sg3 = _nan(n, *eng.renderer.spectrogram_shape)
    eng.observe_columns(cols, spectrogram_out=sg3)
    torch.cuda.synchronize()
    assert torch.equal(sg3, sg0)
    # log-mel: outside the buckets policy (the default) through the waveform scratch - observe-then-features, bit for bit;
    # inside it the one-launch route, equal to the scratch route to the log-mel rule
    ms, mw = _mel(SR)
    lm = _nan(n, N_MELS, 1 + SR // 160, 2)
    ctx.observe(logmel_out=lm, mel_start=ms, mel_w=mw, mel_eps=EPS, **cols)
    ag3 = _nan(n, 2, SR)
    ctx.observe(audiogoal_out=ag3, **cols)
    want = ops.audio_features(ag3, ("logmel",), ms, mw, mel_eps=EPS)["logmel"]
    torch.cuda.synchronize()
    assert not bool(torch.isnan(lm).any()) and torch.equal(lm, want)
    ctx.set_logmel_buckets_policy(1, 100)
    lm2 = _nan(n, N_MELS, 1 + SR // 160, 2)
    ctx.observe(logmel_out=lm2, mel_start=ms, mel_w=mw, mel_eps=EPS, **cols)
    torch.cuda.synchronize()
    a, b = lm2.cpu().numpy(), lm.cpu().numpy()
    assert not np.isnan(a).any()
    for k in range(n):
        assert np.abs(a[k] - b[k]).max() <= MEL_TOL * np.abs(b[k]).max(), k


def test_engine_vector_observer(world):
    """2 in-process envs wandering over 16 poses of mixed length through the 3 + 2 entries (loads evict in both buckets)"""
    from fakes import FakeSim
    from ss_amd import sim_audio
    from test_deferred import apply, trajectory
    rng = np.random.default_rng(3)
    sounds = {"telephone.wav": O.synth_sources(rng, SR, k=1)[0], "long.wav": O.synth_sources(rng, SR, k=1, seconds=3)[0]}
    files = {}
    for az in (0, 90, 180, 270):
        for r in range(4):
            L = int(rng.integers(900, 16001)) if r < 2 else int(rng.integers(17000, 49153))
            files[f"rirs/replica/apartment_0/{az}/{r}_7.wav"] = _rirs(int(rng.integers(1 << 30)), [L])[0]
    eng = _engine()
    eng.store.truncate_to = None                                         # whole RIRs from the first step on (a 3-s clip is in play)
    sims = [FakeSim(SR, sounds, files, False) for _ in range(2)]
    obs = sim_audio.VectorAudioObserver(eng, [sim_audio.attach(s, eng, rir_reader=files.get) for s in sims], want_audiogoal=True)
    trajs = [trajectory(rk, 4) for rk in range(2)]
    for k in range(4):
        for rk, s in enumerate(sims):
            apply(s, k, trajs[rk][k])
        idx = [s._audio_index for s in sims]
        out = obs.observe()
        torch.cuda.synchronize()
        ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
        for rk, s in enumerate(sims):
            path = f"rirs/replica/apartment_0/{s.azimuth_angle}/{s._receiver_position_index}_{s._source_position_index}.wav"
            clip = sounds[s._current_sound]
            t0 = 0 if len(clip) == SR else idx[rk] * SR
            st = eng.store
            slot = st.first[st._where[path]] + st.stores[st._where[path]]._slot_of[path]
            _check_unit(eng, world.perm, ag[rk], sg[rk], clip, files[path], slot, t0, f"vector step {k} env {rk}")
    assert eng.store.bank.spectral_only and eng.store.bank.half and eng.store.misses >= 2
