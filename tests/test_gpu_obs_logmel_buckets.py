"""Fused log-mel from length-bucketed RIR banks on the GPU (include/ss_hip.h ss_audio_obs_logmel_buckets_f32 /
ss_audio_obs_logmel_spec_buckets_f32 / ss_ctx_set_logmel_buckets_policy): ONE launch, no waveform buffer, on every bank form of
the length-bucketed store - rows (with and without spectra, ss_rir_bucket), fp32 spectra alone ("only") and fp16 spectra with
scales ("half", ss_spec_bucket).

16 kHz: the 12-unit scene of tests/spec_buckets_ref.py (four buckets of 1 / 2 / 3 / 5 blocks).  44.1 kHz: the same bank under
three-block rows, 5 units (k_obs_blocks) and 44 units (2 x 44 x 3 = 264 workgroups, more than the chip's 256 CUs: k_obs_rows).
  * stateless: the fused launch against two launches (ss_audio_obs_*buckets_f32 with a waveform, then ss_audio_features_f32) -
    log-mel within 1e-4 of the unit's largest value, the waveform bit-equal, the pooled spectrogram within 1e-4; all three
    outputs and log-mel alone;
  * SS_FLAG_FIRST_BUCKET launches equal the single-allocation log-mel entries on bucket 0's arrays bit for bit;
  * context: under set_logmel_buckets_policy(1, 2**31 - 1) log-mel within 1e-4 of the oracle (half: of the float64 model fed the
    bank's own halves) and no waveform scratch; under the default policy bit-equal to observe-then-features, with the scratch;
    a step outside the range and a cross-faded step take the scratch route; overlap lanes.
Every output is pre-filled with NaN."""
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_buckets_ref as B
import spec_half_rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = B.SR
SR44 = 44100
TOL = 1e-4
EPS = 1e-6
ALWAYS = (1, 2 ** 31 - 1)
# the units of the 44.1 kHz launches over the same bank: every bucket, the 9000-tap entry, the empty entry, a silent unit, a unit
# whose two terms sit in buckets 1 and 2
KINDS44 = [dict(sound=0, t0=0, rir=0), dict(sound=0, t0=0, rir=4), dict(sound=0, t0=0, rir=5), dict(sound=0, t0=0, rir=8),
           dict(sound=0, t0=0, rir=9), dict(sound=0, t0=0, rir=B.EMPTY), dict(rir=-1),
           dict(sound=0, t0=0, rir=3, dis_sound=0, dis_rir=7)]


def _new(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _mel(sr, n_mels=64):
    ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
    return torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)


def _unit_requests(units):
    from ss_amd.renderer import UnitRequest
    return [UnitRequest(silent=True) if u.get("rir", -1) < 0 else
            UnitRequest(u["sound"], u["t0"], u["rir"], dis_sound=u.get("dis_sound", -1), dis_rir=u.get("dis_rir", -1)) for u in units]


def _wav(sc, g):
    return np.ascontiguousarray(B.row_of(sc, g).T)


def _oracle_wave(sc, srcs, u, sr):
    g = u.get("rir", -1)
    if g < 0 or g == B.EMPTY:
        return None
    kw = {}
    if u.get("dis_rir", -1) >= 0:
        kw = dict(distractor=srcs[u["dis_sound"]], distractor_rir=_wav(sc, u["dis_rir"]))
    return np.asarray(O.compute_audiogoal(srcs[u["sound"]], _wav(sc, g), sr, audio_index=u["t0"] // sr, **kw), np.float32)


def _build_world():
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank
    sc = B.scene()
    lengths = torch.from_numpy(sc["lens"]).to(DEV)
    rows = [torch.from_numpy(r).to(DEV) for r in sc["rows"]]
    f32 = [ops.rir_spectra(r) for r in rows]
    half = [ops.rir_spectra16(r) for r in rows]
    q, s = [h[0] for h in half], [h[1] for h in half]

    def views():
        return [lengths[f:f + n] for f, n in zip(B.FIRST, B.COUNTS)]

    def with_rows(spectra):
        banks = []
        for r, v, sp in zip(rows, views(), spectra):
            bank = RirBank(r, v)
            bank.spectra = sp
            banks.append(bank)
        return BucketedRirBank(banks, lengths, B.FIRST)

    def only(spectra, scales=None):
        banks = []
        for b, (v, sp) in enumerate(zip(views(), spectra)):
            bank = RirBank(torch.zeros((B.COUNTS[b], 2, 0), dtype=torch.float32, device=DEV), v, cap=B.CAPS[b])
            bank.spectra = sp
            bank.scales = scales[b] if scales is not None else None
            banks.append(bank)
        return BucketedRirBank(banks, lengths, B.FIRST)

    banks = dict(rows=with_rows(f32), both=with_rows(f32), only=only(f32), half=only(q, s))
    r16 = BatchedAudioRenderer(SR, device=DEV)
    for i, src in enumerate(sc["srcs"]):
        r16.add_source(f"s{i}", src)
    r16.set_rir_bank(banks["both"])
    src44 = [O.synth_sources(np.random.default_rng(4), SR44, k=1)[0]]
    r44 = BatchedAudioRenderer(SR44, device=DEV)
    r44.add_source("a", src44[0])
    r44.set_rir_bank(banks["both"])
    perm = R.kernel_order(lambda x: ops.rir_spectra(torch.from_numpy(np.ascontiguousarray(x)).to(DEV)).cpu().numpy())
    torch.cuda.synchronize()
    w = types.SimpleNamespace(sc=sc, lengths=lengths, banks=banks, rows=rows, f32=f32, q=q, s=s, perm=perm,
                              qn=[a.cpu().numpy() for a in q], sn=[a.cpu().numpy() for a in s],
                              r={SR: r16, SR44: r44}, srcs={SR: sc["srcs"], SR44: src44}, units={SR: sc["units"], SR44: KINDS44})
    w.waves = {sr: [_oracle_wave(sc, w.srcs[sr], u, sr) for u in w.units[sr]] for sr in (SR, SR44)}
    w.ref_mel, w.ref_sg, w.model_mel = {}, {}, {}
    return w


@pytest.fixture(scope="module", autouse=True)
def _private_pool():
    """Every torch allocation of this module - fixtures, tests, the renderers they drive - comes from a memory pool of the
    module's own and goes back to the driver with it.  Later modules of the suite hold torch.cuda.memory_allocated deltas of a
    store to the byte, and the caching allocator hands a cached block out whole when it is less than 1 MiB larger than the
    request: whatever this module left in the process's default pool - and equally an empty_cache() that took other modules'
    blocks out of it - would decide whether they pass.  With the pool the default one never sees this module."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        torch.cuda.synchronize()
    del pool


@pytest.fixture(scope="module")
def world(_private_pool):
    """the scene on the device: per bucket the rows, their fp32 spectra and the half form; the bucketed banks built from them;
    renderers that plan the launches at both rates; the oracle's waveform of every unit (computed once)"""
    import gc
    w = _build_world()
    yield w
    w.__dict__.clear()                                   # (before the pool goes: nothing of it stays allocated)
    del w
    gc.collect()
    torch.cuda.synchronize()


def _ref_mel(w, sr, k):
    if (sr, k) not in w.ref_mel:
        a = w.waves[sr][k]
        w.ref_mel[(sr, k)] = None if a is None else O.compute_logmel(a, sr, n_mels=64, eps=EPS)
        w.ref_sg[(sr, k)] = None if a is None else O.compute_spectrogram(a)
    return w.ref_mel[(sr, k)], w.ref_sg[(sr, k)]


def _model_mel(w, k):
    """log-mel of the float64 overlap-save model of 16 kHz unit k fed the halves and scales the half bank holds"""
    if k not in w.model_mel:
        sc, u = w.sc, w.sc["units"][k]
        out = np.zeros((2, SR))
        for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
            b = B.bucket_of(g)
            nbh = max(1, P.ceil_div(int(sc["lens"][g]), P.KB))          # (the kernel skips the blocks behind the entry's length)
            spectra = R.bank_spectra(w.qn[b][g - B.FIRST[b]], w.sn[b][g - B.FIRST[b]], w.perm)[:, :nbh]
            out += R.model_audiogoal(sc["srcs"][snd], None, t0, SR, spectra=spectra)
        w.model_mel[k] = (O.compute_logmel(out.astype(np.float32), SR, n_mels=64, eps=EPS), O.compute_spectrogram(out.astype(np.float32)))
    return w.model_mel[k]


def _check_vs_reference(w, sr, kinds, lm, sg, form, tag):
    """every unit against the oracle of its kind (half: the model fed the bank's halves): log-mel 1e-4 of the unit's largest value,
    pooled spectrogram 1e-4; silent units and empty RIRs log(eps) and exact zeros"""
    lm = lm.cpu().numpy()
    sg = None if sg is None else sg.cpu().numpy()
    assert not np.isnan(lm).any() and (sg is None or not np.isnan(sg).any()), tag
    worst = 0.0
    for i, k in enumerate(kinds):
        ref, ref_sg = _ref_mel(w, sr, k)
        if ref is None:
            assert np.allclose(lm[i], np.log(EPS), rtol=1e-6, atol=0), (tag, i)
            assert sg is None or not sg[i].any(), (tag, i)
            continue
        if form == "half":
            ref, ref_sg = _model_mel(w, k)
        err = np.abs(lm[i] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= TOL, (tag, i, k, err)
        if sg is not None:
            e = O.relerr(sg[i], ref_sg)
            assert e <= TOL, (tag, i, k, e)
    print(f"[gpu_obs_logmel_buckets] {tag}: worst log-mel error vs {'model' if form == 'half' else 'oracle'} {worst:.3g}")


def _entries(w, form):
    """(bucket array, two-launch entry, fused entry) of a bank form"""
    from ss_amd import ops
    bank = w.banks[form]
    if form in ("only", "half"):
        return bank.spec_c_array(), ops.audio_obs_spec_buckets_into, ops.audio_obs_logmel_spec_buckets_into
    return bank.c_array(form == "both"), ops.audio_obs_buckets_into, ops.audio_obs_logmel_buckets_into


def _fused_vs_two_launches(w, sr, form, kinds, n_mels):
    from ss_amd import ops
    r = w.r[sr]
    plan = r.plan(_unit_requests([w.units[sr][k] for k in kinds]))
    arr, obs, fused = _entries(w, form)
    msd, mwd = _mel(sr, n_mels)
    N, T, t4 = len(kinds), 1 + sr // 160, P.spectrogram_shape(sr)[1]
    ag0, sg0, lm0 = _new(N, 2, sr), _new(N, 65, t4, 2), _new(N, n_mels, T, 2)
    obs(r._spec, arr, 4, w.lengths, plan.desc, ag0, sg0, sr, sr, "reflect", flags=plan.flags)
    ops.audio_features_into(ag0, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    ag1, sg1, lm1 = _new(N, 2, sr), _new(N, 65, t4, 2), _new(N, n_mels, T, 2)            # all three outputs: one launch
    fused(r._spec, arr, 4, w.lengths, plan.desc, ag1, sg1, lm1, msd, mwd, sr, sr, EPS, "reflect", flags=plan.flags)
    lm2 = _new(N, n_mels, T, 2)                                                            # log-mel alone: no buffer at all
    fused(r._spec, arr, 4, w.lengths, plan.desc, None, None, lm2, msd, mwd, sr, sr, EPS, "reflect", flags=plan.flags)
    torch.cuda.synchronize()
    for t in (ag0, sg0, lm0, ag1, sg1, lm1, lm2):
        assert not torch.isnan(t).any()
    assert torch.equal(ag1, ag0)                                         # (same convolution code, same order: same bits)
    e_sg = O.relerr(sg1.cpu().numpy(), sg0.cpu().numpy())
    ref_max = lm0.abs().amax(dim=(1, 2, 3))                              # per unit
    e1 = float(((lm1 - lm0).abs().amax(dim=(1, 2, 3)) / ref_max).max())
    e2 = float(((lm2 - lm0).abs().amax(dim=(1, 2, 3)) / ref_max).max())
    print(f"[gpu_obs_logmel_buckets] sr {sr} {form} n {N}: fused vs two launches log-mel {e1:.3g} (alone {e2:.3g}) spectrogram {e_sg:.3g}")
    assert e_sg <= TOL and e1 <= TOL and e2 <= TOL, (e_sg, e1, e2)
    for i, k in enumerate(kinds):                                        # silent units and empty RIRs
        if w.waves[sr][k] is None:
            assert torch.allclose(lm2[i], torch.full_like(lm2[i], float(np.log(EPS))), rtol=1e-6, atol=0) and not sg1[i].any()
            assert not ag1[i].any()
    return plan, lm1, sg1


@pytest.mark.parametrize("form", ["both", "only", "half"])
def test_stateless_16k_fused_against_two_launches(world, form):
    kinds = list(range(len(world.sc["units"])))
    plan, lm1, sg1 = _fused_vs_two_launches(world, SR, form, kinds, 64)
    assert not (plan.flags & 7)                                          # distractor terms, no cross-fade, not bucket 0 alone
    _check_vs_reference(world, SR, kinds, lm1, sg1, form, f"stateless 16 kHz {form}")


@pytest.mark.parametrize("n_units", [5, 44], ids=["5-units-blocks-kernel", "44-units-rows-kernel"])
@pytest.mark.parametrize("form", ["rows", "both", "only"])
def test_stateless_44k_fused_against_two_launches(world, form, n_units):
    """5 units: k_obs_blocks<.., MEL>; 44 units: the first count whose 264 workgroups exceed the chip: k_obs_rows<.., BUCKETS, MEL>"""
    kinds = [(i + 3) % len(KINDS44) for i in range(n_units)]
    _, lm1, sg1 = _fused_vs_two_launches(world, SR44, form, kinds, 64)
    _check_vs_reference(world, SR44, kinds, lm1, sg1, form, f"stateless 44.1 kHz {form} n {n_units}")


def test_half_buckets_refuse_long_rows(world):
    from ss_amd import _lib, ops
    r = world.r[SR44]
    plan = r.plan(_unit_requests(KINDS44[:2]))
    msd, mwd = _mel(SR44)
    with pytest.raises(_lib.SsHipError):
        ops.audio_obs_logmel_spec_buckets_into(r._spec, world.banks["half"].spec_c_array(), 4, world.lengths, plan.desc, None, None,
                                               _new(2, 64, 1 + SR44 // 160, 2), msd, mwd, SR44, SR44, EPS, "reflect", flags=plan.flags)


@pytest.mark.parametrize("sr,form", [(SR, "rows"), (SR, "both"), (SR, "only"), (SR, "half"), (SR44, "rows"), (SR44, "only")])
def test_first_bucket_launch_is_the_single_allocation_entry_on_bucket_0(world, sr, form):
    """every index in bucket 0: with SS_FLAG_FIRST_BUCKET the launch IS the single-allocation log-mel launch on bucket 0's arrays -
    loop-free kernel (no distractor) or loop kernel - bit for bit on all three outputs"""
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    r = world.r[sr]
    units = [UnitRequest(0, 0, 0), UnitRequest(0, 0, 2), UnitRequest(0, 0, B.EMPTY), UnitRequest(silent=True), UnitRequest(0, 0, 0)]
    plan = r.plan(units)
    assert plan.flags == ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET
    arr, _, fused = _entries(world, form)
    msd, mwd = _mel(sr)
    n, T, t4 = len(units), 1 + sr // 160, P.spectrogram_shape(sr)[1]
    long_rows = sr > P.KB
    for flags in (plan.flags, ops.FLAG_FIRST_BUCKET):
        got = [_new(n, 2, sr), _new(n, 65, t4, 2), _new(n, 64, T, 2)]
        fused(r._spec, arr, 4, world.lengths, plan.desc, *got, msd, mwd, sr, sr, EPS, "reflect", flags=flags)
        want = [_new(n, 2, sr), _new(n, 65, t4, 2), _new(n, 64, T, 2)]
        single_flags = flags & ~ops.FLAG_FIRST_BUCKET
        if form == "rows":
            single = ops.audio_obs_logmel_rows_into if long_rows else ops.audio_obs_logmel_into
            single(r._spec, world.rows[0], world.lengths, plan.desc, *want, msd, mwd, sr, sr, EPS, "reflect", flags=single_flags)
        else:
            single = ops.audio_obs_logmel_rows_spec_into if long_rows else ops.audio_obs_logmel_spec_into
            bank0 = world.q[0] if form == "half" else world.f32[0]
            single(r._spec, bank0, world.lengths, plan.desc, *want, msd, mwd, sr, sr, EPS, "reflect", flags=single_flags,
                   hscale=world.s[0] if form == "half" else None)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert not torch.isnan(a).any() and torch.equal(a, b), (form, flags)
        assert got[0][0].any() and not got[0][2].any() and not got[0][3].any()


# ---- the context: ss_ctx_set_logmel_buckets_policy ---------------------------------------------------------------------------
def _context(w, sr, binding, **kw):
    from ss_amd.context import AudioContext
    ctx = AudioContext(sr, **kw)
    for i, c in enumerate(w.srcs[sr]):
        ctx.add_source(str(i), c)
    if binding in ("only", "half"):
        ctx.set_rir_spec_buckets(w.banks[binding])
    else:
        ctx.set_rir_buckets(w.banks[binding], spectral=binding == "both")
    return ctx


def _cols(w, sr, kinds):
    us = [w.units[sr][k] for k in kinds]
    cols = dict(sound=np.array([u.get("sound", 0) for u in us]), t0=np.array([u.get("t0", 0) for u in us]),
                rir=np.array([u.get("rir", -1) for u in us]))
    if any("dis_rir" in u for u in us):
        cols.update(dis_sound=np.array([u.get("dis_sound", 0) for u in us]), dis_rir=np.array([u.get("dis_rir", -1) for u in us]))
    return cols


@pytest.mark.parametrize("sr,binding", [(SR, "rows"), (SR, "both"), (SR, "only"), (SR, "half"), (SR44, "rows"), (SR44, "only")])
def test_context_default_is_the_scratch_route_and_the_policy_opts_in(world, sr, binding):
    from ss_amd import ops
    kinds = list(range(len(world.units[sr])))
    cols = _cols(world, sr, kinds)
    msd, mwd = _mel(sr)
    n, T, t4 = len(kinds), 1 + sr // 160, P.spectrogram_shape(sr)[1]
    # default policy - and the rows policy set to always, which never applies here: the scratch route, bit-equal to
    # observe-then-features
    ctx = _context(world, sr, binding)
    ctx.set_logmel_rows_policy(*ALWAYS)
    assert ctx.wave_scratch_bytes() == 0
    ag = _new(n, 2, sr)
    ctx.observe(audiogoal_out=ag, **cols)
    lm0 = _new(n, 64, T, 2)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm = _new(n, 64, T, 2)
    ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert not torch.isnan(lm).any() and torch.equal(lm, lm0) and ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    ctx.close()
    # a fresh context that opts in: one fused launch per step, no waveform anywhere
    ctx = _context(world, sr, binding)
    ctx.set_logmel_buckets_policy(*ALWAYS)
    lm1, lm2, sg2 = _new(n, 64, T, 2), _new(n, 64, T, 2), _new(n, 65, t4, 2)
    ctx.observe(logmel_out=lm1, mel_start=msd, mel_w=mwd, **cols)
    ctx.observe(spectrogram_out=sg2, logmel_out=lm2, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert ctx.wave_scratch_bytes() == 0                                 # the fused launch really ran
    _check_vs_reference(world, sr, kinds, lm1, None, binding, f"context {sr} {binding} log-mel alone")
    _check_vs_reference(world, sr, kinds, lm2, sg2, binding, f"context {sr} {binding} with the spectrogram")
    err = float(((lm1 - lm0).abs().amax(dim=(1, 2, 3)) / lm0.abs().amax(dim=(1, 2, 3))).max())
    assert err <= TOL, err                                               # ... and within the rule of the scratch route's result
    ctx.set_logmel_buckets_policy(n + 1, 1000)                           # outside the range: the scratch route
    lm3 = _new(n, 64, T, 2)
    ctx.observe(logmel_out=lm3, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert torch.equal(lm3, lm0) and ctx.wave_scratch_bytes() >= n * 2 * sr * 4
    ctx.close()


def test_cross_faded_step_on_a_rows_bucketed_context_keeps_the_scratch_route(world):
    """SoundSpaces 2.0 steps (0.25 s) with a cross-fade from the previous RIR: bit-equal to observe-then-features under the always
    policy; the same context's plain first step (no previous RIR) takes the fused launch"""
    from ss_amd import ops
    msd, mwd = _mel(SR)
    T = 1 + SR // 160
    ctx = _context(world, SR, "rows", step_time=0.25, wrap=True)
    ctx.set_logmel_buckets_policy(*ALWAYS)
    cur, last = np.array([0, 4, 7, 9]), np.array([3, 0, 8, 2])
    plain = dict(sound=np.zeros(4), t0=np.full(4, 100), rir=cur, wrap=np.zeros(4, np.uint8))
    lm_first = _new(4, 64, T, 2)
    ctx.observe(logmel_out=lm_first, mel_start=msd, mel_w=mwd, **plain)
    torch.cuda.synchronize()
    assert not torch.isnan(lm_first).any() and ctx.wave_scratch_bytes() == 0
    cols = dict(plain, last_rir=last, last_wrap=np.zeros(4, np.uint8))
    ag = _new(4, 2, SR)
    ctx.observe(audiogoal_out=ag, **cols)
    lm0 = _new(4, 64, T, 2)
    ops.audio_features_into(ag, logmel_out=lm0, mel_start=msd, mel_w=mwd, mel_eps=EPS)
    lm = _new(4, 64, T, 2)
    ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, **cols)
    torch.cuda.synchronize()
    assert not torch.isnan(lm).any() and torch.equal(lm, lm0) and ctx.wave_scratch_bytes() >= 4 * 2 * SR * 4
    ctx.close()


@pytest.mark.parametrize("binding", ["both", "half"])
def test_overlap_lanes_under_the_always_policy(world, binding):
    """two internal lanes, three consecutive steps of different units: each within the rule, no waveform scratch"""
    ctx = _context(world, SR, binding)
    ctx.set_logmel_buckets_policy(*ALWAYS)
    ctx.set_overlap(2)
    msd, mwd = _mel(SR)
    T, t4 = 1 + SR // 160, P.spectrogram_shape(SR)[1]
    steps = [[0, 1, 2, 3, 4, 11], [9, 10, 6, 5, 7, 8, 0], [1, 1, 9]]
    outs = []
    for kinds in steps:
        lm, sg = _new(len(kinds), 64, T, 2), _new(len(kinds), 65, t4, 2)
        ctx.observe(spectrogram_out=sg, logmel_out=lm, mel_start=msd, mel_w=mwd, **_cols(world, SR, kinds))
        outs.append((lm, sg))
    ctx.join()
    torch.cuda.synchronize()
    for kinds, (lm, sg) in zip(steps, outs):
        _check_vs_reference(world, SR, kinds, lm, sg, binding, f"overlap {binding} {kinds}")
    assert ctx.wave_scratch_bytes() == 0
    ctx.set_overlap(1)
    ctx.close()
