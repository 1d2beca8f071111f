"""Spectral length buckets on the GPU (include/ss_hip.h "Spectral length buckets"): a length-bucketed bank that keeps fp32 block
spectra alone ("only") or fp16 block spectra with one scale per (entry, ear, block) ("half") and no time-domain rows -
ss_fftconv_binaural_spec_buckets_f32 / ss_audio_obs_spec_buckets_f32 / ss_ctx_set_rir_spec_buckets, k_conv_spec<.., HALF, HBK>,
BucketedRirStore(spectral_buckets=True), AudioEngine(rir_spectral_buckets=True).  16 kHz; the scene of tests/spec_buckets_ref.py:
four buckets of 1 / 2 / 3 / 5 partition blocks and ONE launch of 12 units over the first and last entry of each, a unit whose two
terms live in different buckets, a full-cap entry per bucket, a 9000-tap entry in the 5-block bucket, an empty entry, a silent
unit, the 3-s clip at t0 = 1 s and entries scaled by 32768 and 1e-6 (in different buckets).  Every output is pre-filled with NaN.

  * half against the fp32 sibling ss_*_buckets_f32 fed float(q) * hscale: <= 2e-6 of peak, the project's A/B bound (each fp32
    path is held to <= 1e-6 of peak against float64, the inputs are identical; the host build measures 0.0);
  * half against the float64 overlap-save model fed the bank's own halves and scales: <= 1e-4 of peak on waveform and pooled
    spectrogram (the project's budget); the distance to the UNQUANTISED oracle is printed, not asserted;
  * "only" against the both-forms bucketed bank: bit for bit (16 kHz both entries; 44.1 kHz through the fused row kernels);
  * a SS_FLAG_FIRST_BUCKET launch takes the loop-free kernel and equals the loop kernel to 2e-6;
  * the engine in both forms: eager, vector, deferred and C-context routes against the model, the cross-fade refusal, log-mel
    through the scratch route, re-bucketing, eviction, growth of the last bucket and the HBM formula."""
import os
import pickle
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
BUDGET = 1e-4
AB = 2e-6
EPS = 1e-6
FORMS = ["only", "half"]
ENGINE_BUCKETS = [(3, 16000), (2, 40000)]


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _unit_requests(units):
    from ss_amd.renderer import UnitRequest
    return [UnitRequest(silent=True) if u.get("rir", -1) < 0 else
            UnitRequest(u["sound"], u["t0"], u["rir"], dis_sound=u.get("dis_sound", -1), dis_rir=u.get("dis_rir", -1)) for u in units]


@pytest.fixture(scope="module")
def world():
    """the scene on the device: per bucket the rows, their fp32 spectra, the half form and the dequantised halves; the three
    bucketed banks built from them; a renderer that planned the 12-unit launch; the kernel's component order"""
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank
    sc = B.scene()
    lengths = torch.from_numpy(sc["lens"]).to(DEV)
    rows = [torch.from_numpy(r).to(DEV) for r in sc["rows"]]
    f32 = [ops.rir_spectra(r) for r in rows]
    half = [ops.rir_spectra16(r) for r in rows]
    q, s = [h[0] for h in half], [h[1] for h in half]
    deq = [(a.float() * b[..., None]).contiguous() for a, b in half]          # float(q) * hscale, exact in fp32

    def views():
        return [lengths[f:f + n] for f, n in zip(B.FIRST, B.COUNTS)]

    def both(spectra):
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

    r = BatchedAudioRenderer(SR, device=DEV)
    for i, src in enumerate(sc["srcs"]):
        r.add_source(f"s{i}", src)
    banks = dict(both=both(f32), both_deq=both(deq), only=only(f32), half=only(q, s))
    r.set_rir_bank(banks["both"])
    plan = r.plan(_unit_requests(sc["units"]))
    perm = R.kernel_order(lambda x: ops.rir_spectra(torch.from_numpy(np.ascontiguousarray(x)).to(DEV)).cpu().numpy())
    torch.cuda.synchronize()
    qn, sn = [a.cpu().numpy() for a in q], [a.cpu().numpy() for a in s]
    return types.SimpleNamespace(sc=sc, lengths=lengths, banks=banks, r=r, plan=plan, perm=perm, q=qn, s=sn, rows=rows, f32=f32)


def _stateless(w, which):
    """the 12-unit launch on bank `which` through both stateless entries -> dict(conv, ag, sg) of numpy arrays"""
    from ss_amd import ops
    bank, r, plan = w.banks[which], w.r, w.plan
    n = len(plan)
    conv, ag, sg = _nan(n, 2, SR), _nan(n, 2, SR), _nan(n, *r.spectrogram_shape)
    if which in ("only", "half"):
        arr = bank.spec_c_array()
        ops.fftconv_binaural_spec_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, conv, r.n_valid, flags=plan.flags)
        ops.audio_obs_spec_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
    else:
        arr = bank.c_array(True)
        ops.audio_obs_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, conv, None, r.n_valid, r.out_len, flags=plan.flags)
        ops.audio_obs_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
    torch.cuda.synchronize()
    out = dict(conv=conv.cpu().numpy(), ag=ag.cpu().numpy(), sg=sg.cpu().numpy())
    for k, a in out.items():
        assert not np.isnan(a).any(), (which, k)
    return out


@pytest.fixture(scope="module")
def launches(world):
    assert not (world.plan.flags & 7)                                   # distractor terms, no cross-fade, not bucket 0 alone
    return {which: _stateless(world, which) for which in ("half", "both_deq", "only", "both")}


def _dead(u):
    return u.get("rir", -1) < 0 or u["rir"] == B.EMPTY


def test_half_buckets_equal_the_fp32_bucket_entries_fed_dequantised_spectra(world, launches):
    for k in ("conv", "ag", "sg"):
        a, b = launches["half"][k], launches["both_deq"][k]
        err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()
        print(f"[gpu_spec_buckets] {k}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        assert err <= AB, (k, err)
        for n, u in enumerate(world.sc["units"]):                        # the empty entry and the silent unit: exact zeros
            assert bool(a[n].any()) != _dead(u), (k, n)


def _model(w, u, quant_from_bank=True):
    """float64 overlap-save of unit u from the halves and scales the bank holds (quant_from_bank) or unquantised"""
    sc = w.sc
    out = np.zeros((2, SR))
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        b = B.bucket_of(g)
        if quant_from_bank:
            nbh = max(1, P.ceil_div(int(sc["lens"][g]), P.KB))          # (the kernel skips the blocks behind the entry's length)
            spectra = R.bank_spectra(w.q[b][g - B.FIRST[b]], w.s[b][g - B.FIRST[b]], w.perm)[:, :nbh]
            out += R.model_audiogoal(sc["srcs"][snd], None, t0, SR, spectra=spectra)
        else:
            out += R.model_audiogoal(sc["srcs"][snd], B.row_of(sc, g), t0, SR, quant=False)
    return out


def test_half_buckets_against_the_model_fed_the_banks_halves(world, launches):
    got = launches["half"]
    for n, u in enumerate(world.sc["units"]):
        if _dead(u):
            continue
        ref, oracle = _model(world, u), _model(world, u, quant_from_bank=False)
        ea = O.relerr(got["ag"][n], ref)
        es = O.relerr(got["sg"][n], O.compute_spectrogram(ref.astype(np.float32)))
        print(f"[gpu_spec_buckets] half unit {n}: vs model fed the bank's halves waveform {ea:.3e} spectrogram {es:.3e}; "
              f"vs UNQUANTISED oracle waveform {O.relerr(got['ag'][n], oracle):.3e} "
              f"spectrogram {O.relerr(got['sg'][n], O.compute_spectrogram(oracle.astype(np.float32))):.3e}")
        assert ea <= BUDGET and es <= BUDGET, (n, ea, es)


def test_only_buckets_equal_the_both_forms_bank_bit_for_bit(world, launches):
    for k in ("conv", "ag", "sg"):
        assert launches["only"][k].tobytes() == launches["both"][k].tobytes(), k
    for n, u in enumerate(world.sc["units"]):
        if _dead(u):
            assert not launches["only"]["ag"][n].any() and not launches["only"]["sg"][n].any()
            continue
        assert O.relerr(launches["only"]["ag"][n], _model(world, u, quant_from_bank=False)) <= BUDGET


def test_only_buckets_at_44100_through_the_fused_row_kernels(world):
    """rows of three partition blocks: no waveform buffer (the fused row kernels), a waveform buffer, the waveform alone"""
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, UnitRequest
    sr = 44100
    r = BatchedAudioRenderer(sr, device=DEV)
    r.add_source("a", O.synth_sources(np.random.default_rng(4), sr, k=1)[0])
    r.set_rir_bank(world.banks["both"])
    units = [UnitRequest(0, 0, g) for g in (0, 4, 5, 8, 9, B.EMPTY)] + [UnitRequest(silent=True), UnitRequest(0, 0, 3, dis_sound=0, dis_rir=7)]
    plan = r.plan(units)
    n = len(units)
    res = {}
    for which in ("only", "both"):
        bank = world.banks[which]
        sg0, ag1, sg1, ag2 = _nan(n, *r.spectrogram_shape), _nan(n, 2, sr), _nan(n, *r.spectrogram_shape), _nan(n, 2, sr)
        if which == "only":
            arr = bank.spec_c_array()
            ops.audio_obs_spec_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, None, sg0, r.n_valid, sr, flags=plan.flags)
            ops.audio_obs_spec_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag1, sg1, r.n_valid, sr, flags=plan.flags)
            ops.audio_obs_spec_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag2, None, r.n_valid, sr, flags=plan.flags)
        else:
            arr = bank.c_array(True)
            ops.audio_obs_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, None, sg0, r.n_valid, sr, flags=plan.flags)
            ops.audio_obs_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag1, sg1, r.n_valid, sr, flags=plan.flags)
            ops.audio_obs_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag2, None, r.n_valid, sr, flags=plan.flags)
        torch.cuda.synchronize()
        res[which] = [t.cpu().numpy() for t in (sg0, ag1, sg1, ag2)]
    for a, b in zip(res["only"], res["both"]):
        assert not np.isnan(a).any() and a.tobytes() == b.tobytes()
    assert res["only"][1][0].any() and not res["only"][1][5].any() and not res["only"][1][6].any()


@pytest.mark.parametrize("form", FORMS)
def test_first_bucket_launch_takes_the_loop_free_kernel(world, form):
    """every index in bucket 0 and no distractor: SS_FLAG_FIRST_BUCKET sends the launch to the loop-free kernel on bucket 0's
    arrays; the same launch without the promise runs the bucket-resolving loop kernel"""
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    r = world.r
    units = [UnitRequest(0, 0, 0), UnitRequest(1, 0, 2), UnitRequest(0, 0, B.EMPTY), UnitRequest(silent=True), UnitRequest(2, SR, 0)]
    plan = r.plan(units)
    assert plan.flags == ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET
    arr = world.banks[form].spec_c_array()
    n = len(units)
    out = {}
    for name, flags in (("loop_free", plan.flags), ("loop", ops.FLAG_NO_DISTRACTOR), ("loop_terms", 0)):
        ag, sg, conv = _nan(n, 2, SR), _nan(n, *r.spectrogram_shape), _nan(n, 2, SR)
        ops.audio_obs_spec_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag, sg, r.n_valid, SR, flags=flags)
        ops.fftconv_binaural_spec_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, conv, r.n_valid, flags=flags)
        torch.cuda.synchronize()
        out[name] = [t.cpu().numpy() for t in (ag, sg, conv)]
    for name in ("loop", "loop_terms"):
        for a, b in zip(out["loop_free"], out[name]):
            assert not np.isnan(a).any() and not np.isnan(b).any()
            assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= AB * np.abs(b).max(), name
    assert not out["loop_free"][0][2].any() and not out["loop_free"][0][3].any() and out["loop_free"][0][1].any()


def test_spec_bucket_array_refuses_mixed_forms(world):
    from ss_amd import ops
    spectra = [b.spectra for b in world.banks["half"].banks]
    scales = [b.scales for b in world.banks["half"].banks]
    with pytest.raises(ValueError):
        ops.spec_bucket_array(spectra, scales[:3] + [None], B.FIRST, B.CAPS)


# ---- AudioEngine(rir_buckets=..., rir_spectral=..., rir_spectral_buckets=True) -------------------------------------------------
def _vs_model(got_ag, got_sg, ref, label):
    """waveform and pooled spectrogram against the model's, <= 1e-4 of peak"""
    ea = O.relerr(got_ag, ref)
    es = O.relerr(got_sg, O.compute_spectrogram(ref.astype(np.float32)))
    print(f"[gpu_spec_buckets] {label}: vs model waveform {ea:.3e} spectrogram {es:.3e}")
    assert ea <= BUDGET and es <= BUDGET, (label, ea, es)


def _model_of_file(clip, wav, t0):
    """the float64 model of one unit from the RIR file's samples [L, 2], unquantised"""
    rir = np.ascontiguousarray(np.asarray(wav, np.float32).T)
    if rir.shape[1] == 0:
        return np.zeros((2, SR))
    return R.model_audiogoal(clip, rir, t0, SR, quant=False)


def _slot_of_key(eng, key):
    """global entry the bucketed store holds `key` in right now (first_b + the sub-store's slot)"""
    st = eng.store
    b = st._where[key]
    return st.first[b] + st.stores[b]._slot_of[key]


def _model_of_slot(eng, perm, clip, slot, t0):
    """the float64 model of one unit from what the store holds in global entry `slot`: fp32 spectra, or halves and scales"""
    st = eng.store
    b = st.bank.bucket_of(slot)
    sub, k, n = st.stores[b].bank, slot - st.first[b], int(st.host_len[slot])
    if n == 0:
        return np.zeros((2, SR))
    q = sub.spectra[k].cpu().numpy()
    spectra = R.bank_spectra(q, sub.scales[k].cpu().numpy(), perm) if sub.scales is not None else q[..., perm]
    return R.model_audiogoal(clip, None, t0, SR, spectra=spectra[:, :max(1, P.ceil_div(n, P.KB))])


def _check_unit(eng, perm, form, ag, sg, clip, wav, slot, t0, label):
    """only: against the unquantised model of the FILE (1e-4: staging, routing and launch in
    one).  half: against the model fed the entry's own halves and scales (1e-4), and - the entry holds THIS file - within 1e-3 of
    the unquantised model of the file (the format's loss is 2.0 - 2.6e-4 of peak; another file's RIR is ~1)"""
    exact = _model_of_file(clip, wav, t0)
    if form == "only":
        _vs_model(ag, sg, exact, label)
        return
    _vs_model(ag, sg, _model_of_slot(eng, perm, clip, slot, t0), label)
    loss = O.relerr(ag, exact)
    print(f"[gpu_spec_buckets] {label}: vs UNQUANTISED model of the file {loss:.3e}")
    assert loss <= 1e-3, (label, loss)


def _engine(form, **kw):
    from ss_amd.renderer import AudioEngine
    return AudioEngine(SR, device=DEV, rir_buckets=ENGINE_BUCKETS, rir_spectral=form, rir_spectral_buckets=True, **kw)


def _rirs(seed, lens):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray((O.synth_rir_blocks(rng, SR, L, n=1) if L > P.KB else O.synth_rir(rng, SR, length=L, n=1))[0].T)
            for L in lens]


@pytest.mark.parametrize("form", FORMS)
def test_engine_eager_and_context_routes_rebucketing_eviction_and_refusals(world, form):
    from ss_amd import _lib
    from ss_amd.renderer import UnitRequest
    srcs = world.sc["srcs"]
    eng = _engine(form)
    st = eng.store
    assert st.bank.spectral_only and st.bank.half == (form == "half")
    assert all(s.bank.data.numel() == 0 and s.bank.spectra.dtype == (torch.float16 if form == "half" else torch.float32) for s in st.stores)
    sid = [eng.source_id(f"s{i}", s) for i, s in enumerate(srcs)]          # (the 3-s clip: whole RIRs)
    lens = [9000, 16000, 3000, 20000, 40000, 12000, 33000]
    rirs = _rirs(5, lens)
    cases = [(0, 0, 0), (1, 0, 1), (2, SR, 3), (0, 0, 4)]                  # (sound, t0, rir): both buckets, the 3-s clip at 1 s
    eng.begin_batch()
    slots = [eng.rir_slot(("r", h), lambda h=h: rirs[h]) for _, _, h in cases]
    assert [st.bank.bucket_of(s) for s in slots] == [0, 0, 1, 1] and slots[2] >= 3       # global slot = first_b + local slot
    assert [eng.rir_len(s) for s in slots] == [lens[h] for _, _, h in cases]
    units = [UnitRequest(sid[a], t0, s) for (a, t0, _), s in zip(cases, slots)] + [UnitRequest(silent=True)]
    units.append(UnitRequest(sid[0], 0, slots[0], dis_sound=sid[1], dis_rir=slots[3]))   # two terms, two buckets
    out = eng.observe(units, want_audiogoal=True)
    n = len(units)
    sg2, ag2 = _nan(n, *eng.renderer.spectrogram_shape), _nan(n, 2, SR)
    cols = dict(sound=np.asarray([u.sound for u in units], np.int32), t0=np.asarray([u.t0 for u in units], np.int32),
                rir=np.asarray([-1 if u.silent else u.rir for u in units], np.int32),
                dis_sound=np.asarray([max(u.dis_sound, 0) for u in units], np.int32), dis_rir=np.asarray([u.dis_rir for u in units], np.int32))
    eng.observe_columns(cols, spectrogram_out=sg2, audiogoal_out=ag2)        # the C context (ss_ctx_set_rir_spec_buckets)
    torch.cuda.synchronize()
    for label, ag, sg in (("eager", out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()),
                          ("context", ag2.cpu().numpy(), sg2.cpu().numpy())):
        for k, (a, t0, h) in enumerate(cases):
            _check_unit(eng, world.perm, form, ag[k], sg[k], srcs[a], rirs[h], slots[k], t0, f"{form} {label} unit {k}")
        assert not ag[4].any() and not sg[4].any()
        if form == "only":
            ref = _model_of_file(srcs[0], rirs[0], 0) + _model_of_file(srcs[1], rirs[4], 0)
        else:
            ref = _model_of_slot(eng, world.perm, srcs[0], slots[0], 0) + _model_of_slot(eng, world.perm, srcs[1], slots[3], 0)
        _vs_model(ag[5], sg[5], ref, f"{form} {label} two-bucket unit")
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
    # log-mel through the context's waveform scratch: observe-then-features, bit for bit
    from ss_amd import ops
    ms, mw, _ = P.mel_filterbank_sparse(SR, 64)
    msd, mwd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV)
    lm = _nan(n, 64, 1 + SR // 160, 2)
    ctx.observe(logmel_out=lm, mel_start=msd, mel_w=mwd, mel_eps=EPS, **cols)
    ag3 = _nan(n, 2, SR)
    ctx.observe(audiogoal_out=ag3, **cols)                               # (the waveform-only launch the scratch route runs)
    want = ops.audio_features(ag3, ("logmel",), msd, mwd, mel_eps=EPS)["logmel"]
    torch.cuda.synchronize()
    assert not bool(torch.isnan(lm).any()) and torch.equal(lm, want)
    # a key whose RIR outgrows its bucket moves to the next (a live refresh with a longer response)
    grown = _rirs(6, [30000])[0]
    eng.begin_batch()
    s_new = eng.rir_slot(("r", 0), lambda: grown, refresh=True)
    assert st.bank.bucket_of(s_new) == 1 and ("r", 0) not in st.stores[0]._slot_of and eng.rir_len(s_new) == 30000
    o = eng.observe([UnitRequest(sid[2], SR, s_new)], want_audiogoal=True)
    torch.cuda.synchronize()
    _check_unit(eng, world.perm, form, o["audiogoal"][0].cpu().numpy(), o["spectrogram"][0].cpu().numpy(), srcs[2], grown, s_new, SR,
                f"{form} re-bucketed key")
    # eviction in a full bucket: bucket 1 holds 2 entries, bucket 0 holds 3
    misses = st.misses
    for h in (6, 2, 5, 1, 0):
        eng.begin_batch()
        s_h = eng.rir_slot(("e", h), lambda h=h: rirs[h])
        assert st.bank.bucket_of(s_h) == (1 if lens[h] > 16000 else 0)
        o = eng.observe([UnitRequest(sid[0], 0, s_h)], want_audiogoal=True)
        torch.cuda.synchronize()
        _check_unit(eng, world.perm, form, o["audiogoal"][0].cpu().numpy(), o["spectrogram"][0].cpu().numpy(), srcs[0], rirs[h], s_h, 0,
                    f"{form} after eviction rir {h}")
    assert st.misses == misses + 5 and len(st.stores[0]._slot_of) <= 3 and len(st.stores[1]._slot_of) <= 2 and st.grown == 0


@pytest.mark.parametrize("form", FORMS)
def test_engine_growth_of_the_last_bucket(world, form):
    """a 50000-tap RIR grows the last bucket from 3 blocks per row to 4: its old blocks (and scales) are copied bit for bit, the
    new blocks are zero, bucket 0 is not touched, and both routes render old and new entries"""
    from ss_amd.renderer import UnitRequest
    srcs = world.sc["srcs"]
    eng = _engine(form, rir_max_cap=4 * P.KB)
    st = eng.store
    sid = [eng.source_id(f"s{i}", s) for i, s in enumerate(srcs)]
    rirs = _rirs(8, [12000, 40000, 50000])
    eng.begin_batch()
    a, b = eng.rir_slot("a", lambda: rirs[0]), eng.rir_slot("b", lambda: rirs[1])
    eng.observe([UnitRequest(sid[2], SR, b), UnitRequest(sid[0], 0, a)])
    torch.cuda.synchronize()
    last = st.stores[1].bank
    old_q, old_s, p0 = last.spectra.clone(), (last.scales.clone() if form == "half" else None), st.stores[0].bank.spectra.data_ptr()
    assert last.spectra.shape[2] == 3
    c = eng.rir_slot("c", lambda: rirs[2])
    assert st.grown == 1 and st.bank.bucket_of(c) == 1 and eng.renderer.rirs is st.bank and st.stores[0].bank.spectra.data_ptr() == p0
    eng.begin_batch()
    units = [UnitRequest(sid[2], SR, b), UnitRequest(sid[0], 0, a), UnitRequest(sid[2], SR, c)]
    out = eng.observe(units, want_audiogoal=True)
    sg2, ag2 = _nan(3, *eng.renderer.spectrogram_shape), _nan(3, 2, SR)
    eng.observe_columns(dict(sound=np.asarray([u.sound for u in units], np.int32), t0=np.asarray([u.t0 for u in units], np.int32),
                             rir=np.asarray([u.rir for u in units], np.int32)), spectrogram_out=sg2, audiogoal_out=ag2)
    torch.cuda.synchronize()
    new = st.stores[1].bank
    lb = b - st.first[1]
    assert new.spectra.shape[2] == 4 and new.cap >= 50000
    assert torch.equal(new.spectra[lb, :, :3].view(torch.int16), old_q[lb].view(torch.int16))
    assert not new.spectra[lb, :, 3:].view(torch.int16).any()
    if form == "half":
        assert tuple(new.scales.shape) == (2, 2, 4) and torch.equal(new.scales[lb, :, :3], old_s[lb])
        assert bool(torch.isfinite(new.scales).all())
    for label, ag, sg in (("eager", out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()),
                          ("context", ag2.cpu().numpy(), sg2.cpu().numpy())):
        for k, (snd, h, sl, t0, what) in enumerate(((2, 1, b, SR, "old entry"), (0, 0, a, 0, "bucket 0"), (2, 2, c, SR, "the 4-block entry"))):
            _check_unit(eng, world.perm, form, ag[k], sg[k], srcs[snd], rirs[h], sl, t0, f"{form} {label} after growth, {what}")


def _pose_files(seed=3):
    """in-memory RIR files of the vector test: receivers 0-1 hear short responses, 2-3 responses of two or three blocks"""
    rng = np.random.default_rng(seed)
    sounds = {"telephone.wav": O.synth_sources(rng, SR, k=1)[0], "long.wav": O.synth_sources(rng, SR, k=1, seconds=3)[0]}
    files = {}
    for az in (0, 90, 180, 270):
        for r in range(4):
            L = int(rng.integers(900, 16001)) if r < 2 else int(rng.integers(17000, 40001))
            files[f"rirs/replica/apartment_0/{az}/{r}_7.wav"] = _rirs(int(rng.integers(1 << 30)), [L])[0]
    return sounds, files


@pytest.mark.parametrize("form", FORMS)
def test_engine_vector_observer(world, form):
    """2 in-process envs wandering over 16 poses of mixed length through the 3 + 2 entries (loads evict in both buckets)"""
    from fakes import FakeSim
    from ss_amd import sim_audio
    from test_deferred import apply, trajectory
    sounds, files = _pose_files()
    eng = _engine(form)
    eng.store.truncate_to = None                                         # whole RIRs from the first step on (a 3-s clip is in play)
    sims = [FakeSim(SR, sounds, files, False) for _ in range(2)]
    obs = sim_audio.VectorAudioObserver(eng, [sim_audio.attach(s, eng, rir_reader=files.get) for s in sims], want_audiogoal=True)
    trajs = [trajectory(rk, 6) for rk in range(2)]
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
            path = f"rirs/replica/apartment_0/{s.azimuth_angle}/{s._receiver_position_index}_{s._source_position_index}.wav"
            _check_unit(eng, world.perm, form, ag[rk], sg[rk], clip, wav, _slot_of_key(eng, path), t0, f"{form} vector step {k} env {rk}")
    st = eng.store
    assert st.misses > 5 and len(st.stores[0]._slot_of) <= 3 and len(st.stores[1]._slot_of) <= 2
    assert len(st.stores[1]._slot_of) > 0 and st.bank.spectral_only


@pytest.mark.parametrize("form", FORMS)
def test_engine_deferred_resolver_loads_files_by_probed_length(world, tmp_path, form):
    """DeferredResolver over RIR files on disk: files of 2000-16000 and 17000-40000 frames land in the bucket of their length; a
    3-s clip, so whole files are heard.  Then ``load_files`` on the store itself: the library's reader probes the frame counts
    and routes every file before it is read"""
    from scipy.io import wavfile
    from ss_amd.deferred import DeferredResolver, attach_deferred
    NS = types.SimpleNamespace
    n_nodes, n_env = 4, 2
    root = tmp_path / "rirs"
    rirs = {}
    (root / "0").mkdir(parents=True)
    for rc in range(n_nodes):
        for sc in range(n_nodes):
            rng = np.random.default_rng(7 * rc + sc)
            n = int(rng.integers(2000, 16001)) if (rc + sc) % 2 else int(rng.integers(17000, 40001))
            h = _rirs(100 + 10 * rc + sc, [n])[0]
            p = str(root / "0" / f"{rc}_{sc}.wav")
            wavfile.write(p, SR, h)
            rirs[p] = h
    clip = O.synth_sources(np.random.default_rng(5), SR, k=1, seconds=3)[0]

    class Sim:
        config = NS(AUDIO=NS(RIR_SAMPLING_RATE=SR, HAS_DISTRACTOR_SOUND=False), USE_RENDERED_OBSERVATIONS=True)
        binaural_rir_dir = str(root)
        _source_sound_dict = {"s.wav": clip}
        _current_sound, _audio_index, _episode_step_count, _duration = "s.wav", 0, 0, 500
        _receiver_position_index = _source_position_index = 0
        azimuth_angle = 0
        current_source_sound = property(lambda self: clip)
        _audio_length = 3

    sims = [Sim() for _ in range(n_env)]
    for i, sm in enumerate(sims):
        attach_deferred(sm, env_rank=i)
    eng = _engine(form)
    eng.store.truncate_to = None                                         # whole RIRs from the first step on (the clip is 3 s long)
    res = DeferredResolver(eng, prefetch_azimuths=False)                 # (a bucketed store: the resolver's per-request path)
    walk = np.random.default_rng(3)
    for step in range(5):
        for sm in sims:
            sm._receiver_position_index, sm._source_position_index = int(walk.integers(0, n_nodes)), int(walk.integers(0, n_nodes))
            sm._episode_step_count += 1
        idx = [sm._audio_index for sm in sims]
        reqs = [pickle.loads(pickle.dumps(sm.get_current_spectrogram_observation(None))) for sm in sims]
        out = res.resolve(reqs, want_audiogoal=True)
        torch.cuda.synchronize()
        ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
        for i, sm in enumerate(sims):
            p = os.path.join(str(root), "0", f"{sm._receiver_position_index}_{sm._source_position_index}.wav")
            _check_unit(eng, world.perm, form, ag[i], sg[i], clip, rirs[p], _slot_of_key(eng, p), idx[i] * SR,
                        f"{form} deferred step {step} env {i}")
    st = res.engine.store
    assert st.bank.spectral_only and st.misses >= 4
    assert len(st.stores[0]._slot_of) > 0 and len(st.stores[1]._slot_of) > 0
    for b, sub in enumerate(st.stores):                                   # every resident file sits in the bucket of its length
        for key, sl in sub._slot_of.items():
            assert (int(sub.host_len[sl]) > 16000) == (b == 1)
    # load_files: two short and two long files in one call (the library's wav reader; keys of their own)
    from ss_amd.renderer import UnitRequest
    short = [p for p, h in rirs.items() if len(h) <= 16000][:2]
    long_ = [p for p, h in rirs.items() if len(h) > 16000][:2]
    paths = [short[0], long_[0], short[1], long_[1]]
    slots = st.load_files([("f", p) for p in paths], paths)
    for p, sl in zip(paths, slots):
        b = st.bank.bucket_of(sl)
        assert b == (1 if len(rirs[p]) > 16000 else 0) and sl == st.first[b] + st.stores[b]._slot_of[("f", p)]
        assert eng.rir_len(sl) == len(rirs[p])
    sid = eng.source_id("s.wav", clip)
    out = eng.observe([UnitRequest(sid, SR, sl) for sl in slots], want_audiogoal=True)
    torch.cuda.synchronize()
    ag, sg = out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()
    for k, p in enumerate(paths):
        _check_unit(eng, world.perm, form, ag[k], sg[k], clip, rirs[p], slots[k], SR, f"{form} load_files {os.path.basename(p)}")


# ---- HBM -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_bucketed_store_allocates_spectra_scales_and_lengths_only(form):
    """per entry of bucket b: half 2 * h_blocks_b * (65 536 + 4) + 4 bytes, only 2 * h_blocks_b * 131 072 + 4: no rows"""
    from ss_amd.renderer import BucketedRirStore
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    slots, caps = [64, 16, 8], [16000, 40000, 70000]
    before = torch.cuda.memory_allocated(0)
    st = BucketedRirStore(slots, caps, DEV, spectral=form, spectral_buckets=True)
    torch.cuda.synchronize()
    delta = torch.cuda.memory_allocated(0) - before

    def granule(nbytes):                                                 # (the caching allocator's 512-byte granule)
        return -(-nbytes // 512) * 512
    want = granule(sum(slots) * 4)                                        # ONE length table over all global indices
    per_block = (65536 if form == "half" else 131072)
    formula = 0
    for n, cap in zip(slots, caps):
        hb = P.ceil_div(cap, P.KB)
        want += granule(n * 2 * hb * per_block) + (granule(n * 2 * hb * 4) if form == "half" else 0)
        formula += n * (2 * hb * (per_block + (4 if form == "half" else 0)) + 4)
    # (each sub-store also allocates - and hands back to the allocator's cache - a lengths tensor of its own before it is given
    # its view of the global one: freed blocks do not count in memory_allocated)
    assert delta == want, (delta, want)
    assert 0 <= want - formula < 512 * (2 * len(slots) + 1)               # the formula, up to allocator rounding
    assert st.bank.spectral_only and all(s.bank.data.numel() == 0 for s in st.stores)
