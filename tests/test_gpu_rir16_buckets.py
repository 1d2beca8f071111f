"""Half-precision time-domain rows in length buckets on the GPU (include/ss_hip.h "Half-precision time-domain rows in length
buckets"): k_conv<.., HALF, RBK>, ss_fftconv_binaural_rir16_buckets_f32 / ss_audio_obs_rir16_buckets_f32,
ss_ctx_set_rir16_buckets, BucketedRirStore(rows="half"), AudioEngine(rir_rows="half", rir_buckets=[...]).

  * stateless entries on the 12-unit 16 kHz scene of tests/spec_buckets_ref.py (four buckets of 1 / 2 / 3 / 5 partition blocks whose
    capacities are no multiples of a block: a stride or load bound from another bucket reads the neighbour's halves): <= 2e-6 of
    peak against ops.audio_obs_buckets_into on an fp32 BucketedRirBank of the dequantised rows (the project's A/B bound: each fp32
    path is held to <= 1e-6 of peak against float64, the inputs are identical), <= 1e-4 against the float64 model fed the bank's
    halves and scales (the project's budget), exact zeros for the empty entry and the silent unit; the SS_FLAG_FIRST_BUCKET launch
    bit-equals ops.audio_obs_rir16_into on bucket 0;
  * 44.1 kHz: three units over entries of 1, 2 and 3 blocks in three buckets, the same two bounds; through a context a
    spectrogram-only step takes the hand-over route and equals the convolution + ss_spectrogram_f32 bit for bit;
  * the engine: eager, vector, deferred and C-context routes within 1e-4 of the model, the cross-fade refusal, log-mel through the
    waveform scratch, re-bucketing, eviction, growth of the last bucket, the reported bytes."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
import spec_buckets_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = B.SR
BUDGET = 1e-4
AB = 2e-6
EPS = 1e-6
ENGINE_BUCKETS = [(3, 16000), (2, 40000)]
MODEL_UNITS = (1, 3, 4, 6, 7, 8, 9)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _unit_requests(units):
    from ss_amd.renderer import UnitRequest
    return [UnitRequest(silent=True) if u.get("rir", -1) < 0 else
            UnitRequest(u["sound"], u["t0"], u["rir"], dis_sound=u.get("dis_sound", -1), dis_rir=u.get("dis_rir", -1)) for u in units]


def _banks(rows_np, lens_np, firsts, counts):
    """per-bucket fp32 rows -> (half BucketedRirBank, fp32 BucketedRirBank of float(q) * scale, deq rows as numpy, lengths)"""
    from ss_amd import ops
    from ss_amd.renderer import BucketedRirBank, RirBank
    lengths = torch.from_numpy(np.ascontiguousarray(lens_np, np.int32)).to(DEV)
    rows = [torch.from_numpy(np.ascontiguousarray(r)).to(DEV) for r in rows_np]
    qs = [ops.rir_rows16(r) for r in rows]                                # ss_rir_rows16_f32 of every bucket
    deq = [(q.float() * s[..., None]).contiguous() for q, s in qs]        # float(q) * scale, exact in fp32
    views = [lengths[f:f + n] for f, n in zip(firsts, counts)]
    half = BucketedRirBank([RirBank(q, v, scales=s) for (q, s), v in zip(qs, views)], lengths, list(firsts))
    fp32 = BucketedRirBank([RirBank(d, v) for d, v in zip(deq, views)], lengths, list(firsts))
    torch.cuda.synchronize()
    return half, fp32, [d.cpu().numpy() for d in deq], lengths


@pytest.fixture(scope="module", autouse=True)
def _private_pool():
    """Every torch allocation of this module comes from a memory pool of the module's own and goes back to the driver with it:
    later modules of the suite hold torch.cuda.memory_allocated deltas of a store to the byte (tests/test_gpu_spec_buckets.py),
    and what this module left in the process's default pool would decide whether they pass (tests/test_gpu_obs_logmel_buckets.py)."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        import gc
        gc.collect()
        torch.cuda.synchronize()
    del pool


@pytest.fixture(scope="module")
def world(_private_pool):
    from ss_amd.renderer import BatchedAudioRenderer
    sc = B.scene()
    half, fp32, deq, lengths = _banks(sc["rows"], sc["lens"], B.FIRST, B.COUNTS)
    for b, bank in enumerate(half.banks):                                 # the device producer gives the numpy rule's bits
        q, s = R.quantise(sc["rows"][b])
        assert bank.data.cpu().numpy().tobytes() == q.tobytes() and bank.scales.cpu().numpy().tobytes() == np.asarray(s, np.float32).tobytes()
    assert half.rows_half and not half.spectral_only and not half.half and half.nbytes == sum(n * (4 * c + 8) for n, c in zip(B.COUNTS, B.CAPS))
    r = BatchedAudioRenderer(SR, device=DEV)
    for i, src in enumerate(sc["srcs"]):
        r.add_source(f"s{i}", src)
    r.set_rir_bank(half)
    plan = r.plan(_unit_requests(sc["units"]))
    assert not (plan.flags & 7)                                           # distractor terms, no cross-fade, not bucket 0 alone
    w = types.SimpleNamespace(sc=sc, half=half, fp32=fp32, deq=deq, lengths=lengths, r=r, plan=plan)
    yield w
    w.__dict__.clear()                                   # (before the pool goes: nothing of it stays allocated)


def _stateless(w, which):
    from ss_amd import ops
    r, plan = w.r, w.plan
    n = len(plan)
    conv, ag, sg, sg_only = _nan(n, 2, SR), _nan(n, 2, SR), _nan(n, *r.spectrogram_shape), _nan(n, *r.spectrogram_shape)
    if which == "half":
        arr = w.half.rir16_c_array()
        ops.fftconv_binaural_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, conv, r.n_valid, flags=plan.flags)
        ops.audio_obs_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
        ops.audio_obs_rir16_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, None, sg_only, r.n_valid, r.out_len, flags=plan.flags)
    else:
        arr = w.fp32.c_array(False)
        ops.audio_obs_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, conv, None, r.n_valid, r.out_len, flags=plan.flags)
        ops.audio_obs_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=plan.flags)
        ops.audio_obs_buckets_into(r._spec, arr, 4, w.lengths, plan.desc, None, sg_only, r.n_valid, r.out_len, flags=plan.flags)
    torch.cuda.synchronize()
    out = dict(conv=conv.cpu().numpy(), ag=ag.cpu().numpy(), sg=sg.cpu().numpy(), sg_only=sg_only.cpu().numpy())
    for k, a in out.items():
        assert not np.isnan(a).any(), (which, k)
    return out


@pytest.fixture(scope="module")
def launches(world):
    return {which: _stateless(world, which) for which in ("half", "fp32")}


def _dead(u):
    return u.get("rir", -1) < 0 or u["rir"] == B.EMPTY


def _ab(a, b, label):
    err = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()
    print(f"[gpu_rir16_buckets] {label}: max |half - fp32(dequantised)| / peak = {err:.3e}")
    assert err <= AB, (label, err)


def test_stateless_entries_equal_the_fp32_bucket_entries_fed_dequantised_rows(world, launches):
    for k in ("conv", "ag", "sg", "sg_only"):
        a = launches["half"][k]
        _ab(a, launches["fp32"][k], k)
        for n, u in enumerate(world.sc["units"]):                        # the empty entry and the silent unit: bit-exact +0
            if _dead(u):
                assert not a[n].view(np.uint32).any(), (k, n)
            else:
                assert a[n].any(), (k, n)
    assert np.array_equal(launches["half"]["conv"], launches["half"]["ag"])
    assert np.array_equal(launches["half"]["sg"], launches["half"]["sg_only"])


def _model(sc, deq, firsts, u, sr, bucket_of):
    out = np.zeros((2, sr))
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        b = bucket_of(g)
        row = deq[b][g - firsts[b]][:, :int(sc["lens"][g])]
        out += R.model_audiogoal(sc["srcs"][snd], row, t0, sr, quant=False)
    return out


def _vs_model(got_ag, got_sg, ref, label):
    ea = O.relerr(got_ag, ref)
    es = O.relerr(got_sg, R.model_spectrogram(ref)) if got_sg is not None else 0.0
    print(f"[gpu_rir16_buckets] {label}: vs float64 model fed the bank's halves: waveform {ea:.3e} spectrogram {es:.3e}")
    assert ea <= BUDGET and es <= BUDGET, (label, ea, es)


def test_stateless_entries_against_the_model_fed_the_banks_halves(world, launches):
    got = launches["half"]
    for n in MODEL_UNITS:
        ref = _model(world.sc, world.deq, B.FIRST, world.sc["units"][n], SR, B.bucket_of)
        _vs_model(got["ag"][n], got["sg"][n], ref, f"unit {n}")


def test_first_bucket_launch_bit_equals_the_single_allocation_entry_on_bucket_0(world):
    from ss_amd import ops
    from ss_amd.renderer import UnitRequest
    r = world.r
    units = [UnitRequest(0, 0, 0), UnitRequest(1, 0, 2), UnitRequest(0, 0, B.EMPTY), UnitRequest(silent=True), UnitRequest(1, 4000, 0)]
    plan = r.plan(units)
    assert plan.flags & ops.FLAG_NO_DISTRACTOR
    flags = plan.flags | ops.FLAG_FIRST_BUCKET
    n = len(units)
    b0 = world.half.banks[0]
    arr = world.half.rir16_c_array()
    ag, sg, ag1, sg1, ag2, sg2 = (_nan(n, 2, SR), _nan(n, *r.spectrogram_shape), _nan(n, 2, SR), _nan(n, *r.spectrogram_shape),
                                  _nan(n, 2, SR), _nan(n, *r.spectrogram_shape))
    ops.audio_obs_rir16_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag, sg, r.n_valid, r.out_len, flags=flags)
    ops.audio_obs_rir16_into(r._spec, b0.data, b0.scales, world.lengths, plan.desc, ag1, sg1, r.n_valid, r.out_len, flags=plan.flags)
    ops.audio_obs_rir16_buckets_into(r._spec, arr, 4, world.lengths, plan.desc, ag2, sg2, r.n_valid, r.out_len, flags=plan.flags)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ag).any()) and not bool(torch.isnan(sg).any())
    assert torch.equal(ag, ag1) and torch.equal(sg, sg1)
    _ab(ag.cpu().numpy(), ag2.cpu().numpy(), "first bucket against the bucketed loop kernel, waveform")
    _ab(sg.cpu().numpy(), sg2.cpu().numpy(), "first bucket against the bucketed loop kernel, spectrogram")
    assert not ag[2:4].cpu().numpy().view(np.uint32).any() and bool(ag[0].any())


# ---- 44.1 kHz ------------------------------------------------------------------------------------------------------------------
SR44 = 44100
CAPS44, FIRST44, COUNTS44 = [16000, 30000, 44100], [0, 1, 2], [1, 1, 1]


@pytest.fixture(scope="module")
def world44(_private_pool):
    from ss_amd.renderer import BatchedAudioRenderer
    rng = np.random.default_rng(44)
    srcs = list(O.synth_sources(rng, SR44, k=2, seconds=1))
    lens = np.asarray(CAPS44, np.int32)
    rows = []
    for cap in CAPS44:
        h = (O.synth_rir_blocks(rng, SR44, cap, n=1) if cap > P.KB else O.synth_rir(rng, SR44, length=cap, n=1))[0]
        rows.append(np.ascontiguousarray(h[None].astype(np.float32)))
    sc = dict(srcs=srcs, rows=rows, lens=lens,
              units=[dict(sound=0, t0=0, rir=0), dict(sound=1, t0=0, rir=1), dict(sound=0, t0=0, rir=2, dis_sound=1, dis_rir=1)])
    half, fp32, deq, lengths = _banks(rows, lens, FIRST44, COUNTS44)
    r = BatchedAudioRenderer(SR44, device=DEV)
    for i, src in enumerate(srcs):
        r.add_source(f"s{i}", src)
    r.set_rir_bank(half)
    plan = r.plan(_unit_requests(sc["units"]))
    w = types.SimpleNamespace(sc=sc, half=half, fp32=fp32, deq=deq, lengths=lengths, r=r, plan=plan)
    yield w
    w.__dict__.clear()


def test_44100_three_units_over_three_buckets(world44):
    from ss_amd import ops
    w, r, plan = world44, world44.r, world44.plan
    a, b = _nan(3, 2, SR44), _nan(3, 2, SR44)
    ops.fftconv_binaural_rir16_buckets_into(r._spec, w.half.rir16_c_array(), 3, w.lengths, plan.desc, a, r.n_valid, flags=plan.flags)
    ops.audio_obs_buckets_into(r._spec, w.fp32.c_array(False), 3, w.lengths, plan.desc, b, None, r.n_valid, r.out_len, flags=plan.flags)
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any()
    _ab(a, b, "44100 unfused")
    for n, u in enumerate(w.sc["units"]):
        _vs_model(a[n], None, _model(w.sc, w.deq, FIRST44, u, SR44, lambda g: g), f"44100 unit {n}")
    with pytest.raises(Exception):                                       # the fused entry serves one-block rows only
        ops.audio_obs_rir16_buckets_into(r._spec, w.half.rir16_c_array(), 3, w.lengths, plan.desc, None, _nan(3, *r.spectrogram_shape),
                                         r.n_valid, r.out_len, flags=plan.flags)


def test_44100_context_spectrogram_only_step_takes_the_hand_over_route(world44):
    from ss_amd import ops
    from ss_amd.context import AudioContext
    w, r, plan = world44, world44.r, world44.plan
    units = w.sc["units"]
    cols = dict(sound=np.asarray([u["sound"] for u in units], np.int32), t0=np.asarray([u["t0"] for u in units], np.int32),
                rir=np.asarray([u["rir"] for u in units], np.int32),
                dis_sound=np.asarray([max(u.get("dis_sound", 0), 0) for u in units], np.int32),
                dis_rir=np.asarray([u.get("dis_rir", -1) for u in units], np.int32))
    ctx = AudioContext(SR44)
    try:
        for i, src in enumerate(w.sc["srcs"]):
            ctx.add_source(f"s{i}", src)
        ctx.set_rir16_buckets(w.half)
        sg, sg2, ag2 = _nan(3, *ctx.spectrogram_shape), _nan(3, *ctx.spectrogram_shape), _nan(3, 2, SR44)
        ctx.observe(spectrogram_out=sg, **cols)                          # no waveform buffer: the context's hand-over buffer
        ctx.observe(spectrogram_out=sg2, audiogoal_out=ag2, **cols)
        conv, want = _nan(3, 2, SR44), _nan(3, *r.spectrogram_shape)
        ops.fftconv_binaural_rir16_buckets_into(r._spec, w.half.rir16_c_array(), 3, w.lengths, plan.desc, conv, r.n_valid, flags=plan.flags)
        ops.spectrogram_into(conv, want, r.pad_mode)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(sg).any())
        assert torch.equal(sg, want) and torch.equal(sg2, want) and torch.equal(ag2, conv)
    finally:
        ctx.close()


# ---- AudioEngine(rir_rows="half", rir_buckets=[...]) ------------------------------------------------------------------------------
def _engine(**kw):
    from ss_amd.renderer import AudioEngine
    return AudioEngine(SR, device=DEV, rir_rows="half", rir_buckets=ENGINE_BUCKETS, **kw)


def _rirs(seed, lens):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray((O.synth_rir_blocks(rng, SR, L, n=1) if L > P.KB else O.synth_rir(rng, SR, length=L, n=1))[0].T)
            for L in lens]


def _slot_of_key(eng, key):
    st = eng.store
    b = st._where[key]
    return st.first[b] + st.stores[b]._slot_of[key]


def _model_of_slot(eng, clip, slot, t0):
    """the float64 model of one unit from the halves and scales the store holds in global entry `slot`"""
    st = eng.store
    b = st.bank.bucket_of(slot)
    sub, k, n = st.stores[b].bank, slot - st.first[b], int(st.host_len[slot])
    if n == 0:
        return np.zeros((2, SR))
    row = (sub.data[k].float() * sub.scales[k][:, None]).cpu().numpy()[:, :n]
    return R.model_audiogoal(clip, row, t0, SR, quant=False)


def _check_unit(eng, ag, sg, clip, wav, slot, t0, label):
    """against the model fed the entry's own halves and scales (1e-4), and - the entry holds THIS file - within 1e-3 of the
    unquantised model of the file (the format's loss is 1.7-2.3e-4 of peak, include/ss_hip.h; another file's RIR is ~1)"""
    _vs_model(ag, sg, _model_of_slot(eng, clip, slot, t0), label)
    exact = R.model_audiogoal(clip, np.ascontiguousarray(np.asarray(wav, np.float32).T), t0, SR, quant=False)
    loss = O.relerr(ag, exact)
    print(f"[gpu_rir16_buckets] {label}: vs UNQUANTISED model of the file {loss:.3e}")
    assert loss <= 1e-3, (label, loss)


def _bytes_of(st):
    return sum(s.bank.data.numel() * 2 + s.bank.scales.numel() * 4 for s in st.stores)


def test_engine_eager_and_context_routes_rebucketing_eviction_and_refusals(world):
    from ss_amd import _lib, ops
    from ss_amd.renderer import UnitRequest
    srcs = world.sc["srcs"]
    eng = _engine()
    st = eng.store
    assert st.rows_half and st.bank.rows_half and not st.bank.spectral_only and not eng.rir_spectral
    assert all(s.bank.data.dtype == torch.float16 and s.bank.scales.dtype == torch.float32 and s.bank.spectra is None for s in st.stores)
    assert st.nbytes == _bytes_of(st) == sum(n * (4 * c + 8) for n, c in ENGINE_BUCKETS)        # sum of slots_b * (4 cap_b + 8)
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
    eng.observe_columns(cols, spectrogram_out=sg2, audiogoal_out=ag2)        # the C context (ss_ctx_set_rir16_buckets)
    torch.cuda.synchronize()
    for label, ag, sg in (("eager", out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()),
                          ("context", ag2.cpu().numpy(), sg2.cpu().numpy())):
        assert not np.isnan(ag).any() and not np.isnan(sg).any()
        for k, (a, t0, h) in enumerate(cases):
            _check_unit(eng, ag[k], sg[k], srcs[a], rirs[h], slots[k], t0, f"{label} unit {k}")
        assert not ag[4].any() and not sg[4].any()
        ref = _model_of_slot(eng, srcs[0], slots[0], 0) + _model_of_slot(eng, srcs[1], slots[3], 0)
        _vs_model(ag[5], sg[5], ref, f"{label} two-bucket unit")
    # a cross-faded step is refused and leaves no keys behind: the next step is correct
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
    _check_unit(eng, o["audiogoal"][0].cpu().numpy(), o["spectrogram"][0].cpu().numpy(), srcs[2], grown, s_new, SR, "re-bucketed key")
    # eviction in a full bucket (bucket 1 holds 2 entries, bucket 0 holds 3) leaves the other bucket's halves and scales untouched
    misses = st.misses
    for h in (6, 2, 5, 1, 0):
        other = st.stores[0 if lens[h] > 16000 else 1].bank
        q_before, s_before = other.data.clone(), other.scales.clone()
        eng.begin_batch()
        s_h = eng.rir_slot(("e", h), lambda h=h: rirs[h])
        assert st.bank.bucket_of(s_h) == (1 if lens[h] > 16000 else 0)
        o = eng.observe([UnitRequest(sid[0], 0, s_h)], want_audiogoal=True)
        torch.cuda.synchronize()
        assert torch.equal(other.data.view(torch.int16), q_before.view(torch.int16)) and torch.equal(other.scales, s_before)
        _check_unit(eng, o["audiogoal"][0].cpu().numpy(), o["spectrogram"][0].cpu().numpy(), srcs[0], rirs[h], s_h, 0, f"after eviction rir {h}")
    assert st.misses == misses + 5 and len(st.stores[0]._slot_of) <= 3 and len(st.stores[1]._slot_of) <= 2 and st.grown == 0


def test_engine_growth_of_the_last_bucket(world):
    """a 50000-tap RIR grows the last bucket from 40000 samples per row: its halves and scales are kept bit for bit, the new tail
    is +0, bucket 0 is not touched, and both routes render old and new entries"""
    from ss_amd.renderer import UnitRequest
    srcs = world.sc["srcs"]
    eng = _engine(rir_max_cap=4 * P.KB)
    st = eng.store
    sid = [eng.source_id(f"s{i}", s) for i, s in enumerate(srcs)]
    rirs = _rirs(8, [12000, 40000, 50000])
    eng.begin_batch()
    a, b = eng.rir_slot("a", lambda: rirs[0]), eng.rir_slot("b", lambda: rirs[1])
    eng.observe([UnitRequest(sid[2], SR, b), UnitRequest(sid[0], 0, a)])
    torch.cuda.synchronize()
    last = st.stores[1].bank
    old_q, old_s, p0 = last.data.clone(), last.scales.clone(), st.stores[0].bank.data.data_ptr()
    assert last.cap == 40000
    c = eng.rir_slot("c", lambda: rirs[2])
    assert st.grown == 1 and st.bank.bucket_of(c) == 1 and eng.renderer.rirs is st.bank and st.stores[0].bank.data.data_ptr() == p0
    eng.begin_batch()
    units = [UnitRequest(sid[2], SR, b), UnitRequest(sid[0], 0, a), UnitRequest(sid[2], SR, c)]
    out = eng.observe(units, want_audiogoal=True)
    sg2, ag2 = _nan(3, *eng.renderer.spectrogram_shape), _nan(3, 2, SR)
    eng.observe_columns(dict(sound=np.asarray([u.sound for u in units], np.int32), t0=np.asarray([u.t0 for u in units], np.int32),
                             rir=np.asarray([u.rir for u in units], np.int32)), spectrogram_out=sg2, audiogoal_out=ag2)
    torch.cuda.synchronize()
    new = st.stores[1].bank
    lb = b - st.first[1]
    assert new.cap >= 50000 and new.cap <= 4 * P.KB and new.data.dtype == torch.float16
    assert torch.equal(new.data[lb, :, :40000].view(torch.int16), old_q[lb].view(torch.int16))
    assert not new.data[lb, :, 40000:].view(torch.int16).any()           # the new tail: +0
    assert torch.equal(new.scales[lb], old_s[lb]) and bool(torch.isfinite(new.scales).all())
    assert st.nbytes == _bytes_of(st) == 3 * (4 * 16000 + 8) + 2 * (4 * new.cap + 8)
    for label, ag, sg in (("eager", out["audiogoal"].cpu().numpy(), out["spectrogram"].cpu().numpy()),
                          ("context", ag2.cpu().numpy(), sg2.cpu().numpy())):
        for k, (snd, h, sl, t0, what) in enumerate(((2, 1, b, SR, "old entry"), (0, 0, a, 0, "bucket 0"), (2, 2, c, SR, "the grown entry"))):
            _check_unit(eng, ag[k], sg[k], srcs[snd], rirs[h], sl, t0, f"{label} after growth, {what}")


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


def test_engine_vector_observer():
    """2 in-process envs wandering over 16 poses of mixed length through the 3 + 2 entries (loads evict in both buckets)"""
    from fakes import FakeSim
    from ss_amd import sim_audio
    from test_deferred import apply, trajectory
    sounds, files = _pose_files()
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
            _check_unit(eng, ag[rk], sg[rk], clip, files[path], _slot_of_key(eng, path), t0, f"vector step {k} env {rk}")
    st = eng.store
    assert st.misses > 3 and len(st.stores[0]._slot_of) <= 3 and len(st.stores[1]._slot_of) <= 2 and st.bank.rows_half


def test_engine_deferred_resolver_loads_files_by_probed_length(tmp_path):
    """DeferredResolver over RIR files on disk: files of 2000-16000 and 17000-40000 frames land in the bucket of their length; a
    3-s clip, so whole files are heard"""
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
    eng = _engine()
    eng.store.truncate_to = None                                         # whole RIRs from the first step on (the clip is 3 s long)
    res = DeferredResolver(eng, prefetch_azimuths=False)                 # (a bucketed store: the resolver's per-request path)
    walk = np.random.default_rng(3)
    for step in range(4):
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
            _check_unit(eng, ag[i], sg[i], clip, rirs[p], _slot_of_key(eng, p), idx[i] * SR, f"deferred step {step} env {i}")
    st = res.engine.store
    assert st.bank.rows_half and st.misses >= 3
    for b, sub in enumerate(st.stores):                                   # every resident file sits in the bucket of its length
        for key, sl in sub._slot_of.items():
            assert (int(sub.host_len[sl]) > 16000) == (b == 1)


def test_bucketed_store_allocates_halves_scales_and_lengths_only():
    """per entry of bucket b: 4 * cap_b + 8 bytes, plus one length word over all global indices"""
    from ss_amd.renderer import BucketedRirStore
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    # (every tensor is at most 1 MiB and a multiple of 512 B: such requests are cut to size by the caching allocator, whatever
    #  earlier tests left in its cache)
    slots, caps = [128, 64, 64], [2000, 3968, 4032]
    before = torch.cuda.memory_allocated(0)
    st = BucketedRirStore(slots, caps, DEV, rows="half")
    torch.cuda.synchronize()
    delta = torch.cuda.memory_allocated(0) - before
    formula = sum(n * (4 * c + 8) for n, c in zip(slots, caps))
    assert st.nbytes == formula
    assert delta == formula + 512 * -(-sum(slots) * 4 // 512), (delta, formula)
