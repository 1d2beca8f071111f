"""Parity with RIRs whose every partition block is audible (oracle.synth_rir_blocks).

The other parity tests draw decaying RIRs (synth_rir): past the first one or two 16384-tap partition blocks the RIR is
below the 1e-4-of-peak tolerance, so a kernel could skip, repeat or misplace a later block unnoticed.  Here every block of
every RIR reaches 1e-2 of the peak of some unit, and every block-edge tap 1e-3, and each test proves that about its own
inputs through tests/rir_guard.py before it compares.  The host-build tests pin each kernel (k_conv, k_conv_spec,
k_obs_rows, k_obs_blocks, split rows, the bucketed bank); the GPU tests go through the product entry points."""
import numpy as np
import pytest

import rir_guard as G
from oracle import ss_oracle as O
from ss_amd import planning as P

TOL = 1e-4
_RIRS = {}


def check(got, ref, tol=TOL):
    got = np.asarray(got)
    assert not np.isnan(got).any()
    assert O.relerr(got, ref) <= tol, O.relerr(got, ref)


def check_unit(ag, sg, ref):
    check(ag, ref)
    check(sg, O.compute_spectrogram(ref.astype(np.float32)))


def rir(sr, L, seed):
    """synth_rir_blocks RIR in wav layout [L, 2], memoised (the guard caches by content, the draw is the slow part)."""
    key = (sr, L, seed)
    if key not in _RIRS:
        _RIRS[key] = G.wav(O.synth_rir_blocks(np.random.default_rng(seed), sr, L)[0])
    return _RIRS[key]


def source(sr, seconds, seed):
    return O.synth_sources(np.random.default_rng(1000 + seed), sr, k=1, seconds=seconds)[0]


def bank_of(rirs, cap=None):
    cap = cap or max(h.shape[0] for h in rirs)
    cap += cap & 1
    b = np.zeros((len(rirs), 2, cap), np.float32)
    for i, h in enumerate(rirs):
        b[i, :, :h.shape[0]] = h.T
    return b


def steady_t0(src, sr):
    """SS1.0 multi-second clip, last audio index: the steady branch (index * sr >= RIR length) reads the longest past."""
    return P.window_start_sim(len(src), sr, len(src) // sr - 1)


# ---- host build ---------------------------------------------------------------------------------------------------
hs = None


def _hs():
    global hs
    if hs is None:
        hs = pytest.importorskip("hostsim.hs")
    return hs


def _sim_case(sr, L, seconds, dis_L, seed):
    """Sources, RIRs and units of one multi-block case: unit 0 alone, unit 1 with a distractor whose RIR has several
    blocks (term 1 read at a steady window of its own clip), unit 2 silent.  Returns (srcs, rirs, units, guard refs)."""
    srcs = [source(sr, seconds, seed), source(sr, max(2, -(-dis_L // sr) + 1), seed + 1)]
    rirs = [rir(sr, L, seed), rir(sr, dis_L, seed + 1)]
    t0, dt0 = steady_t0(srcs[0], sr), steady_t0(srcs[1], sr)
    units = [dict(sound=0, t0=t0, rir=0), dict(sound=0, t0=t0, rir=0, dis_sound=1, dis_t0=dt0, dis_rir=1), dict(rir=-1)]
    main = G.Term(srcs[0], rirs[0], t0=t0, out_len=sr, name=f"main {L}")
    dis = G.Term(srcs[1], rirs[1], t0=dt0, out_len=sr, name=f"distractor {dis_L}")
    refs = G.check([main, [main, dis]])
    return srcs, rirs, units, refs


def _check_sim_units(a, sg, refs):
    for n, ref in enumerate(refs):
        check_unit(a[n], sg[n], ref)
    assert not a[2].any() and not sg[2].any()                                      # silent unit: exact zeros


@pytest.mark.parametrize("L", [16385, 32768, 40001, 64000, 262144])
def test_loop_kernel_and_spectral_bank_every_block_16k(L):
    """k_conv (loop kernel, fused) and k_conv_spec at 16 kHz, multi-second clip in the steady branch (a 17-s clip for the
    16-block RIR: the window has to reach back over all of it); the distractor's RIR has several blocks too."""
    h = _hs()
    sr = 16000
    seconds = max(5, -(-L // sr) + 1)
    srcs, rirs, units, refs = _sim_case(sr, L, seconds, 40001, seed=L)
    bank, lens = bank_of(rirs), [r.shape[0] for r in rirs]
    a_t, s_t = h.run(srcs, bank, lens, units, sr, sr, fuse=True, simple=False)
    _check_sim_units(a_t, s_t, refs)
    a_s, s_s = h.run(srcs, bank, lens, units, sr, sr, fuse=True, spectral=True)
    _check_sim_units(a_s, s_s, refs)
    assert np.abs(a_s - a_t).max() <= 2e-6 * np.abs(a_t).max()                     # the two bank forms agree


_ROWS_44K = {44100: 1, 66150: 3, 176400: 5, 262144: 7}                            # RIR length -> clip seconds


@pytest.mark.parametrize("L", sorted(_ROWS_44K))
def test_obs_rows_every_block_44k(L):
    """k_obs_rows at 44.1 kHz (one and three persistent workgroups, stash on and off, spectral bank): 1-s clip for the
    one-second RIR, multi-second clips in the steady branch beyond it.  The 16-block RIR (store cap, kRowsMaxNbh) with a
    16-block distractor sets pair-mask bits 15 and 31."""
    h = _hs()
    sr = 44100
    dis_L = 262144 if L == 262144 else 66150
    srcs, rirs, units, refs = _sim_case(sr, L, _ROWS_44K[L], dis_L, seed=L + 1)
    bank, lens = bank_of(rirs), [r.shape[0] for r in rirs]
    for kw in (dict(row_wgs=1), dict(row_wgs=3, row_stash=True), dict(row_wgs=3, spectral=True)):
        a, sg = h.run(srcs, bank, lens, units, sr, sr, **kw)
        _check_sim_units(a, sg, refs)


@pytest.mark.parametrize("len_prev,sample_index", [(176400, 215000), (66150, 125000)])
def test_obs_rows_crossfade_previous_rir_of_several_blocks_44k(len_prev, sample_index):
    """SS_FLAG_CROSSFADE in k_obs_rows (continuous_simulator.py:47-53, 413-426): the previous step's RIR has 11 / 5 blocks
    and is blended over the first 0.05 s; 0.25-s steps that wrap around the clip end (steady branch)."""
    h = _hs()
    sr = 44100
    src = source(sr, 5 if len_prev > sr * 3 else 3, len_prev)
    cur, prev = rir(sr, 44100, 7), rir(sr, len_prev, len_prev + 7)
    ns = sr // 4
    assert sample_index + ns > len(src) and sample_index >= len_prev
    w1, w2 = G.crossfade_weights(sr)
    terms = [G.Term(src, prev, "cont", sr=sr, sample_index=sample_index, weight=w1, name="previous"),
             G.Term(src, cur, "cont", sr=sr, sample_index=sample_index, weight=w2, name="current")]
    ref, ref_cur = G.check([terms, G.Term(src, cur, "cont", sr=sr, sample_index=sample_index)])
    bank, lens = bank_of([cur, prev]), [cur.shape[0], prev.shape[0]]
    units = [dict(sound=0, t0=sample_index, rir=0, wrap=True, last_rir=1, last_wrap=True),
             dict(sound=0, t0=sample_index, rir=0, wrap=True)]
    a, sg = h.run([src], bank, lens, units, ns, sr, row_wgs=3, crossfade=True)
    check_unit(a[0], sg[0], ref)
    check_unit(a[1], sg[1], ref_cur)
    assert np.abs(ref - O.compute_audiogoal_continuous(src, cur, sr, sample_index, 0.25, last_rir=prev,
                                                       use_crossfade=True)).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("route", [dict(row_blocks=True, parts_log2=0), dict(row_blocks=True, parts_log2=2),
                                   dict(parts_log2=1), dict(parts_log2=3)], ids=["blocks-p0", "blocks-p2", "split-p1", "split-p3"])
@pytest.mark.parametrize("spectral", [False, True])
def test_obs_blocks_and_split_rows_every_block_44k(route, spectral):
    """k_obs_blocks (one workgroup per output block) and the split rows (2^k workgroups per row) at 44.1 kHz with a 5-block
    RIR and a 5-block distractor, 3-s clip in the steady branch."""
    h = _hs()
    sr = 44100
    srcs, rirs, units, refs = _sim_case(sr, 66150, 3, 66150, seed=3)
    bank, lens = bank_of(rirs), [r.shape[0] for r in rirs]
    a, sg = h.run(srcs, bank, lens, units, sr, sr, fuse=True, row_wgs=64, spectral=spectral, **route)
    _check_sim_units(a, sg, refs)


@pytest.mark.parametrize("sr,kw", [(16000, dict(fuse=True, simple=False)), (44100, dict(row_wgs=3))], ids=["16k-loop", "44k-rows"])
def test_bucketed_bank_one_block_and_eleven_block_rirs_in_one_launch(sr, kw):
    """Length-bucketed bank: one-block RIRs in bucket 0, 11-block RIRs in bucket 1, mixed in one launch (a distractor from
    the other bucket), against the guarded oracle."""
    h = _hs()
    long_L = 11 * P.KB - 1000
    seconds = -(-long_L // sr) + 1
    s_long, s_1 = source(sr, seconds, 11), source(sr, 1, 12)
    short = [rir(sr, 9000, 21), rir(sr, min(P.KB, sr - 1), 22)]    # (a 1-s clip from its start reads taps < sr only)
    long_ = [rir(sr, long_L, 23), rir(sr, long_L - 777, 24)]
    t0 = steady_t0(s_long, sr)
    b0, b1 = bank_of(short), bank_of(long_)
    lens = [r.shape[0] for r in short + long_]
    units = [dict(sound=1, t0=0, rir=0), dict(sound=0, t0=t0, rir=2), dict(rir=-1),
             dict(sound=0, t0=t0, rir=3, dis_sound=1, dis_t0=0, dis_rir=1),
             dict(sound=1, t0=0, rir=1, dis_sound=0, dis_t0=t0, dis_rir=2)]
    T = lambda s, hh, t: G.Term(s, hh, t0=t, out_len=sr)
    refs = G.check([T(s_1, short[0], 0), T(s_long, long_[0], t0), [T(s_long, long_[1], t0), T(s_1, short[1], 0)],
                    [T(s_1, short[1], 0), T(s_long, long_[0], t0)]])
    a, sg = h.run([s_long, s_1], b0, lens, units, sr, sr, bucket2=b1, **kw)
    for n, ref in zip((0, 1, 3, 4), refs):
        check_unit(a[n], sg[n], ref)
    assert not a[2].any() and not sg[2].any()


# ---- stale rows: what the store-lifecycle tests below could miss -----------------------------------------------------
_LIFE_SR = 16000
_LIFE_LENS = (64000, 20000, 40001)                      # long, short, long again: one slot, three occupants


def _life_inputs(tmp_path=None):
    """int16 wav files of three synth_rir_blocks RIRs and what the store holds after reading them (scipy's integer values:
    the reference convolves them as they are, simulator.py:615-618), a 5-s clip and its steady window."""
    sr = _LIFE_SR
    src = source(sr, 5, 77)
    rirs, paths = [], []
    for i, L in enumerate(_LIFE_LENS):
        q = np.round(rir(sr, L, 80 + i) * 60000).astype(np.int16)
        rirs.append(q.astype(np.float32))
        if tmp_path is not None:
            from scipy.io import wavfile
            paths.append(str(tmp_path / f"rir{i}.wav"))
            wavfile.write(paths[-1], sr, q)
    return src, steady_t0(src, sr), rirs, paths


def _life_refs(src, t0, rirs):
    sr = _LIFE_SR
    return G.check([G.Term(src, h, t0=t0, out_len=sr, name=f"occupant {i}") for i, h in enumerate(rirs)])


def test_store_lifecycle_inputs_would_show_a_stale_row():
    """The GPU lifecycle tests put a short RIR into a slot that held a long one.  A row (or block spectrum) left stale past
    the short RIR's length would hold the long occupant's taps there: the oracle of that RIR must differ from the true one
    by at least 1e-2 of peak, and the guard must accept the true RIRs."""
    src, t0, rirs, _ = _life_inputs()
    refs = _life_refs(src, t0, rirs)
    for prev, short in ((0, 1), (2, 1)):
        n = rirs[short].shape[0]
        stale = rirs[prev].copy()
        stale[:n] = rirs[short]
        got = G.Term(src, stale, t0=t0, out_len=_LIFE_SR).blocks()[1]
        assert np.abs(got - refs[short]).max() >= 1e-2 * np.abs(refs[short]).max()
    # and a long occupant after the short one: the taps past the short length are the new ones, a row cut at the old
    # length (lengths not updated) would lose them
    cut = rirs[2].copy()
    cut[rirs[1].shape[0]:] = 0
    got = G.Term(src, cut, t0=t0, out_len=_LIFE_SR).blocks()[1]
    assert np.abs(got - refs[2]).max() >= 1e-2 * np.abs(refs[2]).max()


# ---- GPU: the product entry points ----------------------------------------------------------------------------------
DEV = "cuda:0"


def _renderer(sr, srcs, rirs, **kw):
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    r = BatchedAudioRenderer(sr, device=DEV, **kw)
    for i, s in enumerate(srcs):
        r.add_source(f"s{i}", s)
    r.set_rir_bank(RirBank.from_arrays(rirs, DEV))
    return r


# (RIR length, clip seconds) per rate: every combination renders its window in the steady branch (or a 1-s clip from its
# start when the RIR fits the clip's first second: 44100 taps at 44.1 kHz)
_GPU_COMBOS = {44100: [(44100, 1), (66150, 3), (176400, 5)], 16000: [(64000, 5), (40001, 5), (16385, 5), (262144, 18)]}


@pytest.mark.gpu
@pytest.mark.parametrize("sr,n_units", [(44100, 1), (44100, 5), (44100, 10), (44100, 64), (44100, 512), (16000, 1), (16000, 128)])
def test_gpu_renderer_every_block_both_bank_forms(sr, n_units):
    """BatchedAudioRenderer + RirBank and the context API (ss_ctx_observe), time-domain and spectral bank, at the launcher's
    own choice of kernel: at 44.1 kHz 1 / 5 / 10 units take k_obs_blocks and the split rows, 64 / 512 units k_obs_rows; at
    16 kHz multi-second clips through the loop kernels.  Every fourth unit carries a distractor (a 1-s clip convolved from its start), one unit in 7 is silent."""
    import torch
    from ss_amd.context import AudioContext
    from ss_amd.renderer import UnitRequest
    combos = _GPU_COMBOS[sr]
    srcs = [source(sr, sec, 200 + i) for i, (_, sec) in enumerate(combos)] + [source(sr, 1, 299)]
    rirs = [rir(sr, L, 300 + i) for i, (L, _) in enumerate(combos)]
    dis_rir = rir(sr, min(sr - 1, 44100), 399)                  # (only taps < sr reach a distractor's first second)
    rirs.append(dis_rir)
    nd = len(combos)
    units, terms = [], []
    for n in range(n_units):
        if n % 7 == 6:
            units.append(UnitRequest(silent=True))
            terms.append(None)
            continue
        c = n % nd if n_units > 1 else 1 + (sr == 16000)         # (one unit: a multi-block steady window)
        t0 = steady_t0(srcs[c], sr)
        term = G.Term(srcs[c], rirs[c], t0=t0, out_len=sr)
        if n % 4 == 3:
            units.append(UnitRequest(c, t0, c, dis_sound=nd, dis_rir=nd))
            terms.append([term, G.Term(srcs[nd], dis_rir, t0=0, out_len=sr)])
        else:
            units.append(UnitRequest(c, t0, c))
            terms.append(term)
    live = [t for t in terms if t is not None]
    refs = iter(G.check(live))
    refs = [None if t is None else next(refs) for t in terms]
    r = _renderer(sr, srcs, rirs)
    ctx = AudioContext(sr)                                      # the same steps through ss_ctx_observe
    for i, s in enumerate(srcs):
        ctx.add_source(f"s{i}", s)
    ctx.set_rir_bank(r.rirs.data, r.rirs.lengths)
    for spectral in (False, True):
        if spectral:
            r.rirs.build_spectra()
            ctx.set_rir_spectra(r.rirs.spectra)
        ag, sg = r.render(r.plan(units), want_audiogoal=True)
        ag2, sg2 = torch.empty_like(ag), torch.empty_like(sg)
        ctx.observe([u.sound for u in units], [u.t0 for u in units], [u.rir for u in units], spectrogram_out=sg2,
                    audiogoal_out=ag2, dis_sound=[u.dis_sound for u in units], dis_rir=[u.dis_rir for u in units])
        torch.cuda.synchronize()
        for ag, sg in ((ag, sg), (ag2, sg2)):
            ag, sg = ag.cpu().numpy(), sg.cpu().numpy()
            for n, ref in enumerate(refs):
                if ref is None:
                    assert not ag[n].any() and not sg[n].any()
                else:
                    check_unit(ag[n], sg[n], ref)


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [16000, 44100])
def test_gpu_ss2_steps_wrap_and_crossfade(sr):
    """SoundSpaces 2.0 0.25-s steps (BatchedAudioRenderer(step_time=0.25, wrap=True)) with RIRs of several blocks: steady
    windows that wrap around the clip end, an early-branch window, and cross-fades whose previous RIR has several blocks."""
    import torch
    from ss_amd.renderer import UnitRequest
    src = source(sr, 5, 500)
    S = len(src)
    rirs = [rir(sr, L, 510 + i) for i, L in enumerate((64000, 40001, 2 * P.KB + 5))]
    w1, w2 = G.crossfade_weights(sr)
    cases = [(S - sr // 8, 0, -1), (S - 100, 1, 0), (S // 2 + 7, 2, 1), (S - sr // 10, 2, 0), (20000, 0, 1)]   # (last: early)
    units, terms, plain = [], [], []
    for si, h, last in cases:
        steady = si >= rirs[h].shape[0]
        cur = G.Term(src, rirs[h], "cont", sr=sr, sample_index=si)
        if last < 0:
            units.append(UnitRequest(0, P.window_start_continuous(si), h, wrap=None if steady else False))
            terms.append(cur)
            continue
        lw = si >= rirs[last].shape[0]
        units.append(UnitRequest(0, P.window_start_continuous(si), h, wrap=None if steady else False, last_rir=last,
                                 last_wrap=None if lw else False))
        terms.append([G.Term(src, rirs[last], "cont", sr=sr, sample_index=si, weight=w1),
                      G.Term(src, rirs[h], "cont", sr=sr, sample_index=si, weight=w2)])
    refs = G.check(terms)
    for (si, h, last), ref in zip(cases, refs):                # the guard's sums are the reference's crossfade()
        want = O.compute_audiogoal_continuous(src.astype(np.float64), rirs[h].astype(np.float64), sr, si, 0.25,
                                              last_rir=None if last < 0 else rirs[last].astype(np.float64),
                                              use_crossfade=last >= 0)
        assert np.abs(ref - want).max() <= 1e-9 * np.abs(want).max()
    r = _renderer(sr, [src], rirs, step_time=0.25, wrap=True)
    ag, sg = r.render_crossfaded(units)
    torch.cuda.synchronize()
    ag, sg = ag.cpu().numpy(), sg.cpu().numpy()
    for n, ref in enumerate(refs):
        check_unit(ag[n], sg[n], ref)
        assert not ag[n][:, sr // 4:].any()


def _engine_render(eng, src_id, t0, slot):
    import torch
    from ss_amd.renderer import UnitRequest
    out = eng.observe([UnitRequest(src_id, t0, slot)], want_audiogoal=True)
    torch.cuda.synchronize()
    return out["audiogoal"][0].cpu().numpy(), out["spectrogram"][0].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["load_files", "upload_rows", "spectral"])
def test_gpu_store_slot_long_short_long(path, tmp_path):
    """One store slot holds a 4-block RIR, then a 2-block one, then a 3-block one (int16 wav files read by load_files and
    scattered on the device; rows uploaded from the host by upload_rows; the spectral store's block spectra rebuilt by
    sync_spectra).  A single-slot store evicts on every load.  Each render equals its own oracle: no stale taps or block
    spectra of the previous occupant, no row cut at its length (test_store_lifecycle_inputs_would_show_a_stale_row proves
    these inputs would show either)."""
    from ss_amd.renderer import AudioEngine
    sr = _LIFE_SR
    src, t0, rirs, paths = _life_inputs(tmp_path)
    refs = _life_refs(src, t0, rirs)
    eng = AudioEngine(sr, device=DEV, rir_slots=1, rir_spectral=path == "spectral")
    sid = eng.source_id("clip", src)                           # a 5-s clip: whole rows from here on
    store = eng.store
    for i, (h, ref) in enumerate(zip(rirs, refs)):
        if path == "upload_rows":
            slot = 0
            store.upload_rows([slot], [np.ascontiguousarray(h)])
        else:
            slot = store.load_files([f"k{i}"], [paths[i]])[0]
            assert len(store._slot_of) == 1
        assert slot == 0 and int(store.host_len[0]) == h.shape[0]
        ag, sg = _engine_render(eng, sid, t0, slot)
        check_unit(ag, sg, ref)
    if path == "spectral":
        assert store.bank.spectra is not None


@pytest.mark.gpu
@pytest.mark.parametrize("sr,spectral", [(16000, False), (16000, True), (44100, False), (44100, True)])
def test_gpu_bucketed_bank_one_block_and_eleven_block_rirs(sr, spectral):
    """BucketedRirBank (renderer) with one-block RIRs in the short bucket and 11-block RIRs in the long one, mixed in one
    launch (a distractor from the short bucket, a silent unit), both bank forms, against the guarded oracle."""
    import torch
    from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, UnitRequest
    long_L = 11 * P.KB - 1000
    s_long, s_1 = source(sr, -(-long_L // sr) + 1, 601), source(sr, 1, 602)
    rirs = [rir(sr, 9000, 611), rir(sr, long_L, 612), rir(sr, min(P.KB, sr - 1), 613), rir(sr, long_L - 777, 614)]
    bank = BucketedRirBank.from_arrays(rirs, DEV, caps=[P.KB, long_L])
    ix = bank.index_of
    if spectral:
        bank.build_spectra()
    r = BatchedAudioRenderer(sr, device=DEV)
    r.add_source("long", s_long)
    r.add_source("one", s_1)
    r.set_rir_bank(bank)
    t0 = steady_t0(s_long, sr)
    units = [UnitRequest(1, 0, ix[0]), UnitRequest(0, t0, ix[1]), UnitRequest(silent=True),
             UnitRequest(0, t0, ix[3], dis_sound=1, dis_rir=ix[2]), UnitRequest(1, 0, ix[2])]
    T = lambda s, h, t: G.Term(s, h, t0=t, out_len=sr)
    refs = G.check([T(s_1, rirs[0], 0), T(s_long, rirs[1], t0), [T(s_long, rirs[3], t0), T(s_1, rirs[2], 0)],
                    T(s_1, rirs[2], 0)])
    ag, sg = r.render(r.plan(units), want_audiogoal=True)
    torch.cuda.synchronize()
    ag, sg = ag.cpu().numpy(), sg.cpu().numpy()
    for n, ref in zip((0, 1, 3, 4), refs):
        check_unit(ag[n], sg[n], ref)
    assert not ag[2].any() and not sg[2].any()
