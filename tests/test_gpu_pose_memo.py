"""The pose memo on the GPU: k_memo_rows through ``ss_memo_rows_f32`` (a) and the native column path
``FastVectorAudioObserver(pose_cache=True, native_pose_cache=True)`` against ``pose_cache=True`` alone (b).

(a) Row sizes 5 / 3380 / 8970 / 32000 / 88200 floats and bases 4 and 8 bytes off 16-byte alignment, the move list once in device
    memory and once in pinned host memory: bit-exact against ``index_select`` / ``index_copy_``, and the words around the
    arrays and in the rows that are not named - distinct NaN payloads - come back untouched.
(b) Twin states, twin contexts over one RIR store, a 12-step script for 4 envs (stand still, leave and come back, silence after
    the duration, a sound change, a scene change; a 3-s and a 1-s sound), pools that start at 2 rows so that they grow.  Both
    paths run the same render kernels on the same units and the rest is copies: spectrogram and audiogoal are equal BIT FOR
    BIT at every step (tolerance zero by construction), and so are ``_audio_index`` and the hit / miss counts.  16 kHz with
    both outputs, 44.1 kHz with the spectrogram only (8970-float rows: the 8-byte path), and 16 kHz under ``set_overlap(2)``
    with no join between the steps and one ``join()`` before the comparison."""
import numpy as np
import pytest
import torch

from oracle import ss_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """The guarded arrays of (a) are odd-sized blocks of up to 18 MB; left in the caching allocator they would be handed, whole,
    to later tests that account for ``torch.cuda.memory_allocated`` to the byte (tests/test_gpu_spec_buckets.py)."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- (a) the kernel ---------------------------------------------------------------------------------------------------
def _guarded(rows, rf, off_floats, seed):
    """-> (backing int32 tensor, float32 view [rows, rf] starting GUARD + off_floats words in)"""
    n = rows * rf + 2 * GUARD + 8
    back = (torch.arange(n, dtype=torch.int64) * 2654435761 + seed) % (1 << 22)
    back = (back + 0x7fc00000).to(torch.int32).to(DEV)                      # quiet NaNs with distinct payloads
    lo = GUARD + off_floats
    view = back[lo:lo + rows * rf].view(torch.float32).view(rows, rf)
    assert view.data_ptr() % 16 == 4 * off_floats % 16
    return back, view, lo


def _check(pairs, moves_host, n_store, n_fetch, pinned):
    from ss_amd import ops
    moves = moves_host.pin_memory() if pinned else moves_host.to(DEV)
    st, ft = moves_host[:n_store].long().to(DEV), moves_host[n_store:n_store + n_fetch].long().to(DEV)
    expect = []
    for (ob, o, olo), (pb, p, plo) in pairs:
        eo, ep = ob.clone(), pb.clone()
        ov = eo[olo:olo + o.numel()].view(o.shape)
        pv = ep[plo:plo + p.numel()].view(p.shape)
        src_o, src_p = ov.clone(), pv.clone()
        pv.index_copy_(0, st[:, 1], src_o.index_select(0, st[:, 0]))
        ov.index_copy_(0, ft[:, 0], src_p.index_select(0, ft[:, 1]))
        expect.append((eo, ep))
    ops.memo_rows_([(o, p) for (_, o, _), (_, p, _) in pairs], moves, n_store, n_fetch)
    torch.cuda.synchronize()
    for ((ob, _, _), (pb, _, _)), (eo, ep) in zip(pairs, expect):
        assert torch.equal(ob, eo) and torch.equal(pb, ep)


def _moves(n_store, n_fetch, rows, slots, seed):
    g = torch.Generator().manual_seed(seed)
    n = n_store + n_fetch
    return torch.stack([torch.randperm(rows, generator=g)[:n], torch.randperm(slots, generator=g)[:n]], 1).to(torch.int32).contiguous()


@pytest.mark.parametrize("pinned", [False, True], ids=["moves-on-device", "moves-pinned"])
@pytest.mark.parametrize("rfs", [(5,), (3380,), (8970,), (32000,), (88200,), (3380, 32000), (8970, 88200)], ids=str)
def test_memo_rows_bit_exact_and_guards_hold(rfs, pinned):
    rows, slots = 40, 50
    for n_store, n_fetch in ((1, 0), (0, 1), (37, 0), (0, 37), (19, 18)):
        pairs = [(_guarded(rows, rf, 0, 1 + k), _guarded(slots, rf, 0, 11 + k)) for k, rf in enumerate(rfs)]
        _check(pairs, _moves(n_store, n_fetch, rows, slots, sum(rfs) + n_store), n_store, n_fetch, pinned)


@pytest.mark.parametrize("offs", [(1, 1), (2, 2), (0, 1), (2, 0)], ids=lambda o: f"out+{4 * o[0]}B-pool+{4 * o[1]}B")
def test_memo_rows_off_16_byte_alignment(offs):
    for rf in (3380, 8970):
        pairs = [(_guarded(40, rf, offs[0], 3), _guarded(50, rf, offs[1], 4))]
        _check(pairs, _moves(19, 18, 40, 50, rf), 19, 18, False)


def test_memo_rows_more_moves_than_one_argument_table():
    """600 moves: the stateless entry reads them through the pointer in one launch"""
    pairs = [(_guarded(700, 132, 0, 5), _guarded(800, 132, 0, 6))]
    _check(pairs, _moves(300, 300, 700, 800, 9), 300, 300, True)


# ---- (b) the native column path against the Python pose cache ---------------------------------------------------------
N_ENV, STEPS, NODES = 4, 12, 4


def _script():
    """(recv, rot, step_count, sound, scene) per step and env; duration 6: step counts above it are silent"""
    rng = np.random.default_rng(5)
    recv, rot = np.array([1, 2, 0, 3]), np.array([90, 0, 180, 270])
    sound, scene = np.array([0, 0, 1, 0]), np.array([0, 1, 0, 1])
    out = []
    for t in range(STEPS):
        cnt = np.full(N_ENV, t)
        if t in (2, 4, 7, 10):                                               # leave ...
            move = rng.uniform(size=N_ENV) < 0.7
            recv = np.where(move, rng.integers(0, NODES, N_ENV), recv)
            rot = np.where(move, rng.integers(0, 4, N_ENV) * 90, rot)
        if t in (3, 8):                                                      # ... and come back: the first window returns
            recv, rot = np.array([1, 2, 0, 3]), np.array([90, 0, 180, 270])
        if t == 6:
            sound = np.array([1, 0, 1, 0])                                   # env 0 changes its sound: its map is dropped
        if t == 9:
            scene = np.array([0, 0, 0, 1])                                   # env 1 changes its scene
            cnt = np.array([t, 0, t, t])                                     # ... in a new episode: it sounds again
        out.append((recv.copy(), rot.copy(), cnt, sound.copy(), scene.copy()))
    return out


def _world(sr):
    from ss_amd.renderer import RirStore
    from ss_amd.vector import RirIndex
    rng = np.random.default_rng(21)
    clips = [O.synth_sources(rng, sr, k=1, seconds=s)[0] for s in (3, 1)]
    store = RirStore(slots=4 * 2 * NODES, cap=sr, device=DEV, group=4)
    index = RirIndex(4)
    groups = {}
    for scene in range(2):
        index.add_scene(f"s{scene}", NODES)
        for r in range(NODES):                                               # the source stands on node 2
            groups[(scene, r)] = [np.ascontiguousarray(O.synth_rir(rng, sr, length=int(rng.integers(2000, 9000)), n=1)[0].T)
                                  for _ in range(4)]
    bases = store.slot_many(list(groups), [(lambda g=g: g) for g in groups.values()])
    for (scene, r), b in zip(groups, bases):
        index.set(scene, r, 2, b)
    return clips, store, index


def _observer(sr, clips, store, index, overlap, n=N_ENV, **kw):
    from ss_amd.context import AudioContext
    from ss_amd.vector import FastVectorAudioObserver, VectorSimState
    ctx = AudioContext(sr)
    ctx.set_rir_bank(store.bank.data, store.bank.lengths)
    ids = [ctx.add_source(f"snd{k}", c) for k, c in enumerate(clips)]
    if overlap:
        ctx.set_overlap(overlap)
    st = VectorSimState(n)
    st.audio_index[:] = 0
    st.src[:] = 2
    st.duration[:] = 6
    return ctx, st, FastVectorAudioObserver(ctx, st, index, sr, pose_cache=True, **kw), np.asarray(ids)


@pytest.mark.parametrize("sr,want_ag,overlap", [(16000, True, 0), (44100, False, 0), (16000, True, 2)],
                         ids=["16k-both-outputs", "44k-spectrogram-only", "16k-overlap-2-no-join-between-steps"])
def test_native_pose_cache_equals_the_python_pose_cache_bit_for_bit(sr, want_ag, overlap):
    from ss_amd import _lib
    from ss_amd.planning import spectrogram_shape
    clips, store, index = _world(sr)
    ctx_p, st_p, py, ids = _observer(sr, clips, store, index, overlap)
    ctx_n, st_n, nat, _ = _observer(sr, clips, store, index, overlap, native_pose_cache=True, pose_pool_rows=2)
    assert nat.native_memo and not nat.native and not py.native_memo and not py.native
    shape = spectrogram_shape(sr)
    assert sr != 44100 or int(np.prod(shape)) == 8970

    def outs():                                                              # rows of their own per step: steps in flight under
        sg = torch.full((STEPS, N_ENV) + shape, float("nan"), device=DEV)    # overlap must not share output rows
        ag = torch.full((STEPS, N_ENV, 2, sr), float("nan"), device=DEV) if want_ag else None
        return sg, ag
    (sg_p, ag_p), (sg_n, ag_n) = outs(), outs()
    sound = np.full(N_ENV, -1)
    for t, (recv, rot, cnt, snd, scene) in enumerate(_script()):
        for st in (st_p, st_n):
            st.audio_index[:] = np.where(snd != sound, 0, st.audio_index)    # what reconfigure does with a new sound
            st.recv[:], st.rot[:], st.step_count[:], st.sound[:], st.scene[:] = recv, rot, cnt, ids[snd], scene
            st.dirty[:] = False
        sound = snd
        py.observe(spectrogram_out=sg_p[t], audiogoal_out=ag_p[t] if want_ag else None)
        nat.observe(spectrogram_out=sg_n[t], audiogoal_out=ag_n[t] if want_ag else None)
        assert np.array_equal(st_p.audio_index, st_n.audio_index), t
        assert (nat.pose_hits, nat.pose_misses) == (py.pose_hits, py.pose_misses), t
        if not overlap:
            assert torch.equal(sg_n[t], sg_p[t]), t
            assert not want_ag or torch.equal(ag_n[t], ag_p[t]), t
    ctx_n.join()
    ctx_p.join()
    torch.cuda.synchronize()
    assert torch.equal(sg_n, sg_p) and not torch.isnan(sg_n).any()
    assert not want_ag or (torch.equal(ag_n, ag_p) and not torch.isnan(ag_n).any())
    assert py.pose_hits >= 10 and py.pose_misses >= 8                         # the script exercises both
    stats = ctx_n.memo_stats()
    assert stats["dropped"] == 2 and nat._memo_pool["rows"] > 2 and stats["rows"] <= nat._memo_pool["rows"]
    assert bool((sg_n[:, :, 0, 0, 0] == 0).any()) and float(sg_n.abs().max()) > 0       # silence and sound both occurred
    # the memo's rows were stored with this set of outputs: another set is refused, and nothing changes
    other = dict(spectrogram_out=None, audiogoal_out=torch.empty((N_ENV, 2, sr), device=DEV)) if not want_ag else \
        dict(spectrogram_out=sg_n[0], audiogoal_out=None)
    pool = ctx_n.memo_pool(spectrogram=None if not want_ag else nat._memo_pool["keep"][0],
                           audiogoal=torch.empty((nat._memo_pool["rows"], 2, sr), device=DEV) if not want_ag else None)
    before = st_n.audio_index.copy()
    with pytest.raises(_lib.SsHipError):
        ctx_n.observe_sims_memo(nat._bound, pool, **other)
    assert ctx_n.memo_stats() == stats and np.array_equal(st_n.audio_index, before)


def test_more_envs_than_one_argument_table():
    """300 envs: the step's move list rides in the kernel arguments 256 moves at a time - all stores (256 + 44), stores and
    fetches mixed inside one table (150 + 106, then 44 fetches), all fetches"""
    sr, n = 16000, 300
    clips, store, index = _world(sr)
    ctx_p, st_p, py, ids = _observer(sr, clips, store, index, 0, n=n)
    ctx_n, st_n, nat, _ = _observer(sr, clips, store, index, 0, n=n, native_pose_cache=True, pose_pool_rows=2)
    sg_p, sg_n = (torch.full((n, 65, 26, 2), float("nan"), device=DEV) for _ in range(2))
    env = np.arange(n)
    for t, recv in enumerate((env % NODES, np.where(env % 2 == 0, (env + 1) % NODES, env % NODES), env % NODES)):
        for st in (st_p, st_n):
            st.recv[:], st.rot[:], st.step_count[:], st.sound[:], st.scene[:] = recv, 90 * (env % 4), t, ids[env % 2], env % 2
            st.dirty[:] = False
        py.observe(spectrogram_out=sg_p)
        nat.observe(spectrogram_out=sg_n)
        assert torch.equal(sg_n, sg_p) and not torch.isnan(sg_n).any(), t
        assert np.array_equal(st_p.audio_index, st_n.audio_index)
        assert (nat.pose_hits, nat.pose_misses) == (py.pose_hits, py.pose_misses) == ((0, 300), (150, 450), (450, 450))[t]


# ---- (c) deferred mode: the resolver's pool copies as one k_memo_rows launch ---------------------------------------------
def test_deferred_resolver_native_pool_copies_equal_the_index_dispatches_bit_for_bit():
    """6 pose_cache workers over 4 steps (all miss; stand still; half of them leave, one changes its sound; come back): the same
    requests through ``DeferredResolver(native_pose_cache=True)`` and through the unchanged resolver, each on an engine of its
    own - spectrogram and audiogoal equal bit for bit at every step."""
    import pickle
    from fakes import FakeSim
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    from test_deferred import SR, make_world
    sounds, files = make_world()
    sims = [FakeSim(SR, sounds, files) for _ in range(6)]
    for i, s in enumerate(sims):
        attach_deferred(s, env_rank=i, pose_cache=True)
        s._current_sound, s._audio_index, s._duration = "long.wav", 0, 6
    py = DeferredResolver(AudioEngine(SR, device=DEV, rir_slots=64), rir_reader=files.get)
    nat = DeferredResolver(AudioEngine(SR, device=DEV, rir_slots=64), rir_reader=files.get, native_pose_cache=True)
    home = [(i % 4, 90 * (i % 3)) for i in range(6)]
    away = [((i + 1) % 4, 90 * ((i + 1) % 4)) for i in range(6)]
    hits = []
    for step, poses in enumerate((home, home, [away[i] if i % 2 else home[i] for i in range(6)], home)):
        for i, (s, (recv, rot)) in enumerate(zip(sims, poses)):
            if step == 2 and i == 0:                                          # reconfigure with a new sound (:395-397)
                s._current_sound, s._audio_index = "telephone.wav", 0
                s._audiogoal_cache, s._spectrogram_cache = dict(), dict()
            s._receiver_position_index, s._rotation_angle, s._episode_step_count = recv, rot, step
        reqs = [s.get_current_spectrogram_observation(None) for s in sims]
        hits.append(sum(bool(q.cache_hit) for q in reqs))
        a = py.resolve(pickle.loads(pickle.dumps(reqs)), want_audiogoal=True)
        b = nat.resolve(pickle.loads(pickle.dumps(reqs)), want_audiogoal=True)
        torch.cuda.synchronize()
        for name in ("spectrogram", "audiogoal"):
            assert torch.equal(a[name], b[name]) and float(a[name].abs().max()) > 0, (step, name)
    assert hits == [0, 6, 2, 6]
    assert nat._pose_moves and not py._pose_moves                            # the native resolver took the one-launch route
