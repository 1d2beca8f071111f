"""The pose memo's host half through libss_hip.so (ss_ctx_sims_memo_plan: memo plan + unit columns + audio_index, no GPU)
against ``FastVectorAudioObserver(pose_cache=True)`` on an ``OracleContext`` twin, step for step: the script of
tests/test_vector.py's pose-cache test and a seeded walk (8 envs, 200 steps, 6 poses, 3-s and 1-s sounds, sound and scene
changes, durations that run out).  Per step: the same hit and miss sets, the same unit columns for the envs that are rendered,
the same ``_audio_index``, the same counters; every fetch names the pool row stored for that (env, pose) earlier and no row is
live twice (row numbers themselves are the library's own and are not compared); and, end to end, carrying the planned moves out
on a host pool gives every env the observation the Python observer gives it.  The twin's ``observe`` writes a tag naming
(sound, window) instead of running the oracle's convolution: the arithmetic is not what is compared here."""
import ctypes

import numpy as np
import pytest
import torch

from fakes import OracleContext
from ss_amd import _lib
from ss_amd.context import AudioContext
from ss_amd.vector import FastVectorAudioObserver, RirIndex, VectorSimState

SR = 16000
LENGTHS = [3 * SR, SR, 3 * SR]                      # snd0 / snd2: 3-s sounds, snd1: the 1-s sound
NODES = 6


class TagContext(OracleContext):
    """OracleContext whose observe() writes one tag per row - 0 for a silent unit, else 1 + 1000 * sound + window + rir / 4096 -
    instead of audio (so 200 steps of 8 envs stay quick)."""

    def observe(self, sound, t0, rir, spectrogram_out=None, audiogoal_out=None, **kw):
        self.calls += 1
        spectrogram_out[:, 0, 0, 0] = torch.from_numpy(tags(sound, t0, rir))


def tags(sound, t0, rir):
    sound, t0, rir = (np.asarray(v, np.int64) for v in (sound, t0, rir))
    return np.where(rir < 0, 0.0, 1.0 + 1000.0 * sound + t0 // SR + rir / 4096.0).astype(np.float32)


def make_index(skip=()):
    index = RirIndex(4)
    for k in range(2):
        sid = index.add_scene(f"s{k}", NODES)
        for r in range(NODES):
            for s in range(NODES):
                if (k, r, s) not in skip:
                    index.set(sid, r, s, 4 * (100 * k + r * NODES + s))
    return index


class Twins:
    """Python observer on a TagContext (a) and the library's memo on a planner-only AudioContext (b), same columns."""

    def __init__(self, n, index, pool_rows=2):
        self.n, self.index = n, index
        self.py_ctx = TagContext(SR, None)
        self.ctx = AudioContext(SR)
        for k, L in enumerate(LENGTHS):
            self.py_ctx.add_source(f"snd{k}", np.zeros(L, np.float32))
            self.ctx.add_source_len(f"snd{k}", L)
        self.a, self.b = VectorSimState(n), VectorSimState(n)
        for st in (self.a, self.b):
            for col in ("audio_index", "step_count", "recv", "src", "rot", "sound"):
                getattr(st, col)[:] = 0
            st.duration[:] = 1 << 30
        self.obs = FastVectorAudioObserver(self.py_ctx, self.a, index, SR, pose_cache=True)
        self.seen = []
        orig = self.obs.columns

        def spy(hold=None):
            cols = orig(hold=hold)
            self.seen.append((hold.copy(), cols))
            return cols
        self.obs.columns = spy
        self.bound = self.ctx.bind_sims(self.b, index)
        self.ctx.memo_enable(n)
        self.pool_rows = pool_rows
        self.pool = np.full((pool_rows,), np.nan, np.float32)
        self.sg = torch.zeros((n, 65, 26, 2))
        self.stored = {}                             # (env, pose key) -> pool row, as the moves told it
        self.tag = [None] * n
        self.grown = 0

    def set(self, **cols):
        for st in (self.a, self.b):
            for k, v in cols.items():
                getattr(st, k)[:] = v
            st.dirty[:] = False

    def step(self, label):
        a, b, n = self.a, self.b, self.n
        self.obs.observe(spectrogram_out=self.sg)
        hold_py, cols_py = self.seen.pop()
        before = b.audio_index.copy()
        stats0 = self.ctx.memo_stats()
        p = self.ctx.sims_memo_plan(self.bound, self.pool_rows)
        if p["need_rows"]:                                                 # the pool is short: nothing committed, grow, again
            assert p["need_rows"] > self.pool_rows and len(p["stores"]) == len(p["fetches"]) == 0, label
            assert np.array_equal(b.audio_index, before) and self.ctx.memo_stats() == stats0, label
            self.pool = np.concatenate([self.pool, np.full((p["need_rows"] - self.pool_rows,), np.nan, np.float32)])
            self.pool_rows = p["need_rows"]
            self.grown += 1
            p = self.ctx.sims_memo_plan(self.bound, self.pool_rows)
        assert p["need_rows"] == 0 and p["missing"].size == 0, label
        # hit and miss sets; unit columns of the envs that are rendered; audio_index; counters
        assert np.array_equal(p["hold"], hold_py), label
        live = cols_py["rir"] >= 0
        assert not (live & hold_py).any() and np.array_equal(p["cols"]["rir"], cols_py["rir"]), label
        for name in ("sound", "t0"):
            assert np.array_equal(p["cols"][name][live], cols_py[name][live]), (label, name)
        assert np.array_equal(a.audio_index, b.audio_index), label
        s = self.ctx.memo_stats()
        assert (s["hits"], s["misses"]) == (self.obs.pose_hits, self.obs.pose_misses), label
        # the moves: every env once, misses stored, hits fetched from the row stored for that (env, pose); no row live twice
        key = (b.src << 40) | (b.recv << 20) | ((-b.rot) % 360)
        for i in range(n):
            t = (int(b.scene[i]), int(b.sound[i]))
            if self.tag[i] != t:
                self.tag[i] = t
                for k in [k for k in self.stored if k[0] == i]:
                    del self.stored[k]
        assert sorted(p["stores"][:, 0].tolist() + p["fetches"][:, 0].tolist()) == list(range(n)), label
        assert sorted(p["stores"][:, 0].tolist()) == np.flatnonzero(~hold_py).tolist(), label
        for env, row in p["fetches"]:
            assert self.stored[(int(env), int(key[env]))] == int(row), (label, env)
        for env, row in p["stores"]:
            assert 0 <= row < self.pool_rows and int(row) not in self.stored.values(), (label, env, row)
            self.stored[(int(env), int(key[env]))] = int(row)
        assert s["rows"] == len(self.stored) == len(set(self.stored.values())), label
        # end to end: render the planned units as tags, carry the moves out, compare with the Python observer's rows
        out = tags(p["cols"]["sound"], p["cols"]["t0"], p["cols"]["rir"])
        self.pool[p["stores"][:, 1]] = out[p["stores"][:, 0]]
        out[p["fetches"][:, 0]] = self.pool[p["fetches"][:, 1]]
        assert np.array_equal(out, self.sg[:, 0, 0, 0].numpy()), label
        return p


def test_script_of_the_pose_cache_test_step_for_step():
    """stand still, leave and come back, silence after the duration, a sound change (tests/test_vector.py's script), then a
    scene change"""
    tw = Twins(2, make_index())
    tw.set(scene=np.array([0, 1]), src=2, duration=6)
    script = [((1, 90, 0, 0), (2, 0, 0, 0)), ((1, 90, 1, 0), (2, 0, 1, 0)),
              ((3, 90, 2, 0), (2, 90, 2, 0)), ((1, 90, 3, 0), (2, 0, 3, 0)),
              ((4, 180, 4, 0), (4, 0, 4, 0)), ((4, 180, 7, 0), (1, 0, 7, 0)),
              ((1, 90, 8, 1), (1, 0, 8, 0)),
              ((1, 90, 9, 1), (2, 0, 9, 0))]
    sound = np.zeros(2, np.int64)
    for step, moves in enumerate(script):
        recv, rot, cnt, snd = (np.array(v) for v in zip(*moves))
        ai = np.where(snd != sound, 0, tw.a.audio_index)                       # what reconfigure does with a new sound
        sound = snd
        tw.set(recv=recv, rot=rot, step_count=cnt, sound=snd, audio_index=ai)
        tw.step(step)
    assert tw.obs.pose_hits >= 5 and tw.obs.pose_misses >= 8 and tw.grown >= 2
    assert tw.ctx.memo_stats()["dropped"] == 1
    tw.set(scene=np.array([0, 0]))                                             # env 1 changes its scene: its map is dropped
    p = tw.step("scene change")
    assert tw.ctx.memo_stats()["dropped"] == 2 and p["hold"].tolist() == [True, False]


def test_seeded_walk_8_envs_200_steps():
    rng = np.random.default_rng(11)
    n = 8
    tw = Twins(n, make_index())
    poses = [(r, rot) for r in (0, 1, 2) for rot in (0, 90)]
    cols = dict(scene=rng.integers(0, 2, n), sound=rng.integers(0, 3, n), recv=np.zeros(n, np.int64), rot=np.zeros(n, np.int64),
                src=np.full(n, 2), step_count=np.zeros(n, np.int64), duration=rng.integers(2, 8, n), audio_index=np.zeros(n, np.int64))
    for step in range(200):
        cols["audio_index"] = tw.a.audio_index.copy()
        cols["step_count"] = cols["step_count"] + 1
        for i in range(n):
            r = rng.uniform()
            if r < 0.4:
                cols["recv"][i], cols["rot"][i] = poses[int(rng.integers(0, 6))]
            if r > 0.92:                                                       # a new episode
                snd = int(rng.integers(0, 3))
                if snd != cols["sound"][i]:
                    cols["sound"][i], cols["audio_index"][i] = snd, 0
                if r > 0.97:
                    cols["scene"][i] = int(rng.integers(0, 2))
                cols["step_count"][i], cols["duration"][i] = 0, int(rng.integers(2, 8))
        tw.set(**cols)
        tw.step(step)
    s = tw.ctx.memo_stats()
    assert s["hits"] > 200 and s["misses"] > 200 and s["dropped"] > 5 and tw.grown >= 3
    assert (tw.a.step_count > tw.a.duration).any() or s["misses"] > 0


def _twin_contexts(index, n=3):
    out = []
    for _ in range(2):
        ctx = AudioContext(SR)
        for k, L in enumerate(LENGTHS):
            ctx.add_source_len(f"snd{k}", L)
        st = VectorSimState(n)
        for col in ("audio_index", "step_count", "rot", "sound", "scene"):
            getattr(st, col)[:] = 0
        st.duration[:] = 1 << 30
        st.src[:] = 3
        st.recv[:] = np.arange(n)
        ctx.memo_enable(n)
        out.append((ctx, st, ctx.bind_sims(st, index)))
    return out


def _same(p, q):
    return (np.array_equal(p["hold"], q["hold"]) and np.array_equal(p["stores"], q["stores"]) and np.array_equal(p["fetches"], q["fetches"])
            and all(np.array_equal(p["cols"][k], q["cols"][k]) for k in p["cols"]) and p["need_rows"] == q["need_rows"]
            and np.array_equal(p["missing"], q["missing"]))


def test_a_non_resident_pair_commits_nothing():
    """*n_miss > 0: audio_index, the stats and the next plan are what they would have been without the call"""
    index = make_index(skip={(0, 2, 3)})
    (ctx_a, a, bound_a), (ctx_b, b, bound_b) = _twin_contexts(index)
    for st in (a, b):
        st.recv[:] = [0, 1, 4]
    assert _same(ctx_a.sims_memo_plan(bound_a, 8), ctx_b.sims_memo_plan(bound_b, 8))
    a.recv[:] = [0, 2, 5]                                                    # env 1 walks onto the pair that is not resident
    before, stats = a.audio_index.copy(), ctx_a.memo_stats()
    p = ctx_a.sims_memo_plan(bound_a, 8)
    assert p["missing"].tolist() == [1] and p["need_rows"] == 0 and len(p["stores"]) == len(p["fetches"]) == 0
    assert p["hold"].tolist() == [True, False, False]
    assert np.array_equal(a.audio_index, before) and ctx_a.memo_stats() == stats
    index.set(0, 2, 3, 4 * 999)                                               # the loader brings the pair in
    b.recv[:] = [0, 2, 5]
    pa, pb = ctx_a.sims_memo_plan(bound_a, 8), ctx_b.sims_memo_plan(bound_b, 8)
    assert _same(pa, pb) and pa["missing"].size == 0 and len(pa["stores"]) == 2 and pa["cols"]["rir"][1] == 4 * 999
    assert np.array_equal(a.audio_index, b.audio_index) and ctx_a.memo_stats() == ctx_b.memo_stats()
    # a short pool AND a pair that is not resident: one call reports both, and commits nothing
    index.set(0, 2, 3, -1)
    a.recv[:] = [3, 4, 5]
    a.rot[:] = 90
    p = ctx_a.sims_memo_plan(bound_a, 8)
    assert p["missing"].size == 0 and p["need_rows"] == 0 and ctx_a.memo_stats()["rows"] == 8      # the pool of 8 is full now
    a.recv[:] = [0, 2, 1]
    a.rot[:] = 180
    before, stats = a.audio_index.copy(), ctx_a.memo_stats()
    p = ctx_a.sims_memo_plan(bound_a, 8)
    assert p["missing"].tolist() == [1] and p["need_rows"] == 11
    assert np.array_equal(a.audio_index, before) and ctx_a.memo_stats() == stats


def test_need_rows_when_the_pool_is_short():
    index = make_index()
    (ctx, st, bound), _ = _twin_contexts(index)
    p = ctx.sims_memo_plan(bound, 2)
    assert p["need_rows"] == 3 and len(p["stores"]) == 0 and ctx.memo_stats() == dict(hits=0, misses=0, rows=0, dropped=0)
    assert np.array_equal(st.audio_index, [0, 0, 0])
    p = ctx.sims_memo_plan(bound, 3)
    assert p["need_rows"] == 0 and sorted(p["stores"][:, 1].tolist()) == [0, 1, 2] and np.array_equal(st.audio_index, [1, 1, 1])
    st.recv[:] = [3, 4, 5]
    assert ctx.sims_memo_plan(bound, 3)["need_rows"] == 6                     # the total, not the shortfall
    st.sound[:] = [0, 2, 2]                                                   # envs 1 and 2 change their sound: their rows are
    st.audio_index[1:] = 0
    p = ctx.sims_memo_plan(bound, 4)                                          # free again and serve this very step
    assert p["need_rows"] == 0 and len(p["stores"]) == 3 and ctx.memo_stats()["rows"] == 4
    assert ctx.memo_stats()["dropped"] == 2
    with pytest.raises(_lib.SsHipError):                                      # rows never shrink below what was handed out
        ctx.sims_memo_plan(bound, 3)
    ctx.memo_reset()
    assert ctx.memo_stats() == dict(hits=0, misses=0, rows=0, dropped=0)
    assert ctx.sims_memo_plan(bound, 3)["need_rows"] == 0


def test_a_held_env_on_a_non_resident_pair_is_no_miss():
    index = make_index()
    (ctx, st, bound), _ = _twin_contexts(index)
    assert ctx.sims_memo_plan(bound, 4)["missing"].size == 0
    index.set(0, 1, 3, -1)                                                    # env 1's pair is evicted; it stands still
    ai = st.audio_index.copy()
    p = ctx.sims_memo_plan(bound, 4)
    assert p["missing"].size == 0 and p["hold"].all() and (p["cols"]["rir"] == -1).all() and len(p["fetches"]) == 3
    assert np.array_equal(st.audio_index, ai)                                 # hits do not advance
    st.rot[1] = 90                                                            # it turns: a new pose, and now the pair is missed
    assert ctx.sims_memo_plan(bound, 8)["missing"].tolist() == [1]


def test_einval_of_the_context_entries():
    index = make_index()
    lib = _lib.load()
    ctx = AudioContext(SR)
    ctx.add_source_len("snd0", 3 * SR)
    st = VectorSimState(3)
    for col in ("audio_index", "step_count", "rot", "sound", "scene", "recv", "src"):
        getattr(st, col)[:] = 0
    st.duration[:] = 9
    bound = ctx.bind_sims(st, index)
    bound_dis = ctx.bind_sims(st, index, True)
    n_miss, need, ns, nf = (ctypes.c_int(7) for _ in range(4))
    miss, units, hold, moves = (np.zeros(64, np.int32) for _ in range(4))
    pool = _lib.SsMemoPool(4096, 8192, 8, 0)
    AG, SG = 12288, 16384                                                    # dummy device pointers: never dereferenced here
    A = ctypes.addressof

    def plan(cols=bound["cols"], n=3, rows=8, units_p=units.ctypes.data, n_miss_p=A(n_miss), need_p=A(need)):
        return lib.ss_ctx_sims_memo_plan(ctx._h, ctypes.byref(cols) if cols is not None else None, n, rows, units_p, hold.ctypes.data,
                                         moves.ctypes.data, A(ns), A(nf), miss.ctypes.data, n_miss_p, need_p)

    def observe(cols=bound["cols"], n=3, ag=AG, sg=SG, pool_p=ctypes.byref(pool), n_miss_p=A(n_miss), need_p=A(need)):
        return lib.ss_ctx_observe_sims_memo(ctx._h, ctypes.byref(cols) if cols is not None else None, n, ag, sg, pool_p, miss.ctypes.data,
                                            n_miss_p, need_p, None)

    out4 = np.zeros(4, np.int64)
    # the memo is not enabled
    assert plan() == -1 and observe() == -1
    assert lib.ss_ctx_memo_reset(ctx._h) == -1 and lib.ss_ctx_memo_stats(ctx._h, out4.ctypes.data) == -1
    assert lib.ss_ctx_memo_enable(ctx._h, -1) == -1 and lib.ss_ctx_memo_enable(None, 3) == -1
    ctx.memo_enable(3)
    assert lib.ss_ctx_memo_stats(ctx._h, None) == -1
    # n != n_envs, a distractor, a bad pool size
    assert plan(n=2) == -1 and plan(n=4) == -1 and observe(n=2) == -1
    assert plan(cols=bound_dis["cols"]) == -1 and observe(cols=bound_dis["cols"]) == -1
    assert plan(rows=-1) == -1
    # what ss_ctx_observe_sims refuses: no columns, no miss counter; and no need_rows, no outputs of the plan
    assert plan(cols=None) == -1 and observe(cols=None) == -1
    assert plan(n_miss_p=None) == -1 and observe(n_miss_p=None) == -1
    assert plan(need_p=None) == -1 and observe(need_p=None) == -1 and plan(units_p=None) == -1
    bad = _lib.SsSimColumns.from_buffer_copy(bound["cols"])
    bad.azimuths = 7
    assert plan(cols=bad) == -1 and observe(cols=bad) == -1
    # the pool: NULL, rows < 0, an output without its pool array, a pool array without its output, no output at all
    assert observe(pool_p=None) == -1
    assert observe(pool_p=ctypes.byref(_lib.SsMemoPool(4096, 8192, -1, 0))) == -1
    assert observe(pool_p=ctypes.byref(_lib.SsMemoPool(4096, None, 8, 0))) == -1            # audiogoal asked for, no pool for it
    assert observe(pool_p=ctypes.byref(_lib.SsMemoPool(None, 8192, 8, 0))) == -1
    assert observe(ag=None) == -1 and observe(sg=None) == -1                                # pool arrays without their outputs
    assert observe(ag=None, sg=None, pool_p=ctypes.byref(_lib.SsMemoPool(None, None, 8, 0))) == -1
    assert observe(sg=SG + 2, ag=None, pool_p=ctypes.byref(_lib.SsMemoPool(4096, None, 8, 0))) == -1   # a misaligned output
    # none of it changed anything: the plan entry still works from a clean memo, and switching off frees it
    assert ctx.memo_stats() == dict(hits=0, misses=0, rows=0, dropped=0)
    assert plan() == 0 and n_miss.value == 0 and need.value == 0 and ns.value == 3 and nf.value == 0
    ctx.memo_enable(0)
    assert plan() == -1
