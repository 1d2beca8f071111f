"""Captured steps on the GPU (include/ss_hip.h "Captured steps", ss_amd/graphs.py): the stateless ops recorded into a
torch.cuda.CUDAGraph on one side stream and replayed there, their inputs rewritten in place between the replays.

Protocol of every test: a step = ops.source_windows_into + one observation op over fixed tensors (tests/replay_plan.py: three
units - one with a distractor term, one plain, one silent - whose slots, window starts and bank entries move with the step number,
and a clip that is rolled and rescaled).  The step is captured with graphs.capture, then replayed on the inputs of steps 1, 2, ...;
after each replay the same inputs are rendered by an EAGER call of the same ops on ANOTHER stream (its own scratches) into other
tensors, and the two results must be torch.equal: the same kernels on the same numbers - a difference is a finding, there is no
tolerance.  Every output is pre-filled with NaN before every replay and every eager call; live units are non-zero, the silent unit
exact zeros.

  1. 44.1 kHz rows (44 100 samples: three output blocks; 22 050: two), small steps: k_obs_blocks, whose workgroups hand samples
     over through flags that carry the launch's epoch.  A captured launch reads the epoch from a word that k_sync_next moves on at
     every replay: replay_epoch() == -k after replay k.  From fp32 rows, fp32 block spectra and half rows; the stream prepared
     by ss_stream_reserve alone (no warm-up call).
  2. the same with one eager call on the graph's OWN stream between replays 2 and 3 (a positive epoch from the host counter over
     the same hand-off area): everything stays exact, the replay epoch is not moved by it.
  3. 16 kHz: the fused one-block kernel (k_conv), captured after a warm-up call.
  4. k_obs_rows: rows of 16 584 samples of which 16 400 are rendered (n_valid < out_len declines k_obs_blocks, n_valid > one block
     declines the one-block form): the smallest shape of that route; its stash comes from ss_stream_reserve.

Each test first calls ss_release_scratch, so that the stream it captures on - torch deals streams out of a pool - starts without a
hand-off area and its replay epoch at 0.  No test provokes an error inside an open capture (tests/test_stream_reserve_args.py
covers the refusals on the host)."""
import types

import numpy as np
import pytest
import torch

from ss_amd import planning as P

import replay_plan as RP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = ("rows", "spectra", "rir16")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # (a copy: the worlds are read-only arrays)


def _clip(clips, k):
    """the clip of step k: rolled and rescaled (every sample changes)"""
    return np.ascontiguousarray(np.roll(clips, 997 * k, axis=1) * np.float32(1.0 - 0.11 * k)).reshape(-1)


class Step:
    """the tensors of one step: inputs, the window spectra in between, outputs"""

    def __init__(self, n_units, n_windows, clip_len, out_len):
        self.clip = torch.zeros((clip_len,), dtype=torch.float32, device=DEV)
        self.win_desc = torch.zeros((n_windows, 4), dtype=torch.int32, device=DEV)
        self.unit_desc = torch.zeros((n_units, 8), dtype=torch.int32, device=DEV)
        self.spec = torch.zeros((n_windows, P.SPEC_FLOATS), dtype=torch.float32, device=DEV)
        self.ag = torch.empty((n_units, 2, out_len), dtype=torch.float32, device=DEV)
        self.sg = torch.empty((n_units,) + P.spectrogram_shape(out_len), dtype=torch.float32, device=DEV)

    def load(self, clip, wd, desc):
        """rewrite the inputs IN PLACE and poison the outputs (and the window spectra: the step recomputes them)"""
        assert tuple(wd.shape) == tuple(self.win_desc.shape) and tuple(desc.shape) == tuple(self.unit_desc.shape)
        self.clip.copy_(torch.from_numpy(clip))
        self.win_desc.copy_(torch.from_numpy(wd))
        self.unit_desc.copy_(torch.from_numpy(desc))
        for t in (self.spec, self.ag, self.sg):
            t.fill_(float("nan"))


@pytest.fixture()
def env():
    from ss_amd import _lib, ops
    ops.init()
    torch.cuda.synchronize()
    _lib.check(_lib.load().ss_release_scratch(), "ss_release_scratch")
    return types.SimpleNamespace(other=torch.cuda.Stream())


def _setup(form, out_len, n_valid):
    """-> (inputs(k) -> (clip, win_desc, unit_desc, units), fn(step) -> the step's closure, graph tensors, eager tensors)"""
    from ss_amd import ops
    clips, bank, lens = RP.world(out_len, seed=out_len)
    bank_d, lens_d = _dev(bank), _dev(lens)
    if form == "spectra":
        hspec = ops.rir_spectra(bank_d)
    elif form == "rir16":
        q, s = ops.rir_rows16(bank_d)
    torch.cuda.synchronize()

    def inputs(k):
        units = RP.step_units(k, out_len)
        wd, desc = RP.plan(units, clips.shape[1], n_valid)
        return _clip(clips, k), wd, desc, units

    def fn(t):
        def step():
            ops.source_windows_into(t.clip, t.win_desc, t.spec)
            if form == "rows":
                ops.audio_obs_into(t.spec, bank_d, lens_d, t.unit_desc, t.ag, t.sg, n_valid, out_len)
            elif form == "spectra":
                ops.audio_obs_spec_into(t.spec, hspec, lens_d, t.unit_desc, t.ag, t.sg, n_valid, out_len)
            else:
                ops.audio_obs_rows_rir16_into(t.spec, q, s, lens_d, t.unit_desc, t.ag, t.sg, n_valid, out_len)
        return step

    _, wd0, desc0, _ = inputs(0)
    mk = lambda: Step(desc0.shape[0], wd0.shape[0], clips.size, out_len)
    return inputs, fn, mk(), mk()


def _check(label, g, e, units, n_valid):
    """graph result == eager result, bit for bit; nothing left poisoned; live units live, the silent unit exact zeros"""
    for name in ("ag", "sg"):
        a, b = getattr(g, name), getattr(e, name)
        assert not bool(torch.isnan(b).any()), (label, name, "eager")
        same = torch.equal(a, b)
        if not same:
            d = (a - b).abs()
            print(f"[graph_replay] {label} {name}: {int((a != b).sum())} elements differ, max |diff| = {float(d.nan_to_num(nan=float('inf')).max()):.3e}, "
                  f"NaN in the replay: {int(torch.isnan(a).sum())}")
        assert same, (label, name)
    for n, u in enumerate(units):
        if u.get("rir", -1) < 0:
            assert not bool(g.ag[n].view(torch.int32).any()) and not bool(g.sg[n].view(torch.int32).any()), (label, n)
        else:
            assert float(g.ag[n, :, :n_valid].abs().max()) > 0 and float(g.sg[n].abs().max()) > 0, (label, n)
    assert not bool(g.ag[:, :, n_valid:].any())


def _eager(env, fn_e, e, ins):
    """the same inputs through an eager call on the other stream"""
    e.load(*ins[:3])
    env.other.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(env.other):
        fn_e()
    torch.cuda.synchronize()


def _protocol(env, form, out_len, n_valid, reserve, n_replays=4, eager_own_stream_after=None, want_epochs=True):
    from ss_amd import graphs
    inputs, fn, g, e = _setup(form, out_len, n_valid)
    fn_g, fn_e = fn(g), fn(e)
    g.load(*inputs(0)[:3])
    torch.cuda.synchronize()
    cap = graphs.capture(fn_g, reserve=reserve)
    label = f"{form} {out_len}/{n_valid}"
    if want_epochs is not None:
        assert cap.replay_epoch() == 0
    for k in range(1, n_replays + 1):
        ins = inputs(k)
        g.load(*ins[:3])
        cap.replay()
        torch.cuda.synchronize()
        _eager(env, fn_e, e, ins)
        _check(f"{label} replay {k}", g, e, ins[3], n_valid)
        if want_epochs is not None:
            assert cap.replay_epoch() == (-k if want_epochs else 0), (label, k)
        if eager_own_stream_after == k:                                 # an eager launch over the graph's own hand-off area
            ins = inputs(10 + k)
            g.load(*ins[:3])
            cap.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap.stream):
                fn_g()
            torch.cuda.synchronize()
            _eager(env, fn_e, e, ins)
            _check(f"{label} eager call on the graph's stream after replay {k}", g, e, ins[3], n_valid)
            assert cap.replay_epoch() == -k, (label, "the eager call moved the replay epoch")
    return cap


@pytest.mark.parametrize("out_len", [44100, 22050], ids=["3-blocks", "2-blocks"])
@pytest.mark.parametrize("form", FORMS)
def test_obs_blocks_replays_equal_eager_launches(env, form, out_len):
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 6 * P.ceil_div(out_len, P.KB) <= n_cus                       # (rows x output blocks fit the chip: k_obs_blocks)
    _protocol(env, form, out_len, out_len, dict(out_len=out_len, rir_cap=RP.RIR_CAP, n_terms=2))


def test_obs_blocks_eager_call_on_the_graphs_stream_between_replays(env):
    _protocol(env, "rows", 44100, 44100, dict(out_len=44100, rir_cap=RP.RIR_CAP, n_terms=2), eager_own_stream_after=2)


def test_fused_16k_replays_equal_eager_launches(env):
    """the one-block route: no hand-off area, no stash; captured after a warm-up call (ss_stream_reserve serves longer rows)"""
    _protocol(env, "rows", 16000, 16000, None, want_epochs=None)


def test_obs_rows_replays_equal_eager_launches_after_reserve(env):
    """k_obs_rows at its smallest: 2 units' worth of live rows (+ the silent one), two output blocks, the second of 16 samples"""
    out_len, n_valid = P.KB + 200, P.KB + 16
    _protocol(env, "rows", out_len, n_valid, dict(out_len=out_len, rir_cap=RP.RIR_CAP, n_terms=2), n_replays=2, want_epochs=False)
