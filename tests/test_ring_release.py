"""The descriptor ring of ss_ctx_observe releases a group of slots through a completion event ONLY when the device was given
one of the group's slots to read (csrc/ss_ring.hpp): descriptors read in place by a kernel without a unit table, a descriptor
upload, a window upload.  Steps whose launch carries its units in the kernel arguments record nothing and wait for nothing -
their slots are rewritten a ring later with launches still in flight, which must not change a single result."""
import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd.context import AudioContext

SR = 16000
N_STEPS = 40            # 2.5 revolutions of the 16-slot ring
N_UNITS = 3
WARM = 20               # warm-up steps: every key's window upload, and one more revolution so that the group the uploads
                        # were recorded for has been waited for (16 slots, groups of 4: slot 20 is the first of a group)


@pytest.fixture(scope="module")
def world():
    """sources, RIRs, the seeded unit columns of the 40 steps (plain and with one distractor unit), and - computed once, read
    only - the stateless renderer's spectrograms of both forms of every step."""
    import torch
    from ss_amd.renderer import BatchedAudioRenderer, RirBank, UnitRequest
    dev = "cuda:0"
    rng = np.random.default_rng(77)
    src = list(O.synth_sources(rng, SR, k=3))
    rirs = [np.ascontiguousarray(h.T) for h in O.synth_rir(rng, SR, n=8)]
    bank = RirBank.from_arrays(rirs, dev)
    r = BatchedAudioRenderer(SR, device=dev)
    for i, s in enumerate(src):
        r.add_source(f"s{i}", s)
    r.set_rir_bank(bank)
    steps = []
    for k in range(N_STEPS):
        sound = rng.integers(0, 2, N_UNITS)                      # (sound 2 is kept for the "new key" test)
        rir = rng.integers(0, 8, N_UNITS)
        if k % 7 == 3:
            rir[int(rng.integers(0, N_UNITS))] = -1              # a silent unit now and then
        ds = np.full(N_UNITS, -1)
        dr = np.full(N_UNITS, -1)
        i = int(np.flatnonzero(rir >= 0)[0])
        ds[i], dr[i] = int(rng.integers(0, 2)), int(rng.integers(0, 8))
        steps.append(dict(sound=sound, t0=np.zeros(N_UNITS, np.int64), rir=rir, ds=np.maximum(ds, 0), dr=dr))
    plain, mixed = [], []
    for s in steps:
        _, sg = r.render(r.plan_arrays(s["sound"], s["t0"], s["rir"]))
        plain.append(sg.clone())
        units = [UnitRequest(int(a), 0, int(b), silent=b < 0, dis_sound=int(c), dis_rir=int(d))
                 for a, b, c, d in zip(s["sound"], s["rir"], s["ds"], s["dr"])]
        _, sg = r.render(r.plan(units))
        mixed.append(sg.clone())
    torch.cuda.synchronize()
    bank.build_spectra()                                         # the same steps from the spectral rows (the benchmark's route)
    spec = []
    for s in steps:
        _, sg = r.render(r.plan_arrays(s["sound"], s["t0"], s["rir"]))
        spec.append(sg.clone())
    torch.cuda.synchronize()
    return dict(dev=dev, src=src, rirs=rirs, bank=bank, steps=steps, plain=plain, mixed=mixed, spec=spec, oracle={})


def make_ctx(w, sounds=(0, 1, 2), spectral=False):
    ctx = AudioContext(SR)
    for i in sounds:
        ctx.add_source(f"s{i}", w["src"][i])
    ctx.set_rir_bank(w["bank"].data, w["bank"].lengths)
    if spectral:
        ctx.set_rir_spectra(w["bank"].spectra)
    return ctx


def warm_up(ctx, w):
    """WARM steps on sounds 0 and 1 (both keys uploaded by the first one), then a device synchronise"""
    import torch
    out = torch.empty((N_UNITS, 65, 26, 2), device=w["dev"])
    for k in range(WARM):
        ctx.observe([0, 1, 0], [0, 0, 0], [k % 8, 1, 2], spectrogram_out=out)
    torch.cuda.synchronize()
    return ctx.stats()


def observe_step(ctx, s, out, distractor=False):
    if distractor:
        ctx.observe(s["sound"], s["t0"], s["rir"], spectrogram_out=out, dis_sound=s["ds"], dis_rir=s["dr"])
    else:
        ctx.observe(s["sound"], s["t0"], s["rir"], spectrogram_out=out)


def oracle_of(w, k, distractor):
    """the oracle's spectrograms of step k (plain or with its distractor unit): computed once, shared, read only"""
    key = (k, bool(distractor))
    if key not in w["oracle"]:
        s = w["steps"][k]
        ref = np.zeros((N_UNITS, 65, 26, 2), np.float32)
        for i in range(N_UNITS):
            if s["rir"][i] < 0:
                continue
            has = distractor and s["dr"][i] >= 0
            a = O.compute_audiogoal(w["src"][s["sound"][i]], w["rirs"][s["rir"][i]], SR,
                                    distractor=w["src"][s["ds"][i]] if has else None,
                                    distractor_rir=w["rirs"][s["dr"][i]] if has else None)
            ref[i] = O.compute_spectrogram(a.astype(np.float32))
        w["oracle"][key] = ref
    return w["oracle"][key]


def check_outputs(w, outs, dis_of, refs=None):
    """every step: bit-equal to the stateless render of the same columns, and the oracle at the suite's 1e-4"""
    import torch
    for k, o in enumerate(outs):
        ref = ((w["mixed"] if dis_of(k) else w["plain"]) if refs is None else refs)[k]
        assert torch.equal(o, ref), f"step {k}"
        assert O.relerr(o.cpu().numpy(), oracle_of(w, k, dis_of(k))) <= 1e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("spectral", [False, True])               # k_conv<.., TAB> / k_conv_spec<.., TAB> (the benchmark's launcher)
def test_table_route_steps_record_no_event_and_wait_for_none(world, spectral):
    import torch
    w = world
    ctx = make_ctx(w, spectral=spectral)
    st0 = warm_up(ctx, w)
    assert st0["ring_events"] == 1 and st0["ring_waits"] == 1     # the group of the window upload, waited for a ring later
    outs = [torch.full((N_UNITS, 65, 26, 2), float("nan"), device=w["dev"]) for _ in range(N_STEPS)]
    for k, s in enumerate(w["steps"]):                            # nothing synchronised or joined until the end
        observe_step(ctx, s, outs[k])
    st1 = ctx.stats()
    torch.cuda.synchronize()
    check_outputs(w, outs, lambda k: False, refs=w["spec"] if spectral else None)
    assert st1["ring_events"] - st0["ring_events"] == 0 and st1["ring_waits"] - st0["ring_waits"] == 0
    assert st1["misses"] == st0["misses"]                         # (no window was uploaded: the steps were table steps)
    # the host's run-ahead is bounded by the pace event instead: one per 16 steps without a ring event (56 of the 60 here: the
    # first group recorded the ring's), each but the first after a wait for the one before
    assert st1["pace_events"] == 3 and st1["pace_waits"] == 2


@pytest.mark.gpu
def test_mixed_route_records_the_groups_that_were_read(world):
    """every other group holds one step with a distractor unit: the loop kernel, descriptors read in place from the slot"""
    import torch
    w = world
    ctx = make_ctx(w)
    st0 = warm_up(ctx, w)
    dis_of = lambda k: (k // 4) % 2 == 0 and k % 4 == 1           # noqa: E731  (groups 0, 2, 4, 6, 8 of the ten)
    outs = [torch.full((N_UNITS, 65, 26, 2), float("nan"), device=w["dev"]) for _ in range(N_STEPS)]
    for k, s in enumerate(w["steps"]):
        observe_step(ctx, s, outs[k], dis_of(k))
    st1 = ctx.stats()
    torch.cuda.synchronize()
    check_outputs(w, outs, dis_of)
    n_read_groups = 5
    assert st1["ring_events"] - st0["ring_events"] >= n_read_groups
    # ring groups 1, 3, 1, 3, 1 in turn: the second and third visit of group 1 and the second of group 3 find a record
    assert st1["ring_waits"] - st0["ring_waits"] >= 3
    # ... and exactly those: the rule is "an event exists only for groups whose slots the device read"
    assert st1["ring_events"] - st0["ring_events"] == n_read_groups and st1["ring_waits"] - st0["ring_waits"] == 3
    # alternating steps (a table step, a distractor step, ...): every group is read
    st1 = ctx.stats()
    for k, s in enumerate(w["steps"]):
        observe_step(ctx, s, outs[k], k % 2 == 1)
    st2 = ctx.stats()
    torch.cuda.synchronize()
    check_outputs(w, outs, lambda k: k % 2 == 1)
    assert st2["ring_events"] - st1["ring_events"] >= N_STEPS // 4


@pytest.mark.gpu
def test_new_key_and_stream_change_inside_a_group(world):
    import torch
    w = world
    ctx = make_ctx(w)
    st0 = warm_up(ctx, w)
    outs = [torch.full((N_UNITS, 65, 26, 2), float("nan"), device=w["dev"]) for _ in range(N_STEPS)]
    extra = torch.empty((1, 65, 26, 2), device=w["dev"])
    for k, s in enumerate(w["steps"]):
        observe_step(ctx, s, outs[k])
        if k == 5:                                                # third slot of a group of table steps: a new sound key
            ctx.observe([2], [0], [4], spectrogram_out=extra)     # (its window rows are uploaded from the slot)
            assert ctx.stats()["misses"] == st0["misses"] + 1
    st1 = ctx.stats()
    torch.cuda.synchronize()
    check_outputs(w, outs, lambda k: False)
    assert st1["ring_events"] - st0["ring_events"] == 1           # that group, and no other
    a = O.compute_audiogoal(w["src"][2], w["rirs"][4], SR)
    assert O.relerr(extra[0].cpu().numpy(), O.compute_spectrogram(a.astype(np.float32))) <= 1e-4
    # a stream change inside a group: the open group is closed on the OLD stream - with an event when the device read it
    ctx2 = make_ctx(w)
    st0 = warm_up(ctx2, w)
    side = torch.cuda.Stream(device=w["dev"])
    outs = [torch.full((N_UNITS, 65, 26, 2), float("nan"), device=w["dev"]) for _ in range(N_STEPS)]
    dis_of = lambda k: k == 8                                     # noqa: E731
    torch.cuda.synchronize()
    for k, s in enumerate(w["steps"]):
        on_side = 9 <= k < 22 or k >= 30                          # changes at k = 9 (behind the read step), 22 and 30 (table steps)
        with torch.cuda.stream(side if on_side else torch.cuda.current_stream()):
            observe_step(ctx2, s, outs[k], dis_of(k))
        if k == 9:
            assert ctx2.stats()["ring_events"] - st0["ring_events"] == 1   # recorded at the change, two slots into the group
    st1 = ctx2.stats()
    torch.cuda.synchronize()
    check_outputs(w, outs, dis_of)
    assert st1["ring_events"] - st0["ring_events"] == 1           # the groups closed at k = 22 and 30 held table steps only


@pytest.mark.gpu
def test_overlap_mode_equals_single_stream_over_the_same_steps(world):
    """two lanes (the overlap mode keeps the old rule: every lane records its share of every group)"""
    import torch
    w = world
    ctx = make_ctx(w)
    ctx.set_overlap(2)
    dis_of = lambda k: k % 5 == 2                                 # noqa: E731
    outs = [torch.full((N_UNITS, 65, 26, 2), float("nan"), device=w["dev"]) for _ in range(N_STEPS)]
    for k, s in enumerate(w["steps"]):
        observe_step(ctx, s, outs[k], dis_of(k))
    ctx.join()
    st = ctx.stats()
    torch.cuda.synchronize()
    check_outputs(w, outs, dis_of)                                # (= the stateless render = the single-stream context's)
    assert st["ring_events"] >= 2 * (N_STEPS // 4) and st["ring_waits"] >= N_STEPS // 4
    single = make_ctx(w)                                          # the single-stream context over the same 40 steps
    outs1 = [torch.full((N_UNITS, 65, 26, 2), float("nan"), device=w["dev"]) for _ in range(N_STEPS)]
    for k, s in enumerate(w["steps"]):
        observe_step(single, s, outs1[k], dis_of(k))
    torch.cuda.synchronize()
    for k in range(N_STEPS):
        assert torch.equal(outs1[k], outs[k]), k
