"""The one-launch log-mel forms over half-precision time-domain RIR rows on the host-compiled kernels
(tests/obs_logmel_rir16_host.cpp on the host-sim fibers): k_conv<.., MEL, HALF> loop-free and loop, k_conv<.., MEL, HALF, RBK>,
k_obs_rows<.., MEL, .., ROWS16> and k_obs_blocks<.., MEL, .., ROWS16>.

A/B: each new instantiation against its fp32 log-mel sibling fed float(q) * scale, on identical parameters.  The dequantised
sample is exact in fp32 and the arithmetic behind the load is the same code, so the expected figure is 0.0 (measured: 0.0 on every
case and output - profiles/r12/NOTES.md); every figure is printed.  Asserted with the project's existing bounds only: waveform and
pooled spectrogram <= 2e-6 of the reference's peak (each fp32 path is held to <= 1e-6 of peak against float64 and the inputs are
identical), log-mel under the log-mel rule of tests/test_logmel.py (1e-4 of the unit's largest value).

Model: live units against oracle.compute_logmel of rir16_ref.model_audiogoal(quant=True) (zero from n_valid on) under the log-mel
rule; the pooled spectrogram <= 1e-4.  Silent units and units on the empty entry: one value, log(eps), in every band and frame,
bit-exact +0 in the waveform and the pooled spectrogram.

Banks, sources, plan and model: tests/test_rir16_host.py and tests/test_rir16_rows_host.py (imported, never written to); buckets:
the 12-unit scene of tests/spec_buckets_ref.py.  Every output is pre-filled with NaN, the row kernel's stash too."""
import ctypes

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
import spec_buckets_ref as B
import test_rir16_host as T
import test_rir16_rows_host as TR
from test_logmel import TOL as MEL_TOL

hs = pytest.importorskip("hostsim.hs")

BOUND = T.BOUND              # 2e-6 of peak: waveform and pooled spectrogram, A/B
BUDGET = T.BUDGET            # 1e-4: the model
EPS = 1e-6
NO_DISTRACTOR, FIRST_BUCKET = 1, 4
LOOP_FREE, LOOP, RBK_LOOP, ROWS, BLOCKS = range(5)
SR = T.SR


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("obs_logmel_rir16", tmp_path_factory.mktemp("obs_logmel_rir16"))
    L = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.hs_obs_logmel_rir16.argtypes = [ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float, ci, ci, ci,
                                      ci, ci, ci, ci, vp]
    L.hs_source_windows.argtypes = [vp, vp, vp, ci]
    return L


@pytest.fixture(scope="module")
def banks():
    return T.make_banks()


@pytest.fixture(scope="module")
def world():
    """the bucket scene: per bucket its halves, scales and dequantised rows"""
    sc = B.scene()
    qs = [R.quantise(rows) for rows in sc["rows"]]
    sc["q"] = [np.ascontiguousarray(q) for q, _ in qs]
    sc["s"] = [np.ascontiguousarray(s, np.float32) for _, s in qs]
    sc["deq"] = [np.ascontiguousarray(R.dequantise(q, s)) for q, s in qs]
    return sc


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


_MEL = {}


def mel_bank(sr, n_mels):
    if (sr, n_mels) not in _MEL:
        start, w, max_len = P.mel_filterbank_sparse(sr, n_mels)
        _MEL[(sr, n_mels)] = (np.ascontiguousarray(start, np.int32), np.ascontiguousarray(w, np.float32), int(max_len))
    return _MEL[(sr, n_mels)]


def launch(lib, half, kernel, srcs, q, s, deq, first, caps, lens, units, sr, *, n_valid=None, n_mels=64, pad_mode=0, outputs="all",
           flags=0, wgs=2, parts_log2=0, expect=None):
    """one launch of the half (1) or the fp32 (0) form -> dict(mel, wave | None, sgram | None)"""
    n_valid = sr if n_valid is None else n_valid
    wd, desc = T.plan(srcs, units, max(caps), n_valid)
    flat = np.concatenate([np.asarray(x, np.float32) for x in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    n = len(units)
    start, w, max_len = mel_bank(sr, n_mels)
    mel = np.full((n,) + P.logmel_shape(sr, n_mels), np.nan, np.float32)
    wave = np.full((n, 2, sr), np.nan, np.float32) if outputs == "all" else None
    sg = np.full((n,) + P.spectrogram_shape(sr), np.nan, np.float32) if outputs == "all" else None
    first = np.asarray(first, np.int32)
    caps = np.asarray(caps, np.int32)
    lens = np.ascontiguousarray(lens, np.int32)
    taken = ctypes.c_int(-1)
    rc = lib.hs_obs_logmel_rir16(int(half), kernel, spec.ctypes.data, _ptrs(q if half else deq), _ptrs(s) if half else None,
                                 first.ctypes.data, caps.ctypes.data, len(caps), lens.ctypes.data, desc.ctypes.data,
                                 wave.ctypes.data if wave is not None else None, sg.ctypes.data if sg is not None else None,
                                 mel.ctypes.data, start.ctypes.data, w.ctypes.data, n_mels, max_len, EPS, n, n_valid, sr, pad_mode, wgs,
                                 parts_log2, flags, ctypes.addressof(taken))
    assert rc == 0, rc
    assert expect is None or taken.value == expect, (taken.value, expect)
    for name, a in (("mel", mel), ("wave", wave), ("sgram", sg)):
        assert a is None or not np.isnan(a).any(), (name, half)
    return dict(mel=mel, wave=wave, sgram=sg)


def single(lib, half, kernel, b, units, sr, **kw):
    """a launch on one allocation (a bank of tests/test_rir16_host.make_banks)"""
    return launch(lib, half, kernel, T.sources(sr), [b["q"]], [b["s"]], [b["deq"]], [0], [b["cap"]], b["lens"], units, sr, **kw)


def ab(h, f, label, live, quiet):
    """half against fp32(dequantised): the A/B bounds, the quiet units' exact values"""
    for name in ("wave", "sgram"):
        if h[name] is None:
            continue
        peak = np.abs(f[name]).max()
        err = np.abs(h[name].astype(np.float64) - f[name].astype(np.float64)).max() / peak
        print(f"[obs_logmel_rir16_host] {label} {name}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        assert peak > 0 and err <= BOUND, (label, name, err)
        for k in quiet:
            assert not h[name][k].view(np.uint32).any(), (label, name, k)          # bit-exact +0
        assert all(np.abs(h[name][k]).max() > 0 for k in live), (label, name)
    worst = 0.0
    for k in range(len(h["mel"])):
        top = np.abs(f["mel"][k]).max()
        err = np.abs(h["mel"][k].astype(np.float64) - f["mel"][k].astype(np.float64)).max() / top
        worst = max(worst, err)
        assert err <= MEL_TOL, (label, k, err)
    print(f"[obs_logmel_rir16_host] {label} logmel: max over units of |half - fp32(dequantised)| / unit's largest = {worst:.3e}")
    for k in quiet:                                                               # one value, log(eps), as the sibling writes it
        assert np.unique(h["mel"][k]).size == 1 and np.allclose(h["mel"][k], np.log(EPS), rtol=1e-6, atol=0), (label, k)
        assert h["mel"][k].tobytes() == f["mel"][k].tobytes(), (label, k)


def against_model(h, ref_waves, label, live, sr, n_mels=64, pad_mode=0, n_valid=None):
    """live units: log-mel rule against the oracle's log-mel of the quantised float64 model; pooled spectrogram <= 1e-4"""
    pad = "reflect" if pad_mode == 0 else "constant"
    for k in live:
        wave = np.array(ref_waves[k])
        if n_valid is not None:
            wave[:, n_valid:] = 0.0
        ref = O.compute_logmel(wave, sr, n_mels, EPS, pad_mode=pad)
        err = np.abs(h["mel"][k] - ref).max() / np.abs(ref).max()
        print(f"[obs_logmel_rir16_host] {label} unit {k} logmel: half kernel vs quantised float64 model = {err:.3e}")
        assert h["mel"][k].shape == ref.shape and err <= MEL_TOL, (label, k, err)
        if h["sgram"] is not None:
            err = O.relerr(h["sgram"][k], O.compute_spectrogram(wave, pad_mode=pad))
            print(f"[obs_logmel_rir16_host] {label} unit {k} sgram: half kernel vs quantised float64 model = {err:.3e}")
            assert err <= BUDGET, (label, k, err)
        if h["wave"] is not None:
            err = O.relerr(h["wave"][k], wave)
            assert err <= BUDGET, (label, k, err)


_MODELS = {}


def model16(b, name, units, n_valid=None):
    key = (name, n_valid, len(units))
    if key not in _MODELS:
        m = T.model(T.sources(SR), b, units, SR, SR if n_valid is None else n_valid)
        m.setflags(write=False)
        _MODELS[key] = m
    return _MODELS[key]


# ---- one-block rows, one allocation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,pad_mode,outputs", [(64, 0, "all"), (40, 1, "mel"), (64, 1, "all"), (40, 0, "mel")])
def test_loop_free(lib, banks, n_mels, pad_mode, outputs):
    """SIMPLE_UNITS: plain | silent | the empty entry | ears 2^35 apart | the odd length - SS_FLAG_NO_DISTRACTOR, cap <= kB"""
    b = banks["small"]
    kw = dict(n_mels=n_mels, pad_mode=pad_mode, outputs=outputs, flags=NO_DISTRACTOR, expect=LOOP_FREE)
    h, f = single(lib, 1, 0, b, T.SIMPLE_UNITS, SR, **kw), single(lib, 0, 0, b, T.SIMPLE_UNITS, SR, **kw)
    label = f"loop-free mels {n_mels} pad {pad_mode} {outputs}"
    ab(h, f, label, live=[0, 3, 4], quiet=[1, 2])
    against_model(h, model16(b, "small", T.SIMPLE_UNITS), label, [0, 3, 4], SR, n_mels, pad_mode)


@pytest.mark.parametrize("outputs", ["all", "mel"])
def test_loop_with_a_distractor_of_another_entry(lib, banks, outputs):
    b = banks["small"]
    units = [dict(sound=0, t0=0, rir=3, dis_sound=1, dis_rir=2), dict(rir=-1), dict(sound=1, t0=0, rir=0)]
    kw = dict(outputs=outputs, flags=0, expect=LOOP)
    h, f = single(lib, 1, 0, b, units, SR, **kw), single(lib, 0, 0, b, units, SR, **kw)
    ab(h, f, f"loop + distractor {outputs}", live=[0, 2], quiet=[1])
    against_model(h, model16(b, "small", units), f"loop + distractor {outputs}", [0, 2], SR)


def test_loop_three_rir_blocks(lib, banks):
    """the 40 000-sample bank: three RIR blocks, each with a window (the 3-s clip on its steady branch); 40 bands, constant pad"""
    b = banks["long"]
    t0 = P.window_start_sim(3 * SR, SR, 2)
    units = [dict(sound=2, t0=t0, rir=0), dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=0), dict(rir=-1)]
    for n_mels, pad_mode, outputs, flags in ((64, 0, "all", 0), (40, 1, "mel", 0)):
        kw = dict(n_mels=n_mels, pad_mode=pad_mode, outputs=outputs, flags=flags, expect=LOOP)
        h, f = single(lib, 1, 0, b, units, SR, **kw), single(lib, 0, 0, b, units, SR, **kw)
        label = f"loop, 3 RIR blocks, mels {n_mels} pad {pad_mode} {outputs}"
        ab(h, f, label, live=[0, 1], quiet=[2])
        against_model(h, model16(b, "long", units), label, [0, 1], SR, n_mels, pad_mode)


@pytest.mark.parametrize("flags,expect", [(NO_DISTRACTOR, LOOP_FREE), (0, LOOP)], ids=["loop-free", "loop"])
def test_n_valid_4000_of_16000(lib, banks, flags, expect):
    """pooled blocks behind n_valid: log(eps) in every band, exact zeros in the pooled spectrogram and the waveform"""
    b = banks["small"]
    kw = dict(n_valid=4000, flags=flags, expect=expect)
    h, f = single(lib, 1, 0, b, T.SIMPLE_UNITS, SR, **kw), single(lib, 0, 0, b, T.SIMPLE_UNITS, SR, **kw)
    ab(h, f, f"n_valid 4000 flags {flags}", live=[0, 3, 4], quiet=[1, 2])
    against_model(h, model16(b, "small", T.SIMPLE_UNITS, 4000), f"n_valid 4000 flags {flags}", [0, 3, 4], SR, n_valid=4000)
    live = P.live_pooled_blocks(4000, SR)
    assert 0 < live < h["sgram"].shape[2]
    assert not h["wave"][:, :, 4000:].view(np.uint32).any() and not h["sgram"][:, :, live:].view(np.uint32).any()
    assert np.allclose(h["mel"][0][:, 4 * live:], np.log(EPS), rtol=1e-6, atol=0)


# ---- length buckets -------------------------------------------------------------------------------------------------------------
def bucketed(lib, half, sc, units, **kw):
    return launch(lib, half, 0, sc["srcs"], sc["q"], sc["s"], sc["deq"], B.FIRST, B.CAPS, sc["lens"], units, SR, **kw)


@pytest.mark.parametrize("outputs", ["all", "mel"])
def test_buckets_twelve_unit_scene(lib, world, outputs):
    units = world["units"]
    h = bucketed(lib, 1, world, units, outputs=outputs, expect=RBK_LOOP)
    f = bucketed(lib, 0, world, units, outputs=outputs, expect=RBK_LOOP)
    quiet = [k for k, u in enumerate(units) if u.get("rir", -1) < 0 or u["rir"] == B.EMPTY]
    live = [k for k in range(len(units)) if k not in quiet]
    ab(h, f, f"buckets, 12 units, {outputs}", live, quiet)
    refs = {}
    for k in live:                                                          # the model fed the bank's own halves and scales
        u = units[k]
        out = np.zeros((2, SR))
        for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
            bk = B.bucket_of(g)
            out += R.model_audiogoal(world["srcs"][snd], world["deq"][bk][g - B.FIRST[bk]][:, :int(world["lens"][g])], t0, SR, quant=False)
        refs[k] = out
    against_model(h, refs, f"buckets, 12 units, {outputs}", live, SR)


def test_first_bucket_launch_is_the_single_allocation_launch_bit_for_bit(lib, world):
    units = [dict(sound=0, t0=0, rir=0), dict(sound=1, t0=0, rir=2), dict(sound=0, t0=0, rir=B.EMPTY), dict(rir=-1),
             dict(sound=1, t0=4000, rir=0)]
    one = launch(lib, 1, 0, world["srcs"], world["q"][:1], world["s"][:1], world["deq"][:1], B.FIRST[:1], B.CAPS[:1], world["lens"],
                 units, SR, flags=NO_DISTRACTOR, expect=LOOP_FREE)
    fb = bucketed(lib, 1, world, units, flags=NO_DISTRACTOR | FIRST_BUCKET, expect=LOOP_FREE)
    for name in ("mel", "wave", "sgram"):
        assert fb[name].tobytes() == one[name].tobytes(), name
    loop = bucketed(lib, 1, world, units, flags=0, expect=RBK_LOOP)          # ... and agrees with the bucketed loop kernel
    ab(fb, loop, "first bucket against the bucketed loop kernel", live=[0, 1, 4], quiet=[2, 3])


# ---- rows of 2 or 3 blocks (one allocation) -------------------------------------------------------------------------------------
def rows_case(lib, b, name, sr, units, live, quiet, kernel, label, **kw):
    h, f = single(lib, 1, kernel, b, units, sr, **kw), single(lib, 0, kernel, b, units, sr, **kw)
    ab(h, f, label, live, quiet)
    against_model(h, TR.model_of(b, name, sr, units), label, live, sr, kw.get("n_mels", 64), kw.get("pad_mode", 0))
    return h


@pytest.mark.parametrize("parts_log2", [0, 1])
def test_obs_blocks_44100(lib, banks, parts_log2):
    """44 100-sample rows over the 40 000-sample bank (three RIR blocks), three units including a silent one: one workgroup per
    output block (and part)"""
    sr = 44100
    outputs = "all" if parts_log2 == 0 else "mel"
    rows_case(lib, banks["long"], "long", sr, TR.units3(sr), TR.LIVE3, TR.ZERO3, 2, f"blocks 44100 parts {parts_log2} {outputs}",
              parts_log2=parts_log2, outputs=outputs, expect=BLOCKS)


def test_obs_rows_44100(lib, banks):
    sr = 44100
    h = rows_case(lib, banks["long"], "long", sr, TR.units3(sr), TR.LIVE3, TR.ZERO3, 1, "rows 44100 wgs 2", wgs=2, expect=ROWS)
    m = rows_case(lib, banks["long"], "long", sr, TR.units3(sr), TR.LIVE3, TR.ZERO3, 1, "rows 44100 mel only, 40 bands, constant",
                  wgs=3, outputs="mel", n_mels=40, pad_mode=1, expect=ROWS)
    assert h["mel"].shape[1] == 64 and m["mel"].shape[1] == 40


def test_two_blocks_20000(lib, banks):
    """20 000-sample rows over the 16 000-sample bank, every kind of unit, through both row kernels"""
    b = banks["small"]
    rows_case(lib, b, "small", 20000, TR.UNITS2, TR.LIVE2, TR.ZERO2, 1, "rows 20000 wgs 2", wgs=2, expect=ROWS)
    rows_case(lib, b, "small", 20000, TR.UNITS2, TR.LIVE2, TR.ZERO2, 2, "blocks 20000", outputs="mel", expect=BLOCKS)
