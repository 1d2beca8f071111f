"""The half-precision spectral RIR bank on the host-compiled kernels (tests/spec_half_host.cpp on the host-sim fibers).

Quantiser: k_stage_spectra16 (both staging layouts, and the planar-bank form of ss_rir_spectra16_f32) against the numpy rule
(tests/spec_half_ref.py) applied to hs_rir_spectra's fp32 block spectra of the same rows: equal as fp16 VALUES (+0 == -0), the
scales exactly, entries not named untouched.

Consumer: k_conv_spec<.., HALF> against the fp32 instantiation of the same template fed float(q) * hscale, for the unfused
loop-free form (also through the unit table), the unfused loop form (3 RIR blocks + a distractor term), the fused form and the
log-mel form.  Bound 2e-6 of the reference's peak: each fp32 path is held to <= 1e-6 of peak against float64 by the project's
parity record and the inputs are identical; measured 0.0 on every form (the dequantised value is exact in fp32, the arithmetic
behind it is the same instructions) - profiles/r7/NOTES.md."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_half_ref as R

hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 16000
LENGTHS = [0, 1, 15999, 16000, 16384, 16385, 40000]
CAPS = [16000, 49152]
BOUND = 2e-6
EPS = 1e-6


@pytest.fixture(scope="module")
def half_lib(tmp_path_factory):
    so = hs.build_driver("spec_half", tmp_path_factory.mktemp("spec_half"))
    lib = ctypes.CDLL(so)
    vp, ci, ll, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    lib.hs_stage_spectra16.argtypes = [vp, ll, ci, vp, vp, ci, vp, vp, ci, vp]
    lib.hs_rir_spectra16.argtypes = [vp, vp, vp, ci, ll, ci, ci]
    lib.hs_conv_spec_ab.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, ci, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    lib.hs_rir_spectra.argtypes = [vp, vp, ci, ll, ci, ci]
    return lib


# ---- quantiser ----------------------------------------------------------------------------------------------------------------
def _rows(cap, seed):
    """one row per length in LENGTHS (clamped to cap): random samples (signed zeros included) up to the length, GARBAGE beyond it
    in the staging block; row 3 scaled by 32768 (an integer-scaled file), row 4 by 1e-6"""
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.asarray(LENGTHS, np.int32), cap)
    planar = rng.standard_normal((len(LENGTHS), 2, cap)).astype(np.float32)
    planar[:, :, ::97] = -0.0
    planar[3] *= np.float32(32768.0)
    planar[4] *= np.float32(1e-6)
    garbage = planar.copy()
    for i, n in enumerate(lens):
        planar[i, :, n:] = 0.0
        garbage[i, :, n:] = np.nan
    return planar, garbage, np.asarray(LENGTHS, np.int32), lens


def _fp32_spectra(lib, planar):
    """hs_rir_spectra (k_source_windows, scale 1) of planar rows: [R, 2, hb, SPEC_FLOATS]"""
    n, _, cap = planar.shape
    hb = P.ceil_div(cap, P.KB)
    out = np.zeros((n, 2, hb, P.SPEC_FLOATS), np.float32)
    bank = np.ascontiguousarray(planar)
    assert lib.hs_rir_spectra(bank.ctypes.data, out.ctypes.data, n, 2 * cap, cap, cap) == 0
    return out


def _same_halves(got, want):
    """equal as fp16 values: bit-equal except that +0 and -0 compare equal; no NaN anywhere"""
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape
    assert not np.isnan(got).any() and not np.isnan(want).any()
    return np.array_equal(got, want)


@pytest.mark.parametrize("cap", CAPS)
def test_stage_spectra16_equals_numpy_quantisation(half_lib, cap):
    planar, garbage, lens_in, lens = _rows(cap, cap)
    want_q, want_s = R.quantise(_fp32_spectra(half_lib, planar))
    assert np.abs(want_q.astype(np.float32)).max() <= 32768.0          # the scaled maximum lies in [2^14, 2^15]
    n = planar.shape[0]
    hb = P.ceil_div(cap, P.KB)
    slots = np.asarray([2 * i + 1 for i in range(n)], np.int32)[::-1].copy()      # scattered, out of order
    entries = int(slots.max()) + 2
    for layout in ("wav", "planar"):
        staged = np.ascontiguousarray(garbage.transpose(0, 2, 1) if layout == "wav" else garbage)
        hspec16 = np.zeros((entries, 2, hb, P.SPEC_FLOATS), np.float16)   # a bank's arrays are zero-initialised
        hscale = np.zeros((entries, 2, hb), np.float32)
        bank_len = np.full((entries,), -5, np.int32)
        rc = half_lib.hs_stage_spectra16(staged.ctypes.data, 2 * cap, int(layout == "planar"), slots.ctypes.data, lens_in.ctypes.data,
                                         n, hspec16.ctypes.data, hscale.ctypes.data, hb, bank_len.ctypes.data)
        assert rc == 0
        for i in range(n):
            assert _same_halves(hspec16[slots[i]], want_q[i]), (layout, cap, int(lens[i]))
            assert hscale[slots[i]].tobytes() == want_s[i].tobytes(), (layout, cap, int(lens[i]), hscale[slots[i]], want_s[i])
            assert bank_len[slots[i]] == lens[i]
        empty = slots[0 if lens[0] == 0 else list(lens).index(0)]         # the empty row: halves +0, scale 1
        assert not hspec16[empty].view(np.uint16).any() and (hscale[empty] == 1.0).all()
        others = np.setdiff1d(np.arange(entries), slots)
        assert not hspec16[others].view(np.uint16).any() and not hscale[others].any() and (bank_len[others] == -5).all()


@pytest.mark.parametrize("cap", [16000, 40001])
def test_rir_spectra16_of_a_planar_bank(half_lib, cap):
    """the planar-bank form (ss_rir_spectra16_f32): entry r to entry r, even and odd row capacities (8-byte and sample-wise loads)"""
    rng = np.random.default_rng(cap)
    bank = rng.standard_normal((3, 2, cap)).astype(np.float32)
    bank[1] = 0.0
    bank[2, :, 9000:] = 0.0
    want_q, want_s = R.quantise(_fp32_spectra(half_lib, bank))
    hb = P.ceil_div(cap, P.KB)
    hspec16 = np.zeros((3, 2, hb, P.SPEC_FLOATS), np.float16)
    hscale = np.zeros((3, 2, hb), np.float32)
    assert half_lib.hs_rir_spectra16(bank.ctypes.data, hspec16.ctypes.data, hscale.ctypes.data, 3, 2 * cap, cap, cap) == 0
    assert _same_halves(hspec16, want_q) and hscale.tobytes() == want_s.tobytes()
    assert (hscale[1] == 1.0).all() and not hspec16[1].view(np.uint16).any()


def test_quantiser_rule_on_known_values():
    """the numpy rule itself: exponent edges, round-to-nearest-even, the all-zero block"""
    v = np.zeros((4, 8), np.float32)
    v[0, :3] = [1.0, -0.75, 2.0 ** -20]          # mx = 1 = 2^0 in [2^0, 2^1): e = 1, scale 2^-14, q = v * 2^14
    v[1, :2] = [0.999, 0.5]                      # mx in [2^-1, 2^0): e = 0, q = v * 2^15
    v[2, :3] = [32768.0 * 3, 2049.0 * 8, 2051.0 * 8]     # e = 17, q = v / 4: 24576, 4098 (a tie: to even 4096), 4102 (tie: 4104)
    q, s = R.quantise(v)
    assert s.tolist() == [2.0 ** -14, 2.0 ** -15, 4.0, 1.0]
    assert q[0, :3].astype(np.float64).tolist() == [16384.0, -12288.0, 2.0 ** -6]
    assert q[1, 1] == 16384.0 and 2 ** 14 <= float(q[1, 0]) <= 2 ** 15
    assert q[2, :3].astype(np.float64).tolist() == [24576.0, 4096.0, 4104.0]
    assert not q[3].view(np.uint16).any()
    assert np.array_equal(R.dequantise(q, s)[0, :2], v[0, :2])


# ---- consumer -----------------------------------------------------------------------------------------------------------------
def _plan(sources, units, cap, n_valid):
    """window descriptors + unit descriptors of a launch, as hostsim.hs.run plans them"""
    nbh_max = max(1, P.ceil_div(cap, P.KB))
    nby = max(1, P.ceil_div(n_valid, P.KB))
    offs = np.cumsum([0] + [len(s) for s in sources])
    cache, rows = {}, []

    def slot_of(sound, t0):
        if (sound, t0) not in cache:
            ws = P.plan_window_set(len(sources[sound]), t0, nbh_max, nby, False)
            cache[(sound, t0)] = (sum(len(r) for r in rows), ws)
            rows.append(P.window_desc_rows(ws, int(offs[sound]), len(sources[sound]), False))
        return cache[(sound, t0)]

    desc = np.zeros((len(units), 8), np.int32)
    for n, u in enumerate(units):
        if u.get("rir", -1) < 0:
            desc[n] = P.unit_desc_row()
            continue
        s0, ws = slot_of(u["sound"], u["t0"])
        if u.get("dis_rir", -1) >= 0:
            d0, dws = slot_of(u["dis_sound"], 0)
            desc[n] = P.unit_desc_row(u["rir"], s0, ws, u["dis_rir"], d0, dws)
        else:
            desc[n] = P.unit_desc_row(u["rir"], s0, ws)
    wd = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), np.int32), np.int32)
    return wd, desc


@pytest.fixture(scope="module")
def scene(half_lib):
    """sources, a one-block bank and a three-block bank (every block audible), their fp32 spectra and the half form of those"""
    rng = np.random.default_rng(11)
    srcs = list(O.synth_sources(rng, SR, k=2, seconds=1)) + [O.synth_sources(rng, SR, k=1, seconds=3)[0]]
    lens = [SR, 9000, 0]
    bank = np.zeros((len(lens), 2, SR), np.float32)
    for i, n in enumerate(lens):
        if n:
            bank[i, :, :n] = O.synth_rir(rng, SR, length=n, n=1)[0]
    long_len = 40000
    long_bank = np.zeros((2, 2, long_len), np.float32)
    long_bank[0] = O.synth_rir_blocks(rng, SR, long_len, n=1)[0]
    long_bank[1, :, :9000] = bank[1, :, :9000]
    out = {"srcs": srcs, "long_rows": long_bank[0].copy()}
    for name, b, ln in (("one", bank, lens), ("long", long_bank, [long_len, 9000])):
        f32 = _fp32_spectra(half_lib, b)
        q, s = R.quantise(f32)
        out[name] = dict(cap=b.shape[2], lens=np.asarray(ln, np.int32), q=np.ascontiguousarray(q), s=np.ascontiguousarray(s),
                         deq=np.ascontiguousarray(R.dequantise(q, s)))
    return out


def _ab(lib, scene, which, units, fuse, simple, mel, use_tab=False, n_mels=64):
    """run the HALF instantiation and the fp32 one over the dequantised spectra -> {name: (half, fp32)} of every output"""
    b = scene[which]
    srcs = scene["srcs"]
    wd, desc = _plan(srcs, units, b["cap"], SR)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    hb = P.ceil_div(b["cap"], P.KB)
    start, w, max_len = P.mel_filterbank_sparse(SR, n_mels)
    start, w = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(w, np.float32)
    n = len(units)
    t_frames, t4 = 1 + SR // 160, P.spectrogram_shape(SR)[1]
    res = {}
    for half in (1, 0):
        wave = np.full((n, 2, SR), np.nan, np.float32)
        sg = np.full((n, 65, t4, 2), np.nan, np.float32) if fuse else None
        lm = np.full((n, n_mels, t_frames, 2), np.nan, np.float32) if mel else None
        bankp = b["q"].ctypes.data if half else b["deq"].ctypes.data
        rc = lib.hs_conv_spec_ab(half, int(fuse), int(simple), int(mel), int(use_tab), spec.ctypes.data, bankp,
                                 b["s"].ctypes.data if half else None, b["lens"].ctypes.data, desc.ctypes.data, wave.ctypes.data,
                                 sg.ctypes.data if fuse else None, lm.ctypes.data if mel else None, start.ctypes.data, w.ctypes.data,
                                 n_mels, max_len, EPS, n, hb, SR, SR, 0)
        assert rc == 0, rc
        for name, a in (("wave", wave), ("sgram", sg), ("logmel", lm)):
            if a is not None:
                assert not np.isnan(a).any(), (name, half)
                res.setdefault(name, []).append(a)
    return res


def _check(res, label, live):
    for name, (h, f) in res.items():
        peak = np.abs(f).max()
        err = np.abs(h.astype(np.float64) - f.astype(np.float64)).max() / peak
        print(f"[spec_half_host] {label} {name}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        assert err <= BOUND, (label, name, err)
        assert peak > 0 and all(np.abs(f[k]).max() > 0 for k in live)


ONE_BLOCK_UNITS = [dict(sound=0, t0=0, rir=0), dict(rir=-1), dict(sound=1, t0=0, rir=2), dict(sound=1, t0=0, rir=1)]


@pytest.mark.parametrize("use_tab", [False, True], ids=["desc", "unit_table"])
def test_half_consumer_unfused_simple(half_lib, scene, use_tab):
    res = _ab(half_lib, scene, "one", ONE_BLOCK_UNITS, fuse=False, simple=True, mel=False, use_tab=use_tab)
    _check(res, f"unfused SIMPLE tab={int(use_tab)}", live=[0, 3])
    assert not res["wave"][0][1].any() and not res["wave"][0][2].any()            # silent / empty RIR: exact zeros


def test_half_consumer_unfused_loop_three_blocks_and_distractor(half_lib, scene):
    t0 = P.window_start_sim(3 * SR, SR, 2)
    units = [dict(sound=2, t0=t0, rir=0), dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=0), dict(rir=-1)]
    res = _ab(half_lib, scene, "long", units, fuse=False, simple=False, mel=False)
    _check(res, "unfused loop (3 blocks + distractor)", live=[0, 1])
    # every RIR block of unit 0 is audible in the result: the half path agrees with the quantised model, which needs all three
    ref = R.model_audiogoal(scene["srcs"][2], scene["long_rows"], t0, SR)
    err = O.relerr(res["wave"][0][0], ref)                # (the model rounds its fp64 spectra, the kernel its fp32 ones: ~1e-5)
    print(f"[spec_half_host] unfused loop, 3 blocks: half kernel vs quantised model = {err:.3e}")
    assert err <= 1e-4                                    # the project's parity budget; a dropped block would be ~1e-1


def test_half_consumer_fused(half_lib, scene):
    res = _ab(half_lib, scene, "one", ONE_BLOCK_UNITS, fuse=True, simple=True, mel=False)
    _check(res, "fused SIMPLE", live=[0, 3])
    assert not res["sgram"][0][1].any() and not res["sgram"][0][2].any()
    res = _ab(half_lib, scene, "one", ONE_BLOCK_UNITS + [dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=0)], fuse=True, simple=False,
              mel=False)
    _check(res, "fused loop", live=[0, 3, 4])


def test_half_consumer_logmel(half_lib, scene):
    for simple, units in ((True, ONE_BLOCK_UNITS), (False, ONE_BLOCK_UNITS + [dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=0)])):
        res = _ab(half_lib, scene, "one", units, fuse=True, simple=simple, mel=True)
        _check(res, f"MEL simple={int(simple)}", live=[0, 3])
        lm = res["logmel"][0]
        assert np.allclose(lm[1], np.log(EPS), rtol=1e-6) and np.allclose(lm[2], np.log(EPS), rtol=1e-6)


def test_model_matches_the_oracle_unquantised():
    """the overlap-save model of tests/spec_half_ref.py without its quantiser is the oracle's convolution (the issue: 2.8e-7 of
    peak); with it, the waveform moves by the format's error, 2.0-2.2e-4 of peak on these draws"""
    rng = np.random.default_rng(3)
    src = O.synth_sources(rng, SR, k=1, seconds=3)[0]
    worst, moved = 0.0, []
    for n in (3000, 16000, 40000):
        rir = O.synth_rir(rng, SR, length=n, n=1)[0]
        ref = O.compute_audiogoal(src, np.ascontiguousarray(rir.T), SR, audio_index=2)
        worst = max(worst, O.relerr(R.model_audiogoal(src, rir, 2 * SR, SR, quant=False), ref))
        moved.append(O.relerr(R.model_audiogoal(src, rir, 2 * SR, SR, quant=True), ref))
    print(f"[spec_half_host] model vs oracle {worst:.2e}; quantised model vs oracle {min(moved):.2e} .. {max(moved):.2e}")
    assert worst <= 1e-6
    assert 1e-5 < min(moved) and max(moved) < 1e-3
