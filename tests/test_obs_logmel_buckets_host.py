"""Log-mel forms of the fused observation kernels over LENGTH-BUCKETED banks, compiled for the host on the host-sim fibers
(tests/obs_logmel_buckets_host.cpp).

16 kHz, the scene of tests/spec_buckets_ref.py (four buckets of 1 / 2 / 3 / 5 blocks, 12 units), at 64 and at 40 bands:
k_conv<loop, MEL> over time-domain buckets, k_conv_spec<loop, MEL> over fp32 spectral buckets, k_conv_spec<.., MEL, HALF, HBK>.
  * fp32 forms against O.compute_logmel(O.compute_audiogoal(...)) under the project's rules: log-mel 1e-4 of the unit's largest
    value, pooled spectrogram 1e-4, waveform 1e-5;
  * the half form against the fp32 bucketed MEL instantiation fed float(q) * hscale, with the bounds of
    tests/test_spec_half_rows_host.py - 2e-6 of peak on waveform and spectrogram (taken per unit here, which asks more), 1e-4 of
    the unit's largest value on log-mel - and one unit per bucket against the float64 model fed the bank's own halves (1e-4): a
    block or scale read from the wrong bucket is ~1e-1;
  * silent and empty units: log(eps) in every band and exact zeros.

44.1 kHz, a four-bucket bank of caps 16 000 / 30 000 / 44 100 / 70 000 (1 / 2 / 3 / 5 blocks), 8 units (every bucket, a unit
whose two terms sit in different buckets, an empty entry, a silent unit): k_obs_rows<false | true, false, BUCKETS, MEL> with 3
persistent workgroups and with rows split over 2, k_obs_blocks<.., MEL> over the same buckets, and k_obs_rows with n_valid =
20 000 and no waveform buffer.
  * against the oracle, same rules;
  * against the single-allocation instantiation on a dense copy of the bank (every entry padded into one allocation at the
    largest cap): all three outputs EQUAL element for element - only addresses differ.
Every output is pre-filled with NaN, every unit is compared."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_buckets_ref as B
import spec_half_rows_ref as R

hs = pytest.importorskip("hostsim.hs")

from test_spec_half_host import _fp32_spectra, _plan  # noqa: E402  (the planner and the fp32 producer of the half-bank host test)

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-6
TOL = 1e-4            # log-mel (of the unit's largest value), pooled spectrogram, model fed the bank's halves
WAVE_TOL = 1e-5
AB = 2e-6             # half against fp32 fed the dequantised spectra, of peak
K_CONV, K_ROWS, K_BLOCKS = 0, 1, 2
ROWS, SPEC, HALF = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("obs_logmel_buckets", tmp_path_factory.mktemp("obs_logmel_buckets"))
    L = ctypes.CDLL(so)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.hs_obs_logmel_buckets.argtypes = [ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ctypes.c_float,
                                        ci, ci, ci, ci, ci, ci, ci]
    L.hs_source_windows.argtypes = [vp, vp, vp, ci]
    L.hs_rir_spectra.argtypes = [vp, vp, ci, ll, ci, ci]
    return L


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


_MEL = {}


def _mel_bank(sr, n_mels):
    if (sr, n_mels) not in _MEL:
        start, w, max_len = P.mel_filterbank_sparse(sr, n_mels)
        _MEL[(sr, n_mels)] = (np.ascontiguousarray(start, np.int32), np.ascontiguousarray(w, np.float32), int(max_len))
    return _MEL[(sr, n_mels)]


def _launch(lib, kernel, form, srcs, units, banks, scales, firsts, caps, lens, sr, *, n_valid=None, n_mels=64, want_sg=True,
            want_wave=True, wgs=3, parts_log2=0, pad_mode=0):
    """one launch over len(banks) buckets -> (logmel, spectrogram | None, waveform | None), pre-filled with NaN"""
    n_valid = sr if n_valid is None else n_valid
    wd, desc = _plan(srcs, units, max(caps), n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    start, w, max_len = _mel_bank(sr, n_mels)
    n = len(units)
    mel = np.full((n, n_mels, 1 + sr // 160, 2), np.nan, np.float32)
    sg = np.full((n,) + P.spectrogram_shape(sr), np.nan, np.float32) if want_sg else None
    wave = np.full((n, 2, sr), np.nan, np.float32) if want_wave else None
    first, cap = np.asarray(firsts, np.int32), np.asarray(caps, np.int32)
    rl = np.ascontiguousarray(lens, np.int32)
    no_dis = not any(u.get("dis_rir", -1) >= 0 for u in units)
    rc = lib.hs_obs_logmel_buckets(kernel, form, spec.ctypes.data, _ptrs(banks), _ptrs(scales) if scales is not None else None,
                                   first.ctypes.data, cap.ctypes.data, len(banks), rl.ctypes.data, desc.ctypes.data,
                                   wave.ctypes.data if want_wave else None, sg.ctypes.data if want_sg else None, mel.ctypes.data,
                                   start.ctypes.data, w.ctypes.data, n_mels, max_len, EPS, n, n_valid, sr, pad_mode, wgs, parts_log2,
                                   int(no_dis))
    assert rc == 0, rc
    assert not np.isnan(mel).any() and (sg is None or not np.isnan(sg).any())
    assert wave is None or not np.isnan(wave[:, :, :n_valid]).any()
    return mel, sg, wave


def _check_oracle(tag, sr, refs, mel, sg, wave, n_valid, n_mels):
    """refs[k]: the oracle's audiogoal [2, sr], or None for a unit that renders nothing (silent, empty RIR)"""
    for k, a in enumerate(refs):
        if a is None:
            assert np.unique(mel[k]).size == 1 and np.allclose(mel[k], np.log(EPS), rtol=1e-6, atol=0), (tag, k)   # one value: log(eps)
            assert sg is None or not sg[k].any(), (tag, k)
            assert wave is None or not wave[k, :, :n_valid].any(), (tag, k)
            continue
        a = np.array(a, np.float32)
        a[:, n_valid:] = 0.0
        ref = O.compute_logmel(a, sr, n_mels=n_mels, eps=EPS)
        e_mel = np.abs(mel[k] - ref).max() / np.abs(ref).max()
        e_sg = O.relerr(sg[k], O.compute_spectrogram(a)) if sg is not None else 0.0
        e_w = O.relerr(wave[k, :, :n_valid], a[:, :n_valid]) if wave is not None else 0.0
        print(f"[obs_logmel_buckets_host] {tag} unit {k}: log-mel {e_mel:.3e} spectrogram {e_sg:.3e} waveform {e_w:.3e}")
        assert e_mel <= TOL, (tag, k, e_mel)
        assert e_sg <= TOL, (tag, k, e_sg)
        assert e_w <= WAVE_TOL, (tag, k, e_w)


def _wav(row, n):
    return np.ascontiguousarray(row[:, :n].T)


# ---- 16 kHz: the 12-unit scene on the one-block loop kernels ------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(lib):
    sc = B.scene()
    f32 = [_fp32_spectra(lib, rows) for rows in sc["rows"]]
    qs = [R.quantise(f) for f in f32]
    sc["f32"] = f32
    sc["q"] = [np.ascontiguousarray(q) for q, _ in qs]
    sc["s"] = [np.ascontiguousarray(s) for _, s in qs]
    sc["deq"] = [np.ascontiguousarray(R.dequantise(q, s)) for q, s in qs]
    sc["perm"] = R.kernel_order(lambda rows: _fp32_spectra(lib, rows))
    refs = []
    for u in sc["units"]:
        g = u.get("rir", -1)
        if g < 0 or g == B.EMPTY:
            refs.append(None)
            continue
        kw = {}
        if u.get("dis_rir", -1) >= 0:
            kw = dict(distractor=sc["srcs"][u["dis_sound"]], distractor_rir=_wav(B.row_of(sc, u["dis_rir"]), sc["lens"][u["dis_rir"]]))
        refs.append(O.compute_audiogoal(sc["srcs"][u["sound"]], _wav(B.row_of(sc, g), sc["lens"][g]), B.SR,
                                        audio_index=u["t0"] // B.SR, **kw))
    sc["refs"] = refs
    return sc


def _run16(lib, sc, form, n_mels, **kw):
    kernel_form = {"rows": ROWS, "only": SPEC, "deq": SPEC, "half": HALF}[form]
    banks = {"rows": sc["rows"], "only": sc["f32"], "deq": sc["deq"], "half": sc["q"]}[form]
    return _launch(lib, K_CONV, kernel_form, sc["srcs"], sc["units"], banks, sc["s"] if form == "half" else None, B.FIRST, B.CAPS,
                   sc["lens"], B.SR, n_mels=n_mels, **kw)


@pytest.mark.parametrize("n_mels", [64, 40])
@pytest.mark.parametrize("form", ["rows", "only"])
def test_fp32_bucketed_loop_kernels_vs_oracle(lib, world, form, n_mels):
    mel, sg, wave = _run16(lib, world, form, n_mels)
    _check_oracle(f"16 kHz {form} {n_mels} bands", B.SR, world["refs"], mel, sg, wave, B.SR, n_mels)
    mel_alone, _, _ = _run16(lib, world, form, n_mels, want_sg=False, want_wave=False)
    assert mel_alone.tobytes() == mel.tobytes()                       # the other outputs change nothing about this one


def _model(sc, u):
    """float64 overlap-save of unit u from the halves and scales the bank holds"""
    out = np.zeros((2, B.SR))
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        b = B.bucket_of(g)
        spectra = R.bank_spectra(sc["q"][b][g - B.FIRST[b]], sc["s"][b][g - B.FIRST[b]], sc["perm"])
        nbh = max(1, P.ceil_div(int(sc["lens"][g]), P.KB))              # (the kernel skips the blocks behind the entry's length)
        out += R.model_audiogoal(sc["srcs"][snd], None, t0, B.SR, spectra=spectra[:, :nbh])
    return out


@pytest.mark.parametrize("n_mels", [64, 40])
def test_half_bucketed_mel_kernel(lib, world, n_mels):
    """k_conv_spec<.., MEL, HALF, HBK> against k_conv_spec<loop, MEL> over the same buckets fed float(q) * hscale"""
    h_mel, h_sg, h_w = _run16(lib, world, "half", n_mels)
    f_mel, f_sg, f_w = _run16(lib, world, "deq", n_mels)
    for k, u in enumerate(world["units"]):
        if world["refs"][k] is None:                                   # silent / empty: log(eps) exactly, zeros exactly
            assert np.allclose(h_mel[k], np.log(EPS), rtol=1e-6, atol=0) and h_mel[k].tobytes() == f_mel[k].tobytes(), k
            assert not h_sg[k].any() and not h_w[k].any(), k
            continue
        for name, h, f in (("waveform", h_w[k], f_w[k]), ("spectrogram", h_sg[k], f_sg[k])):
            peak = np.abs(f).max()
            err = np.abs(h.astype(np.float64) - f.astype(np.float64)).max() / peak
            print(f"[obs_logmel_buckets_host] half {n_mels} bands unit {k} {name}: |half - fp32(dequantised)| / peak = {err:.3e}")
            assert peak > 0 and err <= AB, (k, name, err)
        e_mel = np.abs(h_mel[k] - f_mel[k]).max() / np.abs(f_mel[k]).max()
        print(f"[obs_logmel_buckets_host] half {n_mels} bands unit {k} log-mel: {e_mel:.3e}")
        assert e_mel <= TOL, (k, e_mel)
    for k in (1, 3, 4, 6, 7, 8, 9):            # every bucket, both scaled entries, the 9000-tap entry, the two-bucket unit
        ref = _model(world, world["units"][k])
        err = O.relerr(h_w[k], ref)
        print(f"[obs_logmel_buckets_host] half {n_mels} bands unit {k}: waveform vs model fed the bank's halves = {err:.3e}")
        assert err <= TOL, (k, err)
        ref_mel = O.compute_logmel(ref.astype(np.float32), B.SR, n_mels=n_mels, eps=EPS)
        e_mel = np.abs(h_mel[k] - ref_mel).max() / np.abs(ref_mel).max()
        print(f"[obs_logmel_buckets_host] half {n_mels} bands unit {k}: log-mel vs model fed the bank's halves = {e_mel:.3e}")
        assert e_mel <= TOL, (k, e_mel)
    mel_alone, _, _ = _run16(lib, world, "half", n_mels, want_sg=False, want_wave=False)
    assert mel_alone.tobytes() == h_mel.tobytes()


# ---- 44.1 kHz: rows of three blocks on k_obs_rows<.., BUCKETS, MEL> and k_obs_blocks<.., MEL> ---------------------------------
SR44 = 44100
CAPS44 = [16000, 30000, 44100, 70000]
FIRST44 = [0, 2, 3, 5]
LENS44 = [16000, 9000, 30000, 44100, 0, 70000, 40000]
EMPTY44 = 4


@pytest.fixture(scope="module")
def world44(lib):
    rng = np.random.default_rng(29)
    srcs = [O.synth_sources(rng, SR44, k=1, seconds=s)[0] for s in (1, 3)]
    counts = [2, 1, 2, 2]
    rows = [np.zeros((n, 2, cap), np.float32) for n, cap in zip(counts, CAPS44)]
    dense = np.zeros((len(LENS44), 2, max(CAPS44)), np.float32)        # every entry in ONE allocation at the largest cap
    for g, n in enumerate(LENS44):
        if n == 0:
            continue
        b = max(k for k in range(4) if FIRST44[k] <= g)
        h = (O.synth_rir(rng, SR44, length=n, n=1) if g in (1, 6) else O.synth_rir_blocks(rng, SR44, n, n=1))[0]
        rows[b][g - FIRST44[b], :, :n] = h
        dense[g, :, :n] = h
    t0 = P.window_start_sim(3 * SR44, SR44, 2)
    units = [dict(sound=0, t0=0, rir=0),                                # bucket 0
             dict(sound=0, t0=0, rir=2),                                # bucket 1
             dict(rir=-1),                                              # silent
             dict(sound=1, t0=t0, rir=3),                               # bucket 2, steady branch of the 3-s clip
             dict(sound=0, t0=0, rir=5),                                # bucket 3, five blocks
             dict(sound=0, t0=0, rir=EMPTY44),                          # empty entry
             dict(sound=0, t0=0, rir=6, dis_sound=1, dis_rir=2),        # two terms, buckets 3 and 1
             dict(sound=0, t0=0, rir=1)]                                # bucket 0's last entry, 9000 taps

    def rir(g):
        return _wav(dense[g], LENS44[g])
    refs = [O.compute_audiogoal(srcs[0], rir(0), SR44), O.compute_audiogoal(srcs[0], rir(2), SR44), None,
            O.compute_audiogoal(srcs[1], rir(3), SR44, audio_index=2), O.compute_audiogoal(srcs[0], rir(5), SR44), None,
            O.compute_audiogoal(srcs[0], rir(6), SR44, distractor=srcs[1], distractor_rir=rir(2)),
            O.compute_audiogoal(srcs[0], rir(1), SR44)]
    return dict(srcs=srcs, rows=rows, dense=dense, units=units, refs=refs, lens=np.asarray(LENS44, np.int32),
                f32=[_fp32_spectra(lib, r) for r in rows], dense_f32=_fp32_spectra(lib, dense))


def _run44(lib, w, kernel, spectral, dense, **kw):
    if dense:
        banks, firsts, caps = [w["dense_f32"] if spectral else w["dense"]], [0], [max(CAPS44)]
    else:
        banks, firsts, caps = (w["f32"] if spectral else w["rows"]), FIRST44, CAPS44
    return _launch(lib, kernel, SPEC if spectral else ROWS, w["srcs"], w["units"], banks, None, firsts, caps, w["lens"], SR44, **kw)


def _same(tag, got, want):
    for name, g, d in zip(("log-mel", "spectrogram", "waveform"), got, want):
        assert (g is None) == (d is None)
        if g is not None:
            assert np.array_equal(g, d), (tag, name, float(np.abs(g - d).max()))


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_rows_kernel_over_buckets(lib, world44, spectral):
    """k_obs_rows<.., BUCKETS, MEL>, 3 persistent workgroups over 16 rows: the oracle, and the single-allocation instantiation"""
    n_mels = 40 if spectral else 64
    got = _run44(lib, world44, K_ROWS, spectral, False, n_mels=n_mels, wgs=3)
    _check_oracle(f"44.1 kHz rows spectral={spectral}", SR44, world44["refs"], *got, SR44, n_mels)
    _same("rows", got, _run44(lib, world44, K_ROWS, spectral, True, n_mels=n_mels, wgs=3))


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_rows_kernel_over_buckets_split_rows(lib, world44, spectral):
    """parts_log2 = 1: every row on two workgroups"""
    got = _run44(lib, world44, K_ROWS, spectral, False, parts_log2=1, want_wave=not spectral)
    _check_oracle(f"44.1 kHz rows parts 1 spectral={spectral}", SR44, world44["refs"], *got, SR44, 64)
    _same("rows parts", got, _run44(lib, world44, K_ROWS, spectral, True, parts_log2=1, want_wave=not spectral))


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_rows_kernel_over_buckets_short_step_without_waveform(lib, world44, spectral):
    """n_valid = 20 000 (two rendered blocks), no waveform buffer: the frames behind the live pooled blocks are log(eps)"""
    n_valid = 20000
    got = _run44(lib, world44, K_ROWS, spectral, False, n_valid=n_valid, want_wave=False, want_sg=spectral)
    _check_oracle(f"44.1 kHz rows n_valid {n_valid} spectral={spectral}", SR44, world44["refs"], *got, n_valid, 64)
    _same("rows short", got, _run44(lib, world44, K_ROWS, spectral, True, n_valid=n_valid, want_wave=False, want_sg=spectral))
    first_quiet = 4 * P.live_pooled_blocks(n_valid, SR44)
    assert first_quiet < got[0].shape[2] and np.allclose(got[0][0][:, first_quiet:], np.log(EPS), rtol=1e-6, atol=0)


@pytest.mark.parametrize("spectral", [False, True], ids=["time", "spectral"])
def test_blocks_kernel_over_buckets(lib, world44, spectral):
    """k_obs_blocks<SPECTRAL, MEL> resolves the buckets itself: same bank, one workgroup per output block"""
    n_mels = 64 if spectral else 40
    got = _run44(lib, world44, K_BLOCKS, spectral, False, n_mels=n_mels)
    _check_oracle(f"44.1 kHz blocks spectral={spectral}", SR44, world44["refs"], *got, SR44, n_mels)
    _same("blocks", got, _run44(lib, world44, K_BLOCKS, spectral, True, n_mels=n_mels))
