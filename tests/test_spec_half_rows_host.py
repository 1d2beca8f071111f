"""The half-precision spectral RIR bank under the fused row kernels of 2 or 3 partition blocks, on the host-compiled kernels
(tests/spec_half_rows_host.cpp on the host-sim fibers).

A/B: k_obs_blocks<true, MEL, HALF> and k_obs_rows<true, false, false, MEL, HALF> against the fp32 instantiations of the same
templates fed float(q) * hscale, on identical parameters.  Bound 2e-6 of the reference's peak (the project's A/B bound: each fp32
path is held to <= 1e-6 of peak against float64 and the inputs are identical); the log-mel output under the project's 1e-4 rule.
Measured: 0.0 on every form and output (the dequantised value is exact in fp32, the arithmetic behind it is the same
instructions) - profiles/r7/NOTES.md.

Model: the half kernels against the float64 multi-block overlap-save model of tests/spec_half_rows_ref.py with the same
quantiser, <= 1e-4 of peak (the project's parity budget); and the format's loss at 44.1 kHz - the quantised model against
oracle.compute_audiogoal - measured and printed (INTEGRATION.md "Half-precision spectral banks").

Bank: 6 entries at capacity 49 152 with RIR lengths 0 / 9 000 / 16 384 / 16 385 / 40 000 / 49 152, every partition block audible,
entry 2 scaled by 32 768 and entry 3 by 1e-6 (scales that differ per block and per entry).  Every output is pre-filled with NaN."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_half_rows_ref as R
hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 49152
LENGTHS = [0, 9000, 16384, 16385, 40000, 49152]
BOUND = 2e-6
MEL_TOL = 1e-4
EPS = 1e-6


@pytest.fixture(scope="module")
def rows_lib(tmp_path_factory):
    so = hs.build_driver("spec_half_rows", tmp_path_factory.mktemp("spec_half_rows"))
    lib = ctypes.CDLL(so)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.hs_obs_rows_spec_ab.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, ci, ci, ci, ci, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    lib.hs_rir_spectra.argtypes = [vp, vp, ci, ctypes.c_longlong, ci, ci]
    return lib


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
def bank(rows_lib):
    """the six-entry bank: time-domain rows, fp32 block spectra (hs_rir_spectra), their half form and its dequantisation.
    Computed once, shared by every test, never written to."""
    rng = np.random.default_rng(31)
    rows = np.zeros((len(LENGTHS), 2, CAP), np.float32)
    for i, n in enumerate(LENGTHS):
        if n:
            rows[i, :, :n] = O.synth_rir_blocks(rng, 44100, n, n=1)[0]
    rows[2] *= np.float32(32768.0)
    rows[3] *= np.float32(1e-6)
    hb = P.ceil_div(CAP, P.KB)
    f32 = np.zeros((len(LENGTHS), 2, hb, P.SPEC_FLOATS), np.float32)
    assert rows_lib.hs_rir_spectra(rows.ctypes.data, f32.ctypes.data, len(LENGTHS), 2 * CAP, CAP, CAP) == 0
    q, s = R.quantise(f32)
    assert len(np.unique(s[1:])) >= 3                    # the scales differ from block to block (2^15 and 1e-6 apart at least)
    out = dict(rows=rows, lens=np.asarray(LENGTHS, np.int32), hb=hb, q=np.ascontiguousarray(q), s=np.ascontiguousarray(s),
               deq=np.ascontiguousarray(R.dequantise(q, s)))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


_SOURCES = {}


def _sources(sr):
    if sr not in _SOURCES:
        rng = np.random.default_rng(sr)
        _SOURCES[sr] = [O.synth_sources(rng, sr, k=1, seconds=1)[0], O.synth_sources(rng, sr, k=1, seconds=3)[0]]
    return _SOURCES[sr]


def _units(sr, variant=0):
    """plain | one with a distractor term | silent | one on the empty RIR.  Between the two variants every bank entry is read."""
    t0 = P.window_start_sim(3 * sr, sr, 2)               # steady branch of the 3-s clip: every RIR block has a window
    if variant == 0:
        return [dict(sound=1, t0=t0, rir=5), dict(sound=0, t0=0, rir=2, dis_sound=1, dis_rir=4), dict(rir=-1), dict(sound=0, t0=0, rir=0)]
    return [dict(sound=1, t0=t0, rir=3), dict(sound=0, t0=0, rir=4, dis_sound=1, dis_rir=1), dict(rir=-1), dict(sound=0, t0=0, rir=0)]


def _ab(lib, bank, sr, units, *, blocks, mel=False, n_valid=None, parts_log2=0, wgs=8, no_distractor=False, want_wave=True,
        want_sg=True, n_mels=64, pad_mode=0, only_half=False):
    """run the HALF instantiation and the fp32 one over the dequantised spectra -> {name: [half, fp32]} of every output"""
    n_valid = sr if n_valid is None else n_valid
    srcs = _sources(sr)
    wd, desc = _plan(srcs, units, CAP, n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    start, w, max_len = P.mel_filterbank_sparse(sr, n_mels)
    start, w = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(w, np.float32)
    n = len(units)
    t_frames, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    res = {}
    for half in ((1,) if only_half else (1, 0)):
        wave = np.full((n, 2, sr), np.nan, np.float32) if want_wave else None
        sg = np.full((n, 65, t4, 2), np.nan, np.float32) if want_sg else None
        lm = np.full((n, n_mels, t_frames, 2), np.nan, np.float32) if mel else None
        bankp = bank["q"].ctypes.data if half else bank["deq"].ctypes.data
        rc = lib.hs_obs_rows_spec_ab(half, int(blocks), int(mel), spec.ctypes.data, bankp, bank["s"].ctypes.data if half else None,
                                     bank["lens"].ctypes.data, desc.ctypes.data, wave.ctypes.data if want_wave else None,
                                     sg.ctypes.data if want_sg else None, lm.ctypes.data if mel else None, start.ctypes.data,
                                     w.ctypes.data, n_mels, max_len, EPS, n, bank["hb"], n_valid, sr, pad_mode, wgs, parts_log2,
                                     int(no_distractor))
        assert rc == 0, rc
        for name, a in (("wave", wave), ("sgram", sg), ("logmel", lm)):
            if a is not None:
                if name == "wave":
                    assert not np.isnan(a[:, :, :n_valid]).any(), (name, half)
                else:
                    assert not np.isnan(a).any(), (name, half)
                res.setdefault(name, []).append(a)
    return res


def _check(res, label, live, n_valid=None):
    for name, (h, f) in res.items():
        if name == "wave" and n_valid is not None:
            h, f = h[:, :, :n_valid], f[:, :, :n_valid]
        peak = np.abs(f).max()
        err = np.abs(h.astype(np.float64) - f.astype(np.float64)).max() / peak
        print(f"[spec_half_rows_host] {label} {name}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        if name == "logmel":
            for k in range(len(f)):                       # the project's log-mel rule: 1e-4 of the largest value per unit
                assert np.abs(h[k] - f[k]).max() <= MEL_TOL * np.abs(f[k]).max(), (label, name, k)
        else:
            assert err <= BOUND, (label, name, err)
            assert peak > 0 and all(np.abs(f[k]).max() > 0 for k in live), (label, name)
            assert not h[2].any() and not h[3].any(), (label, name)       # silent / empty RIR: exact zeros


# ---- A/B ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts_log2", [0, 1])
@pytest.mark.parametrize("sr", [44100, 48000, 20000])
def test_obs_blocks_half_ab(rows_lib, bank, sr, parts_log2):
    """k_obs_blocks<true, false, HALF>: one workgroup per output block (and part), in ascending block order"""
    variant = parts_log2 if sr != 48000 else 1 - parts_log2
    res = _ab(rows_lib, bank, sr, _units(sr, variant), blocks=True, parts_log2=parts_log2, want_wave=parts_log2 == 0)
    _check(res, f"blocks {sr} parts {parts_log2}", live=[0, 1])


@pytest.mark.parametrize("case", ["44100", "48000", "20000", "44100-parts1", "44100-3wgs", "44100-short"])
def test_obs_rows_half_ab(rows_lib, bank, case):
    """k_obs_rows<true, false, false, false, HALF>: a workgroup per row; split rows; 3 workgroups over 8 rows (state carried
    from row to row); n_valid = 20 000 of 44 100 (nb_y < nb_rows) without a waveform buffer"""
    sr = int(case.split("-")[0])
    kw = dict(blocks=False)
    n_valid = None
    if case.endswith("parts1"):
        kw.update(parts_log2=1, want_wave=False)
    elif case.endswith("3wgs"):
        kw.update(wgs=3)
    elif case.endswith("short"):
        n_valid = 20000
        kw.update(n_valid=n_valid, want_wave=False, wgs=3)
    variant = 1 if case in ("48000", "44100-parts1") else 0
    res = _ab(rows_lib, bank, sr, _units(sr, variant), **kw)
    _check(res, f"rows {case}", live=[0, 1], n_valid=n_valid)


@pytest.mark.parametrize("blocks", [False, True], ids=["rows", "blocks"])
def test_no_distractor_flag_half_ab(rows_lib, bank, blocks):
    """the same units under SS_FLAG_NO_DISTRACTOR (n_terms = 1): term 1 of the distractor unit is ignored by both forms"""
    sr = 44100
    res = _ab(rows_lib, bank, sr, _units(sr, 0), blocks=blocks, no_distractor=True, wgs=3)
    _check(res, f"no-distractor blocks={blocks}", live=[0, 1])
    both = _ab(rows_lib, bank, sr, _units(sr, 0)[1:2], blocks=blocks, only_half=True, want_sg=True)
    assert np.abs(both["wave"][0][0] - res["wave"][0][1]).max() > 0      # (the flag did change the unit's waveform)


@pytest.mark.parametrize("want_sg", [True, False], ids=["sgram", "no-sgram"])
@pytest.mark.parametrize("n_mels", [64, 40])
@pytest.mark.parametrize("blocks", [False, True], ids=["rows", "blocks"])
def test_logmel_half_ab(rows_lib, bank, blocks, n_mels, want_sg):
    """the MEL forms at 64 and 40 bands, each with and without the pooled spectrogram (and, the other way round, the waveform)"""
    sr = 44100 if (n_mels == 64) == want_sg else 48000
    res = _ab(rows_lib, bank, sr, _units(sr, int(want_sg)), blocks=blocks, mel=True, n_mels=n_mels, want_sg=want_sg,
              want_wave=not want_sg, wgs=3, parts_log2=int(blocks and want_sg))
    assert set(res) == {"logmel"} | ({"sgram"} if want_sg else {"wave"})
    _check(res, f"MEL {n_mels} blocks={blocks}", live=[0, 1])
    lm = res["logmel"][0]
    assert np.allclose(lm[2], np.log(EPS), rtol=1e-6) and np.allclose(lm[3], np.log(EPS), rtol=1e-6)


# ---- model --------------------------------------------------------------------------------------------------------------------
def test_half_rows_against_the_quantised_model(rows_lib, bank):
    """both kernels at 44.1 kHz against the float64 overlap-save model with the same quantiser: <= 1e-4 of peak (the model
    rounds its fp64 spectra, the kernel its fp32 ones); a dropped or mis-scaled block would be ~1e-1"""
    sr = 44100
    units = _units(sr, 0)
    srcs = _sources(sr)
    rows, lens = bank["rows"], bank["lens"]
    ref0 = R.model_audiogoal(srcs[1], rows[5][:, :lens[5]], units[0]["t0"], sr)
    ref1 = (R.model_audiogoal(srcs[0], rows[2][:, :lens[2]], 0, sr) + R.model_audiogoal(srcs[1], rows[4][:, :lens[4]], 0, sr))

    def spectra_of(probe):                               # the host build of ss_rir_spectra_f32 on one-block rows
        out = np.zeros((probe.shape[0], 2, 1, P.SPEC_FLOATS), np.float32)
        probe = np.ascontiguousarray(probe, np.float32)
        assert rows_lib.hs_rir_spectra(probe.ctypes.data, out.ctypes.data, probe.shape[0], 2 * P.KB, P.KB, P.KB) == 0
        return out
    # ... and the same model fed the halves and scales the BANK holds (the quantiser's decisions on the kernel's own fp32 spectra)
    nat = R.bank_spectra(bank["q"], bank["s"], R.kernel_order(spectra_of))
    own0 = R.model_audiogoal(srcs[1], None, units[0]["t0"], sr, spectra=nat[5])
    own1 = R.model_audiogoal(srcs[0], None, 0, sr, spectra=nat[2]) + R.model_audiogoal(srcs[1], None, 0, sr, spectra=nat[4])
    for blocks in (False, True):
        res = _ab(rows_lib, bank, sr, units, blocks=blocks, only_half=True)
        wave = res["wave"][0]
        for name, refs in (("the model's own quantisation", (ref0, ref1)), ("the bank's halves", (own0, own1))):
            for k, ref in enumerate(refs):
                err = O.relerr(wave[k], ref)
                e = O.relerr(res["sgram"][0][k], O.compute_spectrogram(ref.astype(np.float32)))
                print(f"[spec_half_rows_host] blocks={blocks} unit {k}, model with {name}: waveform {err:.3e}, pooled spectrogram {e:.3e}")
                assert err <= 1e-4 and e <= 1e-4, (blocks, k, name, err, e)


def test_model_matches_the_oracle_unquantised_at_44k():
    """the multi-block model without its quantiser is the oracle's convolution; with it, the waveform moves by the format's loss
    at 44.1 kHz (RIRs of 9 000 / 40 000 / 49 152 samples under a 3-s clip) - measured here, written down in INTEGRATION.md"""
    sr = 44100
    rng = np.random.default_rng(3)
    src = O.synth_sources(rng, sr, k=1, seconds=3)[0]
    worst, moved, moved_sg = 0.0, [], []
    for n in (9000, 40000, 49152):
        rir = O.synth_rir(rng, sr, length=n, n=1)[0]
        ref = O.compute_audiogoal(src, np.ascontiguousarray(rir.T), sr, audio_index=2)
        worst = max(worst, O.relerr(R.model_audiogoal(src, rir, 2 * sr, sr, quant=False), ref))
        got = R.model_audiogoal(src, rir, 2 * sr, sr, quant=True)
        moved.append(O.relerr(got, ref))
        moved_sg.append(O.relerr(O.compute_spectrogram(got.astype(np.float32)), O.compute_spectrogram(np.asarray(ref, np.float32))))
        print(f"[spec_half_rows_host] 44.1 kHz, RIR {n}: quantised model vs oracle: waveform {moved[-1]:.2e}, "
              f"pooled spectrogram {moved_sg[-1]:.2e}")
    print(f"[spec_half_rows_host] model vs oracle {worst:.2e}; quantised model vs oracle {min(moved):.2e} .. {max(moved):.2e}")
    assert worst <= 1e-6
    assert 1e-5 < min(moved) and max(moved) < 1e-3
