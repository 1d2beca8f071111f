"""A half-precision RIR bank in LENGTH BUCKETS under the fused row kernels of 2 or 3 partition blocks, on the host-compiled kernels
(tests/spec_half_bucket_rows_host.cpp on the host-sim fibers): k_obs_rows<true, false, BUCKETS, MEL, HALF> and
k_obs_blocks<true, MEL, HALF, HBK>.  The scene is tests/spec_half_bucket_rows_world.py: three buckets of 1 / 3 / 5 blocks, RIR
lengths below, at and clamped by their bucket's depth, entries scaled by 32 768 and 1e-6 in different buckets, units whose two
terms sit in buckets of different depth, a silent unit, the empty RIR, the 3-s clip at t0 = 1 s.  Every output is pre-filled with NaN.

A/B: against the fp32 BUCKETS instantiations of the same templates fed float(q) * hscale on identical parameters: <= 2e-6 of the
reference's peak (the project's A/B bound: each fp32 path is held to <= 1e-6 of peak against float64 and the inputs are identical);
log-mel under the project's 1e-4 rule.  The measured value is printed.
Model: against the float64 overlap-save model of tests/spec_half_rows_ref.py fed the halves and scales the bank holds, cut at
nbh = min(ceil(rir_len / kB), the bucket's blocks): <= 1e-4 of peak.
One bucket: the bucketed instantiation over a single bucket equals the single-allocation HALF instantiation bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import spec_half_bucket_rows_world as W
import spec_half_rows_ref as R
hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 2e-6
BUDGET = 1e-4
MEL_TOL = 1e-4
EPS = 1e-6


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("spec_half_bucket_rows", tmp_path_factory.mktemp("spec_half_bucket_rows"))
    lib = ctypes.CDLL(so)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.hs_obs_rows_half_buckets.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, ci, ci, ci, ci,
                                             ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    lib.hs_rir_spectra.argtypes = [vp, vp, ci, ctypes.c_longlong, ci, ci]
    return lib


@pytest.fixture(scope="module")
def bank(lib):
    """per bucket: fp32 block spectra (hs_rir_spectra), their half form and its dequantisation; the kernel's component order.
    Computed once, shared by every test, never written to."""
    sc = W.scene()
    f32, q, s, deq = [], [], [], []
    for rows, cap in zip(sc["rows"], W.CAPS):
        a = np.zeros((rows.shape[0], 2, P.ceil_div(cap, P.KB), P.SPEC_FLOATS), np.float32)
        assert lib.hs_rir_spectra(rows.ctypes.data, a.ctypes.data, rows.shape[0], 2 * cap, cap, cap) == 0
        qq, ss = R.quantise(a)
        f32.append(a); q.append(np.ascontiguousarray(qq)); s.append(np.ascontiguousarray(ss))
        deq.append(np.ascontiguousarray(R.dequantise(qq, ss)))
    assert len(np.unique(np.concatenate([x.ravel() for x in s]))) >= 4         # scales differ per block, entry and bucket

    def spectra_of(probe):                               # the host build of ss_rir_spectra_f32 on one-block rows
        out = np.zeros((probe.shape[0], 2, 1, P.SPEC_FLOATS), np.float32)
        probe = np.ascontiguousarray(probe, np.float32)
        assert lib.hs_rir_spectra(probe.ctypes.data, out.ctypes.data, probe.shape[0], 2 * P.KB, P.KB, P.KB) == 0
        return out
    out = dict(q=q, s=s, deq=deq, perm=R.kernel_order(spectra_of), lens=sc["lens"])
    for group in (q, s, deq):
        for a in group:
            a.setflags(write=False)
    return out


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data if a is not None else None for a in arrays])


def _run(lib, bank, form, sr, units, *, blocks, mel=False, n_valid=None, parts_log2=0, wgs=8, want_wave=True, want_sg=True,
         n_mels=64, buckets=(0, 1, 2), lens=None):
    """one launch of instantiation `form` (0 fp32 buckets | 1 half buckets | 2 half, one allocation) -> {name: array}"""
    n_valid = sr if n_valid is None else n_valid
    srcs = W.sources(sr)
    wd, desc = W.plan(srcs, units, n_valid)
    flat = np.concatenate([np.asarray(x, np.float32) for x in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    start, w, max_len = P.mel_filterbank_sparse(sr, n_mels)
    start, w = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(w, np.float32)
    n = len(units)
    t_frames, t4 = 1 + sr // 160, P.spectrogram_shape(sr)[1]
    wave = np.full((n, 2, sr), np.nan, np.float32) if want_wave else None
    sg = np.full((n, 65, t4, 2), np.nan, np.float32) if want_sg else None
    lm = np.full((n, n_mels, t_frames, 2), np.nan, np.float32) if mel else None
    data = [(bank["q"] if form else bank["deq"])[b] for b in buckets]
    scales = [bank["s"][b] if form else None for b in buckets]
    first = np.asarray([W.FIRST[b] - W.FIRST[buckets[0]] for b in buckets], np.int32)
    cap = np.asarray([W.CAPS[b] for b in buckets], np.int32)
    lens = bank["lens"] if lens is None else lens
    rc = lib.hs_obs_rows_half_buckets(form, int(blocks), int(mel), spec.ctypes.data, _ptrs(data), _ptrs(scales), first.ctypes.data,
                                      cap.ctypes.data, len(buckets), lens.ctypes.data, desc.ctypes.data,
                                      wave.ctypes.data if want_wave else None, sg.ctypes.data if want_sg else None,
                                      lm.ctypes.data if mel else None, start.ctypes.data, w.ctypes.data, n_mels, max_len, EPS, n, n_valid,
                                      sr, 0, wgs, parts_log2, 0)
    assert rc == 0, rc
    res = {}
    for name, a in (("wave", wave), ("sgram", sg), ("logmel", lm)):
        if a is not None:
            assert not np.isnan(a[:, :, :n_valid] if name == "wave" else a).any(), (name, form)
            res[name] = a
    return res


def _check_ab(got, ref, label, n_valid=None):
    """half buckets against the fp32 buckets fed the dequantised spectra; silent unit and empty RIR: exact zeros / log(eps)"""
    for name in ref:
        h, f = got[name], ref[name]
        if name == "wave" and n_valid is not None:
            h, f = h[:, :, :n_valid], f[:, :, :n_valid]
        peak = np.abs(f).max()
        err = np.abs(h.astype(np.float64) - f.astype(np.float64)).max() / peak
        print(f"[spec_half_bucket_rows_host] {label} {name}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        if name == "logmel":
            for k in range(len(f)):                       # the project's log-mel rule: 1e-4 of the largest value per unit
                assert np.abs(h[k] - f[k]).max() <= MEL_TOL * np.abs(f[k]).max(), (label, name, k)
            for k in W.DEAD:
                assert np.allclose(h[k], np.log(EPS), rtol=1e-6), (label, k)
        else:
            assert err <= BOUND, (label, name, err)
            assert all(np.abs(f[k]).max() > 0 for k in W.LIVE), (label, name)
            for k in W.DEAD:
                assert not h[k].any(), (label, name, k)


def _model(bank, sr, u):
    """float64 overlap-save of unit u from the halves and scales the bank holds, cut where the kernel stops reading"""
    srcs = W.sources(sr)
    out = np.zeros((2, sr))
    for snd, t0, g in W.terms(u):
        b = W.bucket_of(g)
        nbh = min(P.ceil_div(W.LENS[g], P.KB), P.ceil_div(W.CAPS[b], P.KB))
        if nbh == 0:
            continue
        spectra = R.bank_spectra(bank["q"][b][g - W.FIRST[b]], bank["s"][b][g - W.FIRST[b]], bank["perm"])[:, :nbh]
        out += R.model_audiogoal(srcs[snd], None, t0, sr, spectra=spectra)
    return out


_REFS = {}


def _check_model(bank, sr, units, got, label, n_valid=None):
    for k in W.LIVE:
        if (sr, k) not in _REFS:
            _REFS[(sr, k)] = _model(bank, sr, units[k])
        ref = _REFS[(sr, k)]
        if n_valid is None:
            es = O.relerr(got["sgram"][k], O.compute_spectrogram(ref.astype(np.float32))) if "sgram" in got else 0.0
            ea = O.relerr(got["wave"][k], ref) if "wave" in got else 0.0
        else:
            ea, es = O.relerr(got["wave"][k][:, :n_valid], ref[:, :n_valid]), 0.0
        print(f"[spec_half_bucket_rows_host] {label} unit {k}: vs model fed the bank's halves waveform {ea:.3e} spectrogram {es:.3e}")
        assert ea <= BUDGET and es <= BUDGET, (label, k, ea, es)


@pytest.mark.parametrize("mel", [False, True], ids=["sgram", "mel"])
@pytest.mark.parametrize("kernel", ["rows", "blocks"])
def test_half_buckets_ab_and_model_at_44100(lib, bank, kernel, mel):
    """three-block rows (the last one partial).  rows: 3 persistent workgroups over 14 rows - the row loop runs up to five times
    per workgroup, state carried from row to row; blocks: one workgroup per output block"""
    sr, units = 44100, W.units(44100)
    kw = dict(blocks=kernel == "blocks", mel=mel, wgs=3)
    got, ref = _run(lib, bank, 1, sr, units, **kw), _run(lib, bank, 0, sr, units, **kw)
    _check_ab(got, ref, f"{kernel} mel={mel} 44100")
    _check_model(bank, sr, units, got, f"{kernel} mel={mel} 44100")


@pytest.mark.parametrize("kernel", ["rows", "blocks"])
def test_half_buckets_split_rows_at_22050(lib, bank, kernel):
    """two-block rows with parts_log2 = 1 (a row, or an output block, on two workgroups), the log-mel form without a waveform"""
    sr, units = 22050, W.units(22050)
    kw = dict(blocks=kernel == "blocks", mel=True, parts_log2=1, want_wave=False)
    got, ref = _run(lib, bank, 1, sr, units, **kw), _run(lib, bank, 0, sr, units, **kw)
    assert set(got) == {"sgram", "logmel"}
    _check_ab(got, ref, f"{kernel} parts 22050")
    _check_model(bank, sr, units, got, f"{kernel} parts 22050")


def test_half_buckets_rows_short_step(lib, bank):
    """n_valid = 40 000 of 44 100 on k_obs_rows: the pooled blocks behind it are written, not computed"""
    sr, units, n_valid = 44100, W.units(44100), 40000
    kw = dict(blocks=False, n_valid=n_valid, wgs=8)
    got, ref = _run(lib, bank, 1, sr, units, **kw), _run(lib, bank, 0, sr, units, **kw)
    _check_ab(got, ref, "rows n_valid 40000", n_valid=n_valid)
    _check_model(bank, sr, units, got, "rows n_valid 40000", n_valid=n_valid)


@pytest.mark.parametrize("mel", [False, True], ids=["sgram", "mel"])
@pytest.mark.parametrize("kernel", ["rows", "blocks"])
def test_one_bucket_equals_the_single_allocation_half_instantiation(lib, bank, kernel, mel):
    """the bucketed half instantiation over bucket 1 alone against k_obs_rows / k_obs_blocks <.., HALF> on the same arrays"""
    sr = 44100
    units = [dict(sound=1, t0=sr, rir=1), dict(sound=0, t0=0, rir=0, dis_sound=1, dis_rir=2), dict(rir=-1)]
    lens = np.ascontiguousarray(bank["lens"][W.FIRST[1]:W.FIRST[1] + W.COUNTS[1]])
    kw = dict(blocks=kernel == "blocks", mel=mel, buckets=(1,), lens=lens, wgs=2)
    a, b = _run(lib, bank, 1, sr, units, **kw), _run(lib, bank, 2, sr, units, **kw)
    assert set(a) == set(b) and len(a) == 2 + int(mel)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), (kernel, name)
        assert a[name][0].any() and a[name][1].any()
