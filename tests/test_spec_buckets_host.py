"""Spectral length buckets on the host-compiled loop kernel (tests/spec_buckets_host.cpp on the host-sim fibers).

Four buckets of 1 / 2 / 3 / 5 partition blocks (tests/spec_buckets_ref.py), one launch of 12 units over the first and last entry
of each, a two-bucket distractor unit, an empty entry, a silent unit and entries scaled by 32768 and 1e-6.

Half form: k_conv_spec<.., HALF, HBK> against the fp32 bucketed instantiation of the same template fed float(q) * hscale - the
unfused form at out_len 16000 and at 44100 (three output blocks), the fused form at 16000.  Bound 2e-6 of the reference's peak,
the project's A/B bound (tests/test_spec_half_host.py): each fp32 path is held to <= 1e-6 of peak against float64 and the inputs
are identical.  Measured 0.0 on all three (profiles/r7/NOTES.md): the two instantiations resolve the bucket independently
(bank_spec16 / bank_spec) and run the same arithmetic on the same values.  One unit per bucket is also held to the float64
overlap-save model fed the bank's own halves and scales (1e-4, the parity budget): a block read from the wrong bucket is ~1e-1.

fp32 form: the launch without time-domain rows anywhere in its arguments is bit-identical to the both-forms bucketed launch on
the same spectra."""
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
SR = B.SR
BOUND = 2e-6
BUDGET = 1e-4


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("spec_buckets", tmp_path_factory.mktemp("spec_buckets"))
    L = ctypes.CDLL(so)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.hs_conv_spec_buckets.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci]
    L.hs_source_windows.argtypes = [vp, vp, vp, ci]
    L.hs_rir_spectra.argtypes = [vp, vp, ci, ll, ci, ci]
    return L


@pytest.fixture(scope="module")
def world(lib):
    """the scene, per bucket its fp32 spectra, their half form and the dequantised halves, and the kernel's component order"""
    sc = B.scene()
    f32 = [_fp32_spectra(lib, rows) for rows in sc["rows"]]
    qs = [R.quantise(f) for f in f32]
    sc["f32"] = f32
    sc["q"] = [np.ascontiguousarray(q) for q, _ in qs]
    sc["s"] = [np.ascontiguousarray(s) for _, s in qs]
    sc["deq"] = [np.ascontiguousarray(R.dequantise(q, s)) for q, s in qs]
    sc["perm"] = R.kernel_order(lambda rows: _fp32_spectra(lib, rows))
    # the scale of a wrong bucket or block cannot hide inside a tolerance: the scaled entries' scales are far from every other
    big, small, plain = sc["s"][0][B.BIG - B.FIRST[0]], sc["s"][2][B.SMALL - B.FIRST[2]][:, :2], sc["s"][3][0]
    assert big.min() >= 2.0 ** 10 * plain.max() and small.max() <= 2.0 ** -10 * plain.min()
    return sc


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _run(lib, sc, form, fuse, out_len, n_valid):
    """form: 'half' | 'deq' (fp32 kernel, dequantised halves, no rows) | 'only' (fp32 spectra, no rows) | 'both' (fp32 spectra
    and the time-domain rows in the arguments) -> (waveform, pooled spectrogram or None)"""
    srcs, units = sc["srcs"], sc["units"]
    wd, desc = _plan(srcs, units, max(B.CAPS), n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    n = len(units)
    wave = np.full((n, 2, out_len), np.nan, np.float32)
    sg = np.full((n,) + P.spectrogram_shape(out_len), np.nan, np.float32) if fuse else None
    bank = {"half": sc["q"], "deq": sc["deq"], "only": sc["f32"], "both": sc["f32"]}[form]
    hspec = _ptrs(bank)
    hscale = _ptrs(sc["s"]) if form == "half" else None
    rows = _ptrs(sc["rows"]) if form == "both" else None
    first, caps = np.asarray(B.FIRST, np.int32), np.asarray(B.CAPS, np.int32)
    rc = lib.hs_conv_spec_buckets(int(form == "half"), int(fuse), spec.ctypes.data, hspec, hscale, rows, first.ctypes.data,
                                  caps.ctypes.data, 4, sc["lens"].ctypes.data, desc.ctypes.data, wave.ctypes.data,
                                  sg.ctypes.data if fuse else None, n, n_valid, out_len, 0)
    assert rc == 0, rc
    assert not np.isnan(wave).any() and (sg is None or not np.isnan(sg).any()), form
    return wave, sg


def _ab(got, ref, label):
    peak = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / peak
    print(f"[spec_buckets_host] {label}: max |half - fp32(dequantised)| / peak = {err:.3e}")
    assert peak > 0 and err <= BOUND, (label, err)


def _zeros_and_live(wave, sg, units):
    for n, u in enumerate(units):
        dead = u.get("rir", -1) < 0 or u["rir"] == B.EMPTY
        assert bool(wave[n].any()) != dead, n                          # the empty entry and the silent unit: exact zeros
        if sg is not None:
            assert bool(sg[n].any()) != dead, n


def _model(sc, u, out_len):
    """float64 overlap-save of unit u from the halves and scales the bank holds"""
    out = np.zeros((2, out_len))
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        b = B.bucket_of(g)
        spectra = R.bank_spectra(sc["q"][b][g - B.FIRST[b]], sc["s"][b][g - B.FIRST[b]], sc["perm"])
        nbh = max(1, P.ceil_div(int(sc["lens"][g]), P.KB))              # (the kernel skips the blocks behind the entry's length)
        out += R.model_audiogoal(sc["srcs"][snd], None, t0, out_len, spectra=spectra[:, :nbh])
    return out


@pytest.mark.parametrize("out_len,fuse", [(16000, False), (44100, False), (16000, True)],
                         ids=["unfused-16000", "unfused-44100-three-output-blocks", "fused-16000"])
def test_half_buckets_equal_fp32_buckets_fed_dequantised_spectra(lib, world, out_len, fuse):
    half_w, half_s = _run(lib, world, "half", fuse, out_len, out_len)
    ref_w, ref_s = _run(lib, world, "deq", fuse, out_len, out_len)
    label = f"{'fused' if fuse else 'unfused'} out_len {out_len}"
    _ab(half_w, ref_w, label + " waveform")
    if fuse:
        _ab(half_s, ref_s, label + " spectrogram")
    _zeros_and_live(half_w, half_s, world["units"])
    for n in (1, 3, 4, 6, 7, 8, 9):            # every bucket, both scaled entries, the 9000-tap entry, the two-bucket unit
        ref = _model(world, world["units"][n], out_len)
        err = O.relerr(half_w[n], ref)
        print(f"[spec_buckets_host] {label} unit {n}: half kernel vs model fed the bank's halves = {err:.3e}")
        assert err <= BUDGET, (n, err)


@pytest.mark.parametrize("out_len,fuse", [(16000, False), (44100, False), (16000, True)],
                         ids=["unfused-16000", "unfused-44100", "fused-16000"])
def test_fp32_spectral_only_launch_is_the_both_forms_launch_bit_for_bit(lib, world, out_len, fuse):
    only_w, only_s = _run(lib, world, "only", fuse, out_len, out_len)
    both_w, both_s = _run(lib, world, "both", fuse, out_len, out_len)
    assert only_w.tobytes() == both_w.tobytes()
    if fuse:
        assert only_s.tobytes() == both_s.tobytes()
    _zeros_and_live(only_w, only_s, world["units"])
    ref = O.compute_audiogoal(world["srcs"][2], np.ascontiguousarray(B.row_of(world, 8).T), SR, audio_index=1)
    if out_len == SR:                                                  # (the oracle's rows are one second long)
        assert O.relerr(only_w[6], ref) <= 1e-5
