"""k_stage_spectra (staged RIR rows -> block spectra of a spectral-only bank), compiled for the host on the host-sim fibers,
against the host-sim spectral-bank entry (k_source_windows with scale 1, hostsim.hs_rir_spectra) over the same rows
scattered planar: the spectra must be BIT-identical, in wav and planar staging, for lengths around the block edges."""
import ctypes
import os

import numpy as np
import pytest

from ss_amd import planning as P

hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 15999, 16000, 16384, 16385, 44100, 49152]
CAPS = [16000, 49152]


@pytest.fixture(scope="module")
def stage_lib(tmp_path_factory):
    so = hs.build_driver("stage_spectra", tmp_path_factory.mktemp("stage_spectra"))
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.hs_stage_spectra.argtypes = [vp, ctypes.c_longlong, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp]
    return lib


def _rows(cap, seed):
    """one row per length in LENGTHS (clamped to cap), random samples (signed zeros included) up to the length,
    GARBAGE beyond it in the staging block (the kernel must not read it)"""
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.asarray(LENGTHS, np.int32), cap)
    planar = rng.standard_normal((len(LENGTHS), 2, cap)).astype(np.float32)
    planar[:, :, ::97] = -0.0
    garbage = planar.copy()
    for i, n in enumerate(lens):
        planar[i, :, n:] = 0.0
        garbage[i, :, n:] = np.nan
    return planar, garbage, np.asarray(LENGTHS, np.int32), lens


def _reference(planar):
    """hs_rir_spectra (k_source_windows, scale 1) of the scattered planar rows: [R, 2, hb, SPEC_FLOATS]"""
    R, _, cap = planar.shape
    hb = P.ceil_div(cap, P.KB)
    out = np.zeros((R, 2, hb, P.SPEC_FLOATS), np.float32)
    bank = np.ascontiguousarray(planar)
    rc = hs.lib().hs_rir_spectra(bank.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), R, ctypes.c_longlong(2 * cap), cap, cap)
    assert rc == 0
    return out


@pytest.mark.parametrize("cap", CAPS)
def test_stage_spectra_bit_identical_to_bank_spectra(stage_lib, cap):
    planar, garbage, lens_in, lens = _rows(cap, cap)
    ref = _reference(planar)
    R = planar.shape[0]
    hb = P.ceil_div(cap, P.KB)
    slots = np.asarray([2 * i + 1 for i in range(R)], np.int32)[::-1].copy()      # scattered, out of order
    entries = int(slots.max()) + 2
    for layout in ("wav", "planar"):
        if layout == "wav":
            staged = np.ascontiguousarray(garbage.transpose(0, 2, 1))           # [R, cap, 2]
        else:
            staged = np.ascontiguousarray(garbage)                              # [R, 2, cap]
        hspec = np.full((entries, 2, hb, P.SPEC_FLOATS), 7.0, np.float32)       # sentinel: entries not named stay untouched
        bank_len = np.full((entries,), -5, np.int32)
        rc = stage_lib.hs_stage_spectra(staged.ctypes.data, 2 * cap, int(layout == "planar"), slots.ctypes.data,
                                        lens_in.ctypes.data, R, hspec.ctypes.data, hb, bank_len.ctypes.data)
        assert rc == 0
        for i in range(R):
            got = hspec[slots[i]]
            assert got.view(np.uint32).tobytes() == ref[i].view(np.uint32).tobytes(), (layout, cap, int(lens[i]))
            assert bank_len[slots[i]] == lens[i]
        others = np.setdiff1d(np.arange(entries), slots)
        assert (hspec[others] == 7.0).all() and (bank_len[others] == -5).all()
