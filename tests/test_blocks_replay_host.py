"""k_obs_blocks with its epoch read from a word of the hand-off area - the form a captured graph replays, k_sync_next in front
(csrc/ss_kernels.hpp) - on the host-compiled kernels (tests/blocks_replay_host.cpp on the host-sim fibers).

Per bank form (k_obs_blocks<false> on fp32 rows, <true> on block spectra) and row length (44 100: three output blocks, 22 050:
two): ONE hand-off area, zeroed once as the library zeroes it, then
    replay 1, replay 2, an eager launch with a positive kernel-argument epoch, replay 3
each on other unit descriptors (tests/replay_plan.py: two live units - one with a distractor term - and a silent one, their slots,
window starts and bank entries moving with the step).  Every run is compared with the kernel-argument form of the same inputs
over a fresh private area: BIT-equal waveform and spectrogram (the same instructions on the same numbers; a consumer whose epoch
does not match its producer's flag poisons its first frames with NaN on this build, so a wrong epoch cannot pass).  The flag words
of the rows a run rendered hold that run's epoch afterwards: -k after replay k, the positive epoch after the eager launch; the
epoch word holds -k after replay k and is not moved by the eager launch.  Every output is pre-filled with NaN."""
import ctypes

import numpy as np
import pytest

from ss_amd import planning as P

import replay_plan as RP
hs = pytest.importorskip("hostsim.hs")

EAGER_EPOCH = 5


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("blocks_replay", tmp_path_factory.mktemp("blocks_replay"))
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hs_obs_blocks_replay.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    lib.hs_rir_spectra.argtypes = [vp, vp, ci, ctypes.c_longlong, ci, ci]
    lib.hs_replay_area_reset.argtypes = [ci]
    lib.hs_replay_area_flags.argtypes = [vp, ci]
    return lib


def _run(lib, mode, epoch, w, spectral, k, sr):
    """step k in `mode` (tests/blocks_replay_host.cpp) -> (waveform, spectrogram, live rows)"""
    clips, bank, lens, hspec = w
    units = RP.step_units(k, sr)
    wd, desc = RP.plan(units, clips.shape[1], sr)
    flat = np.ascontiguousarray(clips.reshape(-1))
    spec = np.zeros((len(wd), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    n = len(units)
    wave = np.full((n, 2, sr), np.nan, np.float32)
    sg = np.full((n,) + P.spectrogram_shape(sr), np.nan, np.float32)
    rc = lib.hs_obs_blocks_replay(mode, epoch, spec.ctypes.data, bank.ctypes.data, hspec.ctypes.data if spectral else None,
                                  lens.ctypes.data, desc.ctypes.data, wave.ctypes.data, sg.ctypes.data, n, RP.RIR_CAP, 1, sr)
    assert rc == 0, rc
    live = [2 * i + c for i, u in enumerate(units) if u.get("rir", -1) >= 0 for c in range(2)]
    return wave, sg, live


def _area(lib, n_rows):
    out = np.zeros((2 * n_rows + 1,), np.int32)
    assert lib.hs_replay_area_flags(out.ctypes.data, len(out)) == 0
    return out[:-1], int(out[-1])


@pytest.mark.parametrize("sr", [44100, 22050], ids=["3-blocks", "2-blocks"])
@pytest.mark.parametrize("spectral", [False, True], ids=["rows", "spectra"])
def test_replays_over_one_area_equal_the_kernel_argument_form(lib, spectral, sr):
    clips, bank, lens = RP.world(sr, seed=sr)
    hspec = np.zeros((RP.N_BANK, 2, 1, P.SPEC_FLOATS), np.float32)
    assert lib.hs_rir_spectra(bank.ctypes.data, hspec.ctypes.data, RP.N_BANK, 2 * RP.RIR_CAP, RP.RIR_CAP, RP.RIR_CAP) == 0
    w = (clips, bank, lens, hspec)
    n_rows, nb = 6, P.ceil_div(sr, P.KB)
    lib.hs_replay_area_reset(n_rows)
    flags, word = _area(lib, n_rows)
    assert word == 0 and not flags.any()
    # (mode, what the rendered rows' flags and the epoch word hold afterwards)
    schedule = [(1, -1, -1), (1, -2, -2), (2, EAGER_EPOCH, -2), (1, -3, -3)]
    for k, (mode, want_flag, want_word) in enumerate(schedule):
        wave, sg, live = _run(lib, mode, EAGER_EPOCH, w, spectral, k, sr)
        ref_wave, ref_sg, _ = _run(lib, 0, 7, w, spectral, k, sr)
        assert not np.isnan(ref_wave).any() and not np.isnan(ref_sg).any()
        assert np.array_equal(wave.view(np.uint32), ref_wave.view(np.uint32)), (k, mode)
        assert np.array_equal(sg.view(np.uint32), ref_sg.view(np.uint32)), (k, mode)
        assert all(np.abs(wave[r // 2, r % 2]).max() > 0 for r in live) and len(live) == 4
        flags, word = _area(lib, n_rows)
        assert word == want_word, (k, word)
        used = [r * (nb - 1) + j for r in live for j in range(nb - 1)]
        assert [int(flags[i]) for i in used] == [want_flag] * len(used), (k, flags)
        others = set(range(n_rows * (nb - 1))) - set(used)         # the silent unit's rows: whatever an earlier run left
        assert all(int(flags[i]) != want_flag for i in others), (k, flags)


def test_replay_epochs_are_negative_and_wrap_to_minus_one(lib):
    lib.hs_next_replay_epoch.argtypes = [ctypes.c_int]
    lib.hs_next_replay_epoch.restype = ctypes.c_int
    nxt = lib.hs_next_replay_epoch
    assert nxt(0) == -1 and nxt(-1) == -2 and nxt(-0x7ffffffe) == -0x7fffffff and nxt(-0x7fffffff) == -1
    assert nxt(12345) == -1                                        # (never written there; a replay epoch all the same)
