"""Argument checks of the one-launch log-mel observation entries (ss_audio_obs_logmel_f32 / ss_audio_obs_logmel_spec_f32): the
stateless level owns no scratch, so every shape the fused kernels do not serve and every bad mel argument is SS_EINVAL (-1) from
the argument checks alone - no device is touched (dummy pointers, CPU-only machine)."""
import ctypes

import pytest

from ss_amd import _lib
from ss_amd import planning as P

F = ctypes.c_float
ONE = ctypes.c_void_p(16)              # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
FLAG_CROSSFADE = 2                     # SS_FLAG_CROSSFADE of include/ss_hip.h


def _time(lib, out_len=16000, flags=0, logmel=ONE, n_mels=64, max_len=36, eps=1e-6, mel_w=ONE, n_units=1, pad_mode=0):
    return lib.ss_audio_obs_logmel_f32(ONE, ONE, ONE, ONE, None, None, logmel, ONE, mel_w, n_mels, max_len, F(eps), n_units,
                                       2 * 16000, 16000, 1, 16000, min(16000, out_len), out_len, pad_mode, flags, None)


def _spec(lib, out_len=16000, flags=0, logmel=ONE, n_mels=64, max_len=36, eps=1e-6, mel_w=ONE, n_units=1, pad_mode=0):
    return lib.ss_audio_obs_logmel_spec_f32(ONE, ONE, ONE, ONE, None, None, logmel, ONE, mel_w, n_mels, max_len, F(eps), n_units,
                                            1, min(16000, out_len), out_len, pad_mode, flags, None)


@pytest.mark.parametrize("entry", [_time, _spec], ids=["time", "spectral"])
def test_unserved_shapes_and_bad_mel_arguments_return_einval_without_a_gpu(entry):
    lib = _lib.load()
    assert entry(lib, n_units=0) == 0                                   # empty batch is a no-op
    assert entry(lib, out_len=256) == -1                                # too short for the reflect padding
    assert entry(lib, out_len=P.KB + 1) == -1                           # more than one partition block
    assert entry(lib, flags=FLAG_CROSSFADE) == -1                    # cross-faded steps need the waveform route
    assert entry(lib, logmel=None) == -1
    assert entry(lib, n_mels=0) == -1
    assert entry(lib, n_mels=65) == -1
    assert entry(lib, max_len=23) == -1                                 # not a multiple of 4
    assert entry(lib, max_len=68) == -1
    assert entry(lib, n_mels=64, max_len=52) == -1                      # table of 3328 floats > 3072
    assert entry(lib, eps=0.0) == -1
    assert entry(lib, mel_w=ctypes.c_void_p(20)) == -1                  # unaligned table
    assert entry(lib, pad_mode=7) == -1


def test_exports_are_listed():
    for name in ("ss_audio_obs_logmel_f32", "ss_audio_obs_logmel_spec_f32", "ss_ctx_set_logmel_policy"):
        assert name in _lib.EXPORTS
