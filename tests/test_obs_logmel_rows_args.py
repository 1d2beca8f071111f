"""Argument checks of the one-launch log-mel observation entries for rows of 2 or 3 partition blocks
(ss_audio_obs_logmel_rows_f32 / ss_audio_obs_logmel_rows_spec_f32): the stateless level owns no scratch, so every shape the log-mel
form of the fused row kernels does not serve and every bad mel argument is SS_EINVAL (-1) from the argument checks alone - no
device is touched (dummy pointers, CPU-only machine)."""
import ctypes

import pytest

from ss_amd import _lib
from ss_amd import planning as P

F = ctypes.c_float
ONE = ctypes.c_void_p(16)              # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
FLAG_CROSSFADE = 2                     # SS_FLAG_CROSSFADE of include/ss_hip.h
SR = 44100


def _time(lib, out_len=SR, n_valid=None, flags=0, logmel=ONE, n_mels=64, max_len=36, eps=1e-6, mel_w=ONE, n_units=1, pad_mode=0,
          cap=SR):
    n_valid = out_len if n_valid is None else n_valid
    return lib.ss_audio_obs_logmel_rows_f32(ONE, ONE, ONE, ONE, None, None, logmel, ONE, mel_w, n_mels, max_len, F(eps), n_units,
                                            2 * cap, cap, 1, cap, n_valid, out_len, pad_mode, flags, None)


def _spec(lib, out_len=SR, n_valid=None, flags=0, logmel=ONE, n_mels=64, max_len=36, eps=1e-6, mel_w=ONE, n_units=1, pad_mode=0,
          h_blocks=3):
    n_valid = out_len if n_valid is None else n_valid
    return lib.ss_audio_obs_logmel_rows_spec_f32(ONE, ONE, ONE, ONE, None, None, logmel, ONE, mel_w, n_mels, max_len, F(eps),
                                                 n_units, h_blocks, n_valid, out_len, pad_mode, flags, None)


@pytest.mark.parametrize("entry", [_time, _spec], ids=["time", "spectral"])
def test_unserved_shapes_and_bad_mel_arguments_return_einval_without_a_gpu(entry):
    lib = _lib.load()
    assert entry(lib, n_units=0) == 0                                   # empty batch is a no-op
    assert entry(lib, out_len=P.KB) == -1                               # one partition block: the other pair of entries
    assert entry(lib, out_len=3 * P.KB + 1) == -1                       # more than three partition blocks
    assert entry(lib, out_len=256) == -1
    assert entry(lib, n_valid=SR + 1) == -1                             # n_valid > out_len
    assert entry(lib, n_valid=-1) == -1
    assert entry(lib, flags=FLAG_CROSSFADE) == -1                       # cross-faded steps need the waveform route
    assert entry(lib, logmel=None) == -1
    assert entry(lib, n_mels=0) == -1
    assert entry(lib, n_mels=65) == -1
    assert entry(lib, max_len=23) == -1                                 # not a multiple of 4
    assert entry(lib, max_len=68) == -1
    assert entry(lib, n_mels=64, max_len=52) == -1                      # table of 3328 floats > 3072
    assert entry(lib, eps=0.0) == -1
    assert entry(lib, mel_w=ctypes.c_void_p(20)) == -1                  # unaligned table
    assert entry(lib, pad_mode=7) == -1
    assert entry(lib, n_units=-1) == -1


def test_rir_block_limits():
    lib = _lib.load()
    assert _spec(lib, h_blocks=0) == -1
    assert _spec(lib, h_blocks=17) == -1                                # the pair masks hold 16 RIR blocks per term
    assert _time(lib, cap=0) == -1
    assert _time(lib, cap=16 * P.KB + 1) == -1


def test_rows_policy_of_a_null_context_is_einval():
    lib = _lib.load()
    assert lib.ss_ctx_set_logmel_rows_policy(None, 1, 5) == -1
    assert lib.ss_ctx_wave_scratch_bytes(None) == 0


def test_exports_are_listed():
    for name in ("ss_audio_obs_logmel_rows_f32", "ss_audio_obs_logmel_rows_spec_f32", "ss_ctx_set_logmel_rows_policy"):
        assert name in _lib.EXPORTS
    assert "ss_ctx_wave_scratch_bytes" in _lib.EXPORTS_SIZE and hasattr(_lib.load(), "ss_ctx_wave_scratch_bytes")
