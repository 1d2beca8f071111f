"""Argument checks of the one-launch log-mel entry for SoundSpaces 2.0 steps (ss_audio_obs_logmel_ss2_f32): it serves cross-faded
one-block rows and rows of which only block 0 is rendered; every other shape and every bad mel argument is SS_EINVAL (-1) from
the argument checks alone - no device is touched (dummy pointers, CPU-only machine)."""
import ctypes

from ss_amd import _lib
from ss_amd import planning as P

F = ctypes.c_float
ONE = ctypes.c_void_p(16)              # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
FLAG_CROSSFADE = 2                     # SS_FLAG_CROSSFADE of include/ss_hip.h


def _ss2(lib, out_len=16000, n_valid=4000, flags=FLAG_CROSSFADE, logmel=ONE, n_mels=64, max_len=36, eps=1e-6, mel_w=ONE,
         n_units=1, pad_mode=0):
    return lib.ss_audio_obs_logmel_ss2_f32(ONE, ONE, ONE, ONE, None, None, logmel, ONE, mel_w, n_mels, max_len, F(eps), n_units,
                                           2 * 16000, 16000, 1, 16000, n_valid, out_len, pad_mode, flags, None)


def test_exports_are_listed():
    for name in ("ss_audio_obs_logmel_ss2_f32", "ss_ctx_set_logmel_ss2_policy"):
        assert name in _lib.EXPORTS


def test_unserved_shapes_and_bad_mel_arguments_return_einval_without_a_gpu():
    lib = _lib.load()
    assert _ss2(lib, n_units=0) == 0                                    # empty batch is a no-op
    assert _ss2(lib, n_units=0, out_len=44100, n_valid=11025, flags=0) == 0
    assert _ss2(lib, out_len=16000, flags=0) == -1                      # plain one-block rows: ss_audio_obs_logmel_f32
    assert _ss2(lib, out_len=256) == -1                                 # too short for the reflect padding
    assert _ss2(lib, out_len=44100, n_valid=P.KB + 1) == -1             # two rendered blocks: the _rows_ entry
    assert _ss2(lib, out_len=44100, n_valid=P.KB + 1, flags=0) == -1
    assert _ss2(lib, out_len=3 * P.KB + 1, n_valid=4000) == -1
    assert _ss2(lib, out_len=3 * P.KB + 1, n_valid=4000, flags=0) == -1
    for shape in (dict(), dict(out_len=44100, n_valid=11025), dict(out_len=44100, n_valid=11025, flags=0)):
        assert _ss2(lib, logmel=None, **shape) == -1
        assert _ss2(lib, n_mels=0, **shape) == -1
        assert _ss2(lib, n_mels=65, **shape) == -1
        assert _ss2(lib, max_len=23, **shape) == -1                     # not a multiple of 4
        assert _ss2(lib, max_len=68, **shape) == -1
        assert _ss2(lib, n_mels=64, max_len=52, **shape) == -1          # table of 3328 floats > 3072
        assert _ss2(lib, eps=0.0, **shape) == -1
        assert _ss2(lib, mel_w=ctypes.c_void_p(20), **shape) == -1      # unaligned table
        assert _ss2(lib, pad_mode=7, **shape) == -1
        assert _ss2(lib, **dict(shape, n_valid=-1)) == -1
