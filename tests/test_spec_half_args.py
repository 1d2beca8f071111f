"""Half-precision spectral RIR bank: every refusal of its entry points is SS_EINVAL (-1) from the argument checks, before a device
is touched (this file runs without a GPU), and the Python layers raise ValueError before they allocate anything."""
import ctypes

import pytest

from ss_amd import _lib, ops, planning as P

KB = P.KB
F = ctypes.c_float
ONE = ctypes.c_void_p(16)           # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
ODD = ctypes.c_void_p(20)           # ... and one that is not 8-byte aligned
NULL = None
XF = ops.FLAG_CROSSFADE


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_and_exported(lib):
    for name in ("ss_rir_spectra16_f32", "ss_bank_scatter_spectra16_f32", "ss_fftconv_binaural_spec16_f32", "ss_audio_obs_spec16_f32",
                 "ss_audio_obs_logmel_spec16_f32", "ss_ctx_set_rir_spectra16"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None


def test_conv_entry_refusals(lib):
    f = lib.ss_fftconv_binaural_spec16_f32
    #        spec hspec16 hscale rir_len desc out  n  hb  n_valid out_len flags stream
    assert f(ONE, ONE, ONE, ONE, ONE, ONE, 0, 1, 16000, 16000, 0, NULL) == 0          # no units: nothing to do
    assert f(ONE, ONE, NULL, ONE, ONE, ONE, 2, 1, 16000, 16000, 0, NULL) == -1        # null hscale
    assert f(ONE, NULL, ONE, ONE, ONE, ONE, 2, 1, 16000, 16000, 0, NULL) == -1        # null bank
    assert f(ONE, ODD, ONE, ONE, ONE, ONE, 2, 1, 16000, 16000, 0, NULL) == -1         # bank not 8-byte aligned
    assert f(ONE, ONE, ONE, ONE, ONE, ONE, 2, 0, 16000, 16000, 0, NULL) == -1         # h_blocks < 1
    assert f(ONE, ONE, ONE, ONE, ONE, ONE, 2, 1, 16000, 16000, XF, NULL) == -1        # cross-fade
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, 2, 1, 16000, 16000, 0, NULL) == -1        # no output
    assert f(ONE, ONE, ONE, ONE, ONE, ONE, -1, 1, 16000, 16000, 0, NULL) == -1
    assert f(ONE, ONE, ONE, ONE, ONE, ONE, 2, 1, 16001, 16000, 0, NULL) == -1         # n_valid > out_len
    assert f(ONE, ONE, ONE, ONE, ONE, ONE, 2, 4, 3 * KB + 1, 4 * KB, 0, NULL) == -1   # more than three output blocks
    assert f(NULL, ONE, ONE, ONE, ONE, ONE, 2, 1, 16000, 16000, 0, NULL) == -1        # null window spectra


def test_fused_entry_refusals(lib):
    f = lib.ss_audio_obs_spec16_f32
    #        spec hspec16 hscale rir_len desc ag   sgram n  hb n_valid out_len pad flags stream
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, ONE, 0, 1, 16000, 16000, 0, 0, NULL) == 0
    assert f(ONE, ONE, NULL, ONE, ONE, NULL, ONE, 2, 1, 16000, 16000, 0, 0, NULL) == -1     # null hscale
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, ONE, 2, 0, 16000, 16000, 0, 0, NULL) == -1      # h_blocks < 1
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, ONE, 2, 1, 16000, 16000, 0, XF, NULL) == -1     # cross-fade
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, NULL, 2, 1, 16000, 16000, 0, 0, NULL) == -1     # no spectrogram
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, ONE, 2, 1, 16000, 16000, 7, 0, NULL) == -1      # unknown pad mode
    for out_len in (KB + 1, 44100, 48000):                                                # rows longer than one partition block
        assert f(ONE, ONE, ONE, ONE, ONE, ONE, ONE, 2, 3, out_len, out_len, 0, 0, NULL) == -1
    assert f(ONE, ONE, ONE, ONE, ONE, NULL, ONE, 2, 1, 256, 256, 0, 0, NULL) == -1          # shorter than the reflect padding
    assert f(ONE, ODD, ONE, ONE, ONE, NULL, ONE, 2, 1, 16000, 16000, 0, 0, NULL) == -1


def test_logmel_entry_refusals(lib):
    f = lib.ss_audio_obs_logmel_spec16_f32

    def call(hscale=ONE, hb=1, n_mels=64, max_len=24, eps=1e-6, out_len=16000, flags=0, logmel=ONE, mel_w=ONE, n=2, pad=0):
        return f(ONE, ONE, hscale, ONE, ONE, NULL, NULL, logmel, ONE, mel_w, n_mels, max_len, F(eps), n, hb, out_len, out_len, pad,
                 flags, NULL)

    assert call(n=0) == 0
    assert call(hscale=NULL) == -1
    assert call(hb=0) == -1
    assert call(flags=XF) == -1
    assert call(out_len=KB + 1) == -1 and call(out_len=44100) == -1 and call(out_len=256) == -1
    assert call(logmel=NULL) == -1
    assert call(n_mels=65) == -1 and call(n_mels=0) == -1                  # the mel limits of ss_audio_features_f32
    assert call(max_len=23) == -1 and call(max_len=68) == -1 and call(max_len=0) == -1
    assert call(n_mels=64, max_len=52) == -1                               # n_mels * max_len > 3072
    assert call(eps=0.0) == -1
    assert call(mel_w=ODD) == -1                                           # table not 16-byte aligned
    assert call(pad=7) == -1


def test_producer_refusals(lib):
    s = lib.ss_bank_scatter_spectra16_f32
    #        staged stride planar slots lens n  hspec16 hscale hb bank_len stream
    assert s(ONE, 32000, 0, ONE, ONE, 0, ONE, ONE, 1, ONE, NULL) == 0
    assert s(ONE, 32000, 0, ONE, ONE, 2, ONE, NULL, 1, ONE, NULL) == -1        # null hscale
    assert s(ONE, 32000, 0, ONE, ONE, 2, NULL, ONE, 1, ONE, NULL) == -1
    assert s(ONE, 32000, 0, ONE, ONE, 2, ONE, ONE, 0, ONE, NULL) == -1         # h_blocks < 1
    assert s(NULL, 32000, 0, ONE, ONE, 2, ONE, ONE, 1, ONE, NULL) == -1
    assert s(ONE, 32001, 0, ONE, ONE, 2, ONE, ONE, 1, ONE, NULL) == -1         # odd row stride
    assert s(ONE, 32002, 1, ONE, ONE, 2, ONE, ONE, 1, ONE, NULL) == -1         # planar: the second ear must be 8-byte aligned
    assert s(ODD, 32000, 0, ONE, ONE, 2, ONE, ONE, 1, ONE, NULL) == -1
    assert s(ONE, 32000, 0, ONE, ONE, 2, ODD, ONE, 1, ONE, NULL) == -1
    r = lib.ss_rir_spectra16_f32
    #        rir hspec16 hscale n  unit_stride chan_stride cap stream
    assert r(ONE, ONE, ONE, 0, 32000, 16000, 16000, NULL) == 0
    assert r(ONE, ONE, NULL, 2, 32000, 16000, 16000, NULL) == -1
    assert r(ONE, NULL, ONE, 2, 32000, 16000, 16000, NULL) == -1
    assert r(NULL, ONE, ONE, 2, 32000, 16000, 16000, NULL) == -1
    assert r(ONE, ONE, ONE, 2, 32000, 16000, 0, NULL) == -1
    assert r(ONE, ODD, ONE, 2, 32000, 16000, 16000, NULL) == -1
    assert r(ONE, ONE, ONE, -1, 32000, 16000, 16000, NULL) == -1


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


def test_context_refusals(lib):
    h = _ctx(lib, 16000)
    try:
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, 16000) == 0            # the spectral-only binding's first half
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, NULL, 1) == -1                    # null hscale
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 0) == -1                     # h_blocks < 1
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 2) == -1                     # ... or not ceil(rir_cap / kB)
        assert lib.ss_ctx_set_rir_spectra16(h, ODD, ONE, 1) == -1
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 1) == 0
        assert lib.ss_ctx_set_rir_spectra(h, ONE, 1) == -1                            # fp32 spectra next to the half ones
        assert lib.ss_ctx_set_rir_spectra16(h, NULL, NULL, 0) == 0                    # unbind ...
        assert lib.ss_ctx_set_rir_spectra(h, ONE, 1) == 0                             # ... now the fp32 form binds,
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 1) == -1                     # and the half one is refused next to it
        assert lib.ss_ctx_set_rir_spectra(h, NULL, 0) == 0
        assert lib.ss_ctx_set_rir_bank(h, ONE, ONE, 32000, 16000, 1, 16000) == 0      # a bank that keeps time-domain rows
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 1) == -1
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, 40000) == 0             # three blocks per row: fine at 16 kHz
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 3) == 0
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, 16000) == 0             # a new bank drops the binding
        assert lib.ss_ctx_set_rir_spectra(h, ONE, 1) == 0
    finally:
        lib.ss_ctx_destroy(h)
    for sr in (44100, 48000):                                                         # rows longer than one partition block
        h = _ctx(lib, sr)
        try:
            assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, sr) == 0
            assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, P.ceil_div(sr, KB)) == -1
            assert lib.ss_ctx_set_rir_spectra(h, ONE, P.ceil_div(sr, KB)) == 0        # (the fp32 spectral-only binding serves them)
        finally:
            lib.ss_ctx_destroy(h)
    assert lib.ss_ctx_set_rir_spectra16(NULL, ONE, ONE, 1) == -1


def test_store_and_engine_value_errors():
    from ss_amd.renderer import AudioEngine, BucketedRirStore, RirStore
    with pytest.raises(ValueError):
        RirStore(8, 16000, "cpu", spectral="half")                       # no CPU form of a spectral-only bank
    with pytest.raises(ValueError):
        RirStore(8, 16000, "cpu", spectral="quarter")
    with pytest.raises(ValueError):
        BucketedRirStore([8, 4], [16000, 2 * KB], "cpu", spectral="half")
    with pytest.raises(ValueError):
        AudioEngine(16000, device="cpu", rir_spectral="half", step_time=0.25)                         # SoundSpaces 2.0
    with pytest.raises(ValueError):
        AudioEngine(16000, device="cpu", rir_spectral="half", wrap=True)
    with pytest.raises(ValueError):
        AudioEngine(16000, device="cpu", rir_spectral="half", rir_buckets=[(8, 16000), (4, 2 * KB)])
    with pytest.raises(ValueError):
        AudioEngine(16000, device="cpu", rir_spectral="half", spectral_max_units=64)
    for sr in (44100, 48000):                                            # rows longer than one partition block
        with pytest.raises(ValueError, match="one partition block"):
            AudioEngine(sr, device="cpu", rir_spectral="half")
    with pytest.raises(ValueError):
        AudioEngine(16000, device="cpu", rir_spectral="fp8")
