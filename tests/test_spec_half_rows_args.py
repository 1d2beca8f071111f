"""Half-precision spectral RIR bank for rows of 2 or 3 partition blocks (44.1 / 48 kHz): every refusal of the new entry points is
SS_EINVAL (-1) from the argument checks, before a device is touched (this file runs without a GPU); the new context binding is
accepted where the old one is refused and the other way round; the engine's opt-in keyword."""
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
    for name in ("ss_audio_obs_rows_spec16_f32", "ss_audio_obs_logmel_rows_spec16_f32", "ss_ctx_set_rir_spectra16_rows"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None


def test_rows_entry_refusals(lib):
    f = lib.ss_audio_obs_rows_spec16_f32

    def call(spec=ONE, bank=ONE, hscale=ONE, ag=NULL, sgram=ONE, n=2, hb=3, n_valid=None, out_len=44100, pad=0, flags=0):
        return f(spec, bank, hscale, ONE, ONE, ag, sgram, n, hb, out_len if n_valid is None else n_valid, out_len, pad, flags, NULL)

    assert call(n=0) == 0                                                  # no units: nothing to do
    assert call(flags=XF) == -1                                            # cross-fade
    assert call(bank=NULL) == -1 and call(bank=ODD) == -1                  # null / misaligned halves
    assert call(hscale=NULL) == -1                                         # null scales
    assert call(hb=0) == -1 and call(hb=17) == -1 and call(hb=-1) == -1    # h_blocks outside 1..16
    for out_len in (256, 16000, KB):                                       # one partition block: the 16 kHz entry's rows
        assert call(out_len=out_len) == -1
    assert call(out_len=3 * KB + 1) == -1 and call(out_len=65536) == -1    # more than three
    assert call(sgram=NULL) == -1                                          # no spectrogram
    assert call(pad=7) == -1
    assert call(n=-1) == -1
    assert call(n_valid=44101) == -1 and call(n_valid=-1) == -1
    assert call(spec=NULL) == -1
    assert call(n=0, flags=XF, bank=NULL) == 0                             # (n_units == 0 comes first)
    for out_len in (KB + 1, 20000, 48000, 3 * KB):                         # (the served lengths get past the checks: n = 0 only here)
        assert call(n=0, out_len=out_len) == 0


def test_logmel_rows_entry_refusals(lib):
    f = lib.ss_audio_obs_logmel_rows_spec16_f32

    def call(bank=ONE, hscale=ONE, hb=3, n_mels=64, max_len=24, eps=1e-6, out_len=44100, n_valid=None, flags=0, logmel=ONE, mel_w=ONE,
             n=2, pad=0, ag=NULL, sgram=NULL):
        return f(ONE, bank, hscale, ONE, ONE, ag, sgram, logmel, ONE, mel_w, n_mels, max_len, F(eps), n, hb,
                 out_len if n_valid is None else n_valid, out_len, pad, flags, NULL)

    assert call(n=0) == 0
    assert call(n=0, ag=ONE, sgram=ONE) == 0                               # (audiogoal and spectrogram are optional)
    assert call(flags=XF) == -1
    assert call(bank=NULL) == -1 and call(bank=ODD) == -1
    assert call(hscale=NULL) == -1
    assert call(hb=0) == -1 and call(hb=17) == -1
    assert call(out_len=16000) == -1 and call(out_len=KB) == -1 and call(out_len=3 * KB + 1) == -1
    assert call(n_valid=48000) == -1
    assert call(logmel=NULL) == -1
    assert call(n_mels=65) == -1 and call(n_mels=0) == -1                  # the mel limits of ss_audio_features_f32
    assert call(max_len=23) == -1 and call(max_len=68) == -1 and call(max_len=0) == -1
    assert call(n_mels=64, max_len=52) == -1                               # n_mels * max_len > 3072
    assert call(eps=0.0) == -1
    assert call(mel_w=ODD) == -1                                           # table not 16-byte aligned
    assert call(pad=7) == -1


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


@pytest.mark.parametrize("sr", [44100, 48000])
def test_context_binding_on_long_rows(lib, sr):
    hb = P.ceil_div(sr, KB)
    h = _ctx(lib, sr)
    try:
        bind = lib.ss_ctx_set_rir_spectra16_rows
        assert bind(h, ONE, ONE, hb) == -1                                            # no bank yet (rir_len unset)
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, sr) == 0                # the spectral-only binding's first half
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, hb) == -1                    # the old binding is still refused here
        assert bind(h, ONE, NULL, hb) == -1                                           # null hscale
        assert bind(h, ODD, ONE, hb) == -1
        assert bind(h, ONE, ONE, 0) == -1 and bind(h, ONE, ONE, hb - 1) == -1         # h_blocks must be ceil(rir_cap / kB)
        assert bind(h, ONE, ONE, hb) == 0
        assert lib.ss_ctx_set_rir_spectra(h, ONE, hb) == -1                           # fp32 spectra next to the half ones
        assert bind(h, ONE, ONE, hb) == 0                                             # (rebinding a half bank is fine)
        assert bind(h, NULL, NULL, 0) == 0                                            # unbind ...
        assert lib.ss_ctx_set_rir_spectra(h, ONE, hb) == 0                            # ... now the fp32 form binds,
        assert bind(h, ONE, ONE, hb) == -1                                            # and the half one is refused next to it
        assert lib.ss_ctx_set_rir_spectra(h, NULL, 0) == 0
        assert lib.ss_ctx_set_rir_bank(h, ONE, ONE, 2 * sr, sr, 1, sr) == 0           # a bank that keeps time-domain rows
        assert bind(h, ONE, ONE, hb) == -1
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, 16 * KB) == 0           # 16 blocks per row: the most the kernels take
        assert bind(h, ONE, ONE, 16) == 0
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, 16 * KB + 1) == 0
        assert bind(h, ONE, ONE, 17) == -1
    finally:
        lib.ss_ctx_destroy(h)
    assert lib.ss_ctx_set_rir_spectra16_rows(NULL, ONE, ONE, hb) == -1


def test_context_binding_refused_on_one_block_rows(lib):
    h = _ctx(lib, 16000)
    try:
        assert lib.ss_ctx_set_rir_bank(h, NULL, ONE, 0, 0, 1, 16000) == 0
        assert lib.ss_ctx_set_rir_spectra16_rows(h, ONE, ONE, 1) == -1
        assert lib.ss_ctx_set_rir_spectra16(h, ONE, ONE, 1) == 0                      # (the 16 kHz binding serves them)
        assert lib.ss_ctx_set_rir_spectra16_rows(h, NULL, NULL, 0) == 0               # NULL unbinds whatever half bank is bound
        assert lib.ss_ctx_set_rir_spectra(h, ONE, 1) == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_engine_keyword():
    from ss_amd.renderer import AudioEngine
    for sr in (44100, 48000):
        with pytest.raises(ValueError, match="one partition block"):                  # without the keyword: as before
            AudioEngine(sr, device="cpu", rir_spectral="half")
        with pytest.raises(ValueError, match="one partition block"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_half_rows=False)
    with pytest.raises(ValueError):
        AudioEngine(44100, device="cpu", rir_spectral="half", rir_half_rows=True, step_time=0.25)       # SoundSpaces 2.0
    with pytest.raises(ValueError):
        AudioEngine(44100, device="cpu", rir_spectral="half", rir_half_rows=True, wrap=True)
    with pytest.raises(ValueError):
        AudioEngine(44100, device="cpu", rir_spectral="half", rir_half_rows=True, rir_buckets=[(8, 44100), (4, 4 * KB)])
    with pytest.raises(ValueError):
        AudioEngine(44100, device="cpu", rir_spectral="half", rir_half_rows=True, spectral_max_units=64)
    with pytest.raises(ValueError, match="three partition blocks"):
        AudioEngine(96000, device="cpu", rir_spectral="half", rir_half_rows=True)     # rates above 3 kB are not served
    for other in (None, True, False, "only"):
        with pytest.raises(ValueError, match="rir_half_rows"):
            AudioEngine(44100, device="cpu", rir_spectral=other, rir_half_rows=True)  # the keyword belongs to the half store
    for sr in (44100, 48000):                                                         # the opt-in passes every argument check:
        with pytest.raises(_lib.SsHipError, match="no CPU path"):                     # only the missing device stops it here
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_half_rows=True)
