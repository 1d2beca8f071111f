"""Half-precision time-domain RIR rows (include/ss_hip.h "Half-precision time-domain rows": ``ss_rir_rows16_f32``,
``ss_bank_scatter_rows16_f32``, ``ss_fftconv_binaural_rir16_f32``, ``ss_audio_obs_rir16_f32``, ``ss_ctx_set_rir_bank16``): every
refusal is SS_EINVAL (-1) from the argument checks, before a device is touched (this file runs without a GPU: a call that got
past the checks would come back with a HIP error, not -1); n_units == 0 returns 0; the binding replaces and is replaced; and
``RirStore`` / ``AudioEngine`` raise ValueError before they allocate anything."""
import ctypes

import numpy as np
import pytest

from ss_amd import _lib, ops, planning as P

KB = P.KB
ONE = 16                            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
NULL = None
P1 = ctypes.c_void_p(ONE)
ODD2 = ctypes.c_void_p(18)          # 2-byte aligned only: not a base for 4-byte loads
AL4 = ctypes.c_void_p(20)           # 4-byte aligned is enough
XF = ops.FLAG_CROSSFADE
BAD_CAPS = (0, 1, 15999, -2, 16 * KB + 2)       # < 2, odd, negative, more than 16 partition blocks


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_and_exported(lib):
    for name in ("ss_rir_rows16_f32", "ss_bank_scatter_rows16_f32", "ss_fftconv_binaural_rir16_f32", "ss_audio_obs_rir16_f32",
                 "ss_ctx_set_rir_bank16"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    for name in ("rir_rows16", "scatter_rows16_into", "fftconv_binaural_rir16_into", "audio_obs_rir16_into"):
        assert hasattr(ops, name)
    from ss_amd.context import AudioContext
    assert hasattr(AudioContext, "set_rir_bank16")


def test_rows16_producer_refusals(lib):
    f = lib.ss_rir_rows16_f32
    #        rir rir16 rscale n us cs cap stream
    assert f(P1, P1, P1, 0, 32000, 16000, 16000, NULL) == 0                            # no entries: nothing to do
    assert f(NULL, NULL, NULL, 0, 0, 0, 0, NULL) == 0
    assert f(NULL, P1, P1, 2, 32000, 16000, 16000, NULL) == -1
    assert f(P1, NULL, P1, 2, 32000, 16000, 16000, NULL) == -1                         # null halves
    assert f(P1, P1, NULL, 2, 32000, 16000, 16000, NULL) == -1                         # null scales
    assert f(P1, ODD2, P1, 2, 32000, 16000, 16000, NULL) == -1                         # base not 4-byte aligned
    assert f(P1, P1, P1, -1, 32000, 16000, 16000, NULL) == -1
    assert f(P1, P1, P1, 2, -1, 16000, 16000, NULL) == -1 and f(P1, P1, P1, 2, 32000, -1, 16000, NULL) == -1
    for cap in BAD_CAPS:
        assert f(P1, P1, P1, 2, 32000, 16000, cap, NULL) == -1, cap


def test_scatter_rows16_refusals(lib):
    f = lib.ss_bank_scatter_rows16_f32
    #        staged stride slots lens n rir16 rscale cap bank_len stream
    assert f(P1, 32000, P1, P1, 0, P1, P1, 16000, P1, NULL) == 0
    assert f(NULL, 0, NULL, NULL, 0, NULL, NULL, 0, NULL, NULL) == 0
    assert f(NULL, 32000, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 32000, NULL, P1, 2, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 32000, P1, NULL, 2, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 32000, P1, P1, 2, NULL, P1, 16000, P1, NULL) == -1                    # null halves
    assert f(P1, 32000, P1, P1, 2, P1, NULL, 16000, P1, NULL) == -1                    # null scales
    assert f(P1, 32000, P1, P1, 2, ODD2, P1, 16000, P1, NULL) == -1                    # misaligned halves
    assert f(P1, 32000, P1, P1, -1, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 31998, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1                      # rows shorter than the capacity
    assert f(P1, 32001, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1                      # odd stride: frames are 8-byte loads
    assert f(AL4, 32000, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1                     # staged not 8-byte aligned
    for cap in BAD_CAPS:
        assert f(P1, 1 << 20, P1, P1, 2, P1, P1, cap, P1, NULL) == -1, cap
    # pageable host memory: refused, not dereferenced (the pointer attributes are asked before anything is launched)
    staged = np.zeros((2, 16000, 2), np.float32)
    idx, lens = np.zeros((2,), np.int32), np.zeros((2,), np.int32)
    assert f(staged.ctypes.data, 32000, idx.ctypes.data, lens.ctypes.data, 2, P1, P1, 16000, NULL, NULL) == -1


def test_fftconv_rir16_refusals(lib):
    f = lib.ss_fftconv_binaural_rir16_f32

    def call(spec=P1, rir16=P1, rscale=P1, lens=P1, desc=P1, out=P1, n=2, cap=16000, n_valid=16000, out_len=16000, flags=0):
        return f(spec, rir16, rscale, lens, desc, out, n, cap, n_valid, out_len, flags, NULL)

    assert call(n=0) == 0 and call(n=0, rir16=NULL, rscale=NULL, out=NULL, cap=0) == 0
    assert call(rir16=NULL) == -1 and call(rscale=NULL) == -1 and call(rir16=ODD2) == -1
    for cap in BAD_CAPS:
        assert call(cap=cap) == -1, cap
    assert call(flags=XF) == -1 and call(flags=XF | ops.FLAG_NO_DISTRACTOR) == -1
    assert call(out=NULL) == -1                                                        # the required output
    assert call(spec=NULL) == -1 and call(lens=NULL) == -1 and call(desc=NULL) == -1
    assert call(n=-1) == -1
    assert call(n_valid=16001) == -1 and call(n_valid=-1) == -1 and call(out_len=0, n_valid=0) == -1
    assert call(n_valid=3 * KB + 1, out_len=4 * KB) == -1                              # more than three output blocks
    for sr in (44100, 48000):                                                          # (the same at the longer rows)
        assert call(n_valid=sr, out_len=sr, cap=sr, flags=XF) == -1
        assert call(n_valid=sr, out_len=sr, cap=sr, out=NULL) == -1


def test_audio_obs_rir16_refusals(lib):
    f = lib.ss_audio_obs_rir16_f32

    def call(spec=P1, rir16=P1, rscale=P1, lens=P1, desc=P1, ag=NULL, sg=P1, n=2, cap=16000, n_valid=16000, out_len=16000, pad=0,
             flags=0):
        return f(spec, rir16, rscale, lens, desc, ag, sg, n, cap, n_valid, out_len, pad, flags, NULL)

    assert call(n=0) == 0 and call(n=0, rir16=NULL, rscale=NULL, sg=NULL) == 0
    for ag in (NULL, P1):                                                              # `audiogoal` is optional, everything else is not
        assert call(ag=ag, rir16=NULL) == -1 and call(ag=ag, rscale=NULL) == -1 and call(ag=ag, rir16=ODD2) == -1
        for cap in BAD_CAPS:
            assert call(ag=ag, cap=cap) == -1, cap
        assert call(ag=ag, flags=XF) == -1
        assert call(ag=ag, sg=NULL) == -1                                              # the required output
        assert call(ag=ag, pad=7) == -1 and call(ag=ag, pad=-1) == -1
        assert call(ag=ag, spec=NULL) == -1 and call(ag=ag, lens=NULL) == -1 and call(ag=ag, desc=NULL) == -1
        assert call(ag=ag, n=-1) == -1
        assert call(ag=ag, n_valid=16001) == -1 and call(ag=ag, n_valid=-1) == -1
        for out_len in (1, 256, KB + 1, 16385, 44100, 48000, 4 * KB):                  # outside the fused entry's range
            assert call(ag=ag, out_len=out_len, n_valid=min(out_len, KB)) == -1, out_len


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


@pytest.mark.parametrize("sr", [16000, KB, 44100, 48000])
def test_context_binding(lib, sr):
    s = lib.ss_ctx_set_rir_bank16
    h = _ctx(lib, sr)
    try:
        assert s(NULL, P1, P1, P1, 16000) == -1
        assert s(h, P1, NULL, P1, 16000) == -1                                         # null scales
        assert s(h, ODD2, P1, P1, 16000) == -1                                         # misaligned halves
        assert s(h, P1, P1, NULL, 16000) == -1                                         # no lengths
        for cap in BAD_CAPS:
            assert s(h, P1, P1, P1, cap) == -1, cap
        assert s(h, NULL, NULL, NULL, 0) == 0                                          # unbinding nothing is fine
        assert s(h, P1, P1, P1, 16000) == 0 and s(h, AL4, P1, P1, 40000) == 0          # (re)binding, at any capacity up to 16 blocks
        # one form at a time: no spectra next to the half rows ...
        assert lib.ss_ctx_set_rir_spectra(h, P1, 3) == -1
        assert lib.ss_ctx_set_rir_spectra16(h, P1, P1, 3) == -1
        assert lib.ss_ctx_set_rir_spectra16_rows(h, P1, P1, 3) == -1
        # ... and every other bank call replaces them: the spectral bindings work again
        assert lib.ss_ctx_set_rir_bank(h, NULL, P1, 0, 0, 1, 16000) == 0
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == 0
        assert s(h, P1, P1, P1, 16000) == 0                                            # replaces any earlier binding (fp32 spectra here)
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == -1
        assert s(h, NULL, NULL, NULL, 0) == 0                                          # NULL unbinds
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_context_plans_at_the_half_banks_depth(lib):
    """the planner alone (host only): planning depth = the rows' blocks + the output's blocks - 1, as for any bank"""
    from ss_amd.context import AudioContext
    ctx = AudioContext(44100)
    try:
        ctx.add_source_len("a", 44100)
        assert lib.ss_ctx_set_rir_bank16(ctx._h, P1, P1, P1, 40000) == 0
        assert ctx.stats()["slots_per_key"] == 3 + 3 - 1
        plan = ctx.plan(np.asarray([0, 0], np.int32), np.asarray([0, 0], np.int32), np.asarray([0, 2], np.int32))
        assert plan[1] == ops.FLAG_NO_DISTRACTOR
    finally:
        ctx.close()


def test_in_call_file_loader_answers_not_served(lib):
    """ss_ctx_load_rir_files on a context bound to half rows: 1 (not served), before its loader struct is looked at"""
    h = _ctx(lib, 16000)
    try:
        assert lib.ss_ctx_set_rir_bank16(h, P1, P1, P1, 16000) == 0
        ld = _lib.SsMissLoader()
        paths = (ctypes.c_char_p * 1)(b"/nonexistent.wav")
        assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 4, NULL) == 1
        assert ld.n_loaded == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_store_and_engine_value_errors():
    from ss_amd.renderer import AudioEngine, RirStore
    with pytest.raises(ValueError, match="rows must be None or 'half'"):
        RirStore(4, 16000, "cpu", rows="quarter")
    with pytest.raises(ValueError, match="GPU"):
        RirStore(4, 16000, "cpu", rows="half")
    for spectral in (True, "only", "half"):
        with pytest.raises(ValueError, match="does not go with spectral"):
            RirStore(4, 16000, "cpu", rows="half", spectral=spectral)
    with pytest.raises(ValueError, match="rir_rows must be None or 'half'"):
        AudioEngine(16000, device="cpu", rir_rows="fp8")
    for sr in (16000, 44100, 48000):
        for spectral in (True, "only", "half"):
            with pytest.raises(ValueError, match="does not go with rir_spectral"):
                AudioEngine(sr, device="cpu", rir_rows="half", rir_spectral=spectral)
        with pytest.raises(ValueError, match="rir_buckets"):
            AudioEngine(sr, device="cpu", rir_rows="half", rir_buckets=[(8, 16384), (4, 3 * KB)])
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(sr, device="cpu", rir_rows="half", step_time=0.25)
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(sr, device="cpu", rir_rows="half", wrap=True)
        with pytest.raises(ValueError, match="GPU"):                                   # accepted at every rate up to 3 KB - on a GPU
            AudioEngine(sr, device="cpu", rir_rows="half")
    with pytest.raises(ValueError, match="three partition blocks"):
        AudioEngine(96000, device="cuda", rir_rows="half")


def test_engine_hands_the_form_to_the_store(monkeypatch):
    """the constructor's plumbing, without a device"""
    import types
    from ss_amd import renderer as Rn
    seen = {}

    class Store:
        def __init__(self, slots, cap, device, **kw):
            seen.update(kw, slots=slots, cap=cap)
            self.bank = types.SimpleNamespace(cap=cap)

    class Renderer:
        def __init__(self, sr, device="cuda", **kw):
            self.sr = self.n_valid = self.out_len = int(sr)
            self.wrap, self.device = False, "cuda"

        def set_rir_bank(self, bank):
            self.rirs = bank

    monkeypatch.setattr(Rn, "RirStore", Store)
    monkeypatch.setattr(Rn, "BatchedAudioRenderer", Renderer)
    for sr in (16000, 44100, 48000):
        eng = Rn.AudioEngine(sr, device="cuda", rir_slots=6, rir_rows="half")
        assert seen["rows"] == "half" and seen["spectral"] is False and seen["cap"] == sr and seen["slots"] == 6
        assert eng.rir_rows_half and not eng.rir_spectral and not eng.rir_spectral_only and eng.renderer.rirs is eng.store.bank
    seen.clear()
    Rn.AudioEngine(16000, device="cuda", rir_slots=6, rir_spectral=False)
    assert "rows" not in seen                                                          # every other engine: the store as it was
