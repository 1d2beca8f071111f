"""Half-precision time-domain RIR rows under the fused 44.1 / 48 kHz row kernels (include/ss_hip.h "Half-precision time-domain
rows": ``ss_audio_obs_rows_rir16_f32``, ``ss_ctx_set_rir_bank16_rows``): every refusal is SS_EINVAL (-1) from the argument checks,
before a device is touched (this file runs without a GPU: a call that got past the checks would come back with a HIP error, not
-1); n_units == 0 returns 0; the binding replaces and is replaced exactly as ss_ctx_set_rir_bank16; and
``AudioEngine(rir_rows16_fused=True)`` without ``rir_rows="half"`` is a ValueError before anything is allocated."""
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
    for name in ("ss_audio_obs_rows_rir16_f32", "ss_ctx_set_rir_bank16_rows"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert hasattr(ops, "audio_obs_rows_rir16_into")
    import inspect
    from ss_amd.context import AudioContext
    from ss_amd.renderer import AudioEngine
    assert inspect.signature(AudioContext.set_rir_bank16).parameters["rows"].default is False
    assert inspect.signature(AudioEngine.__init__).parameters["rir_rows16_fused"].default is False      # no default changes


def test_audio_obs_rows_rir16_refusals(lib):
    f = lib.ss_audio_obs_rows_rir16_f32

    def call(spec=P1, rir16=P1, rscale=P1, lens=P1, desc=P1, ag=NULL, sg=P1, n=2, cap=44100, n_valid=44100, out_len=44100, pad=0,
             flags=0):
        return f(spec, rir16, rscale, lens, desc, ag, sg, n, cap, n_valid, out_len, pad, flags, NULL)

    assert call(n=0) == 0 and call(n=0, rir16=NULL, rscale=NULL, sg=NULL, cap=0) == 0      # no units: nothing to do
    for ag in (NULL, P1):                                                              # `audiogoal` is optional, everything else is not
        assert call(ag=ag, rir16=NULL) == -1 and call(ag=ag, rscale=NULL) == -1 and call(ag=ag, rir16=ODD2) == -1
        for cap in BAD_CAPS:                                                           # rows16_bank_ok: odd, < 2, more than 16 RIR blocks
            assert call(ag=ag, cap=cap) == -1, cap
        assert call(ag=ag, flags=XF) == -1 and call(ag=ag, flags=XF | ops.FLAG_NO_DISTRACTOR) == -1
        assert call(ag=ag, sg=NULL) == -1                                              # the required output
        assert call(ag=ag, pad=7) == -1 and call(ag=ag, pad=-1) == -1
        assert call(ag=ag, spec=NULL) == -1 and call(ag=ag, lens=NULL) == -1 and call(ag=ag, desc=NULL) == -1
        assert call(ag=ag, n=-1) == -1
        assert call(ag=ag, n_valid=44101) == -1 and call(ag=ag, n_valid=-1) == -1
        for out_len in (1, 256, 257, 16000, KB, 3 * KB + 1, 4 * KB):                   # outside (kB, 3 kB]
            assert call(ag=ag, out_len=out_len, n_valid=out_len) == -1, out_len
        for sr in (48000, KB + 1, 3 * KB):                                             # (the same at the other rates inside it)
            assert call(ag=ag, out_len=sr, n_valid=sr, flags=XF) == -1
            assert call(ag=ag, out_len=sr, n_valid=sr, sg=NULL) == -1
            assert call(ag=ag, out_len=sr, n_valid=sr, pad=3) == -1


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


@pytest.mark.parametrize("sr", [16000, KB, 44100, 48000])
def test_context_binding(lib, sr):
    """the refusals and the replace / unbind rules of ss_ctx_set_rir_bank16, at one-block rates too (inert there)"""
    s, plain = lib.ss_ctx_set_rir_bank16_rows, lib.ss_ctx_set_rir_bank16
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
        assert plain(h, P1, P1, P1, 16000) == 0 and s(h, P1, P1, P1, 16000) == 0       # the two bindings replace each other
        assert plain(h, NULL, NULL, NULL, 0) == 0                                      # either call's NULL unbinds
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == 0
        assert s(h, P1, P1, P1, 16000) == 0 and s(h, NULL, NULL, NULL, 0) == 0
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_context_plans_at_the_half_banks_depth(lib):
    """the planner alone (host only): the binding plans as ss_ctx_set_rir_bank16 does"""
    from ss_amd.context import AudioContext
    ctx = AudioContext(44100)
    try:
        ctx.add_source_len("a", 44100)
        assert lib.ss_ctx_set_rir_bank16_rows(ctx._h, P1, P1, P1, 40000) == 0
        assert ctx.stats()["slots_per_key"] == 3 + 3 - 1
        plan = ctx.plan(np.asarray([0, 0], np.int32), np.asarray([0, 0], np.int32), np.asarray([0, 2], np.int32))
        assert plan[1] == ops.FLAG_NO_DISTRACTOR
    finally:
        ctx.close()


def test_in_call_file_loader_answers_not_served(lib):
    """ss_ctx_load_rir_files on a context bound by ss_ctx_set_rir_bank16_rows: 1 (not served), as on the plain binding"""
    h = _ctx(lib, 44100)
    try:
        assert lib.ss_ctx_set_rir_bank16_rows(h, P1, P1, P1, 44100) == 0
        ld = _lib.SsMissLoader()
        paths = (ctypes.c_char_p * 1)(b"/nonexistent.wav")
        assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 4, NULL) == 1
        assert ld.n_loaded == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_engine_value_errors():
    from ss_amd.renderer import AudioEngine
    for sr in (16000, 44100, 48000):
        with pytest.raises(ValueError, match="rir_rows16_fused goes with rir_rows='half'"):
            AudioEngine(sr, device="cpu", rir_rows16_fused=True)
        for spectral in (True, "only", "half"):
            with pytest.raises(ValueError, match="rir_rows16_fused goes with rir_rows='half'"):
                AudioEngine(sr, device="cpu", rir_rows16_fused=True, rir_spectral=spectral)
        with pytest.raises(ValueError, match="GPU"):                                   # with the form: every refusal of the form stands
            AudioEngine(sr, device="cpu", rir_rows="half", rir_rows16_fused=True)
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(sr, device="cpu", rir_rows="half", rir_rows16_fused=True, step_time=0.25)
    with pytest.raises(ValueError, match="three partition blocks"):
        AudioEngine(96000, device="cuda", rir_rows="half", rir_rows16_fused=True)


def test_engine_hands_the_opt_in_to_renderer_and_context(monkeypatch):
    """the constructor's plumbing, without a device: accepted at every rate (inert at one-block rates), off by default"""
    import types
    from ss_amd import renderer as Rn
    seen = {}

    class Store:
        def __init__(self, slots, cap, device, **kw):
            seen.update(kw, slots=slots, cap=cap)
            self.bank = types.SimpleNamespace(cap=cap)

    class Renderer:
        rows16_fused = False

        def __init__(self, sr, device="cuda", **kw):
            self.sr = self.n_valid = self.out_len = int(sr)
            self.wrap, self.device = False, "cuda"

        def set_rir_bank(self, bank):
            self.rirs = bank

    monkeypatch.setattr(Rn, "RirStore", Store)
    monkeypatch.setattr(Rn, "BatchedAudioRenderer", Renderer)
    for sr in (16000, 44100, 48000):
        eng = Rn.AudioEngine(sr, device="cuda", rir_slots=6, rir_rows="half", rir_rows16_fused=True)
        assert seen["rows"] == "half" and eng.rir_rows_half and eng.rir_rows16_fused and eng.renderer.rows16_fused is True
        eng = Rn.AudioEngine(sr, device="cuda", rir_slots=6, rir_rows="half")
        assert eng.rir_rows_half and not eng.rir_rows16_fused and eng.renderer.rows16_fused is False
    assert Rn.BatchedAudioRenderer.rows16_fused is False
