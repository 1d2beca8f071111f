"""Half-precision time-domain rows in length buckets (include/ss_hip.h "Half-precision time-domain rows in length buckets":
``ss_fftconv_binaural_rir16_buckets_f32``, ``ss_audio_obs_rir16_buckets_f32``, ``ss_ctx_set_rir16_buckets``): every refusal is
SS_EINVAL (-1) from the argument checks, before a device is touched (this file runs without a GPU: a call that got past the checks
would come back with a HIP error, not -1); n_units == 0 returns 0; the binding replaces and is replaced as every other bank call;
the in-call file loader answers "not served"; ``AudioEngine(rir_rows="half", rir_buckets=[...])`` is accepted and keeps every
other refusal of the form; no default changed."""
import ctypes
import inspect

import numpy as np
import pytest

from ss_amd import _lib, ops, planning as P

KB = P.KB
NULL = None
P1 = ctypes.c_void_p(16)            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
ONE, ODD2, AL4 = 16, 18, 20         # 16-byte, 2-byte and 4-byte aligned dummy addresses
XF = ops.FLAG_CROSSFADE
BAD_CAPS = (0, 1, 15999, -2, 16 * KB + 2)       # < 2, odd, negative, more than 16 partition blocks


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _buckets(*rows):
    """rows: (rir16, rscale, first, n_entries, cap) -> (ss_rir16_bucket array as a void pointer, n)"""
    arr = (_lib.SsRir16Bucket * max(1, len(rows)))()
    for b, (q, s, first, n, cap) in enumerate(rows):
        arr[b].rir16, arr[b].rscale, arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = q, s, first, n, cap, 0
    return ctypes.cast(arr, ctypes.c_void_p), len(rows), arr


GOOD = ((ONE, ONE, 0, 3, 16000), (AL4, ONE, 3, 2, 20000), (ONE, ONE, 5, 3, 40000), (ONE, ONE, 8, 2, 70000))


def _bad_arrays():
    """(label, rows) of every bucket array the checks refuse"""
    out = [("null halves", ((None, ONE, 0, 3, 16000),)), ("2-byte aligned halves", ((ODD2, ONE, 0, 3, 16000),)),
           ("null scales", ((ONE, None, 0, 3, 16000),)), ("null halves in bucket 2", GOOD[:2] + ((None, ONE, 5, 3, 40000),)),
           ("misaligned halves in bucket 1", GOOD[:1] + ((ODD2, ONE, 3, 2, 20000),)),
           ("null scales in bucket 3", GOOD[:3] + ((ONE, None, 8, 2, 70000),)),
           ("unordered", (GOOD[0], GOOD[2], GOOD[1])), ("overlapping", (GOOD[0], (ONE, ONE, 2, 2, 20000))),
           ("bucket 0 not at 0", ((ONE, ONE, 1, 3, 16000),)), ("negative entries", ((ONE, ONE, 0, -1, 16000),)),
           ("negative first", ((ONE, ONE, 0, 3, 16000), (ONE, ONE, -4, 1, 20000))),
           ("five buckets", GOOD + ((ONE, ONE, 10, 1, 80000),))]
    for cap in BAD_CAPS:
        out.append((f"cap {cap}", ((ONE, ONE, 0, 3, cap),)))
        out.append((f"cap {cap} in bucket 1", (GOOD[0], (ONE, ONE, 3, 2, cap))))
    return out


def test_declared_and_exported(lib):
    for name in ("ss_fftconv_binaural_rir16_buckets_f32", "ss_audio_obs_rir16_buckets_f32", "ss_ctx_set_rir16_buckets"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.SsRir16Bucket) == ctypes.sizeof(_lib.SsRirBucket) == 32
    assert hasattr(ops, "fftconv_binaural_rir16_buckets_into") and hasattr(ops, "audio_obs_rir16_buckets_into")
    assert hasattr(ops, "rir16_bucket_array")
    from ss_amd.context import AudioContext
    from ss_amd.renderer import AudioEngine, BucketedRirBank, BucketedRirStore
    assert hasattr(AudioContext, "set_rir16_buckets") and hasattr(BucketedRirBank, "rir16_c_array")
    # no default changed
    assert inspect.signature(BucketedRirStore.__init__).parameters["rows"].default is None
    sig = inspect.signature(AudioEngine.__init__).parameters
    assert sig["rir_rows"].default is None and sig["rir_buckets"].default is None and sig["rir_rows16_fused"].default is False
    assert sig["rir_max_cap"].default == 1 << 18


def test_fftconv_binaural_rir16_buckets_refusals(lib):
    f = lib.ss_fftconv_binaural_rir16_buckets_f32

    def call(rows=GOOD, spec=P1, lens=P1, desc=P1, out=P1, n=2, n_valid=16000, out_len=16000, flags=0, n_buckets=None, null=False):
        ptr, nb, keep = _buckets(*rows)
        return f(spec, NULL if null else ptr, nb if n_buckets is None else n_buckets, lens, desc, out, n, n_valid, out_len, flags, NULL)

    assert call(n=0) == 0 and call(n=0, null=True, n_buckets=0, out=NULL) == 0           # no units: nothing to do
    for label, rows in _bad_arrays():
        assert call(rows=rows) == -1, label
    assert call(null=True) == -1 and call(n_buckets=0) == -1 and call(n_buckets=5) == -1
    assert call(flags=XF) == -1 and call(flags=XF | ops.FLAG_NO_DISTRACTOR) == -1
    assert call(out=NULL) == -1 and call(lens=NULL) == -1 and call(spec=NULL) == -1 and call(desc=NULL) == -1
    assert call(n=-1) == -1
    for out_len, n_valid in ((16000, 16001), (16000, -1), (44100, 3 * KB + 1), (4 * KB, 4 * KB)):
        assert call(out_len=out_len, n_valid=n_valid) == -1, (out_len, n_valid)


def test_audio_obs_rir16_buckets_refusals(lib):
    f = lib.ss_audio_obs_rir16_buckets_f32

    def call(rows=GOOD, spec=P1, lens=P1, desc=P1, ag=NULL, sg=P1, n=2, n_valid=16000, out_len=16000, pad=0, flags=0, n_buckets=None,
             null=False):
        ptr, nb, keep = _buckets(*rows)
        return f(spec, NULL if null else ptr, nb if n_buckets is None else n_buckets, lens, desc, ag, sg, n, n_valid, out_len, pad,
                 flags, NULL)

    assert call(n=0) == 0 and call(n=0, null=True, n_buckets=0, sg=NULL) == 0
    for ag in (NULL, P1):                                                              # `audiogoal` is optional, everything else is not
        for label, rows in _bad_arrays():
            assert call(ag=ag, rows=rows) == -1, label
        assert call(ag=ag, null=True) == -1 and call(ag=ag, n_buckets=0) == -1 and call(ag=ag, n_buckets=5) == -1
        assert call(ag=ag, flags=XF) == -1 and call(ag=ag, flags=XF | ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET) == -1
        assert call(ag=ag, sg=NULL) == -1                                              # the required output
        assert call(ag=ag, pad=7) == -1 and call(ag=ag, pad=-1) == -1
        assert call(ag=ag, spec=NULL) == -1 and call(ag=ag, lens=NULL) == -1 and call(ag=ag, desc=NULL) == -1
        assert call(ag=ag, n=-1) == -1
        assert call(ag=ag, n_valid=16001) == -1 and call(ag=ag, n_valid=-1) == -1
        for out_len in (1, 256, KB + 1, 16640, 44100, 48000):                          # outside [257, kB] / more than 26 pooled blocks
            assert call(ag=ag, out_len=out_len, n_valid=min(out_len, KB)) == -1, out_len


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


@pytest.mark.parametrize("sr", [16000, 44100])
def test_context_binding(lib, sr):
    s = lib.ss_ctx_set_rir16_buckets
    good, n_good, keep = _buckets(*GOOD)
    one, n_one, keep1 = _buckets(GOOD[0])
    h = _ctx(lib, sr)
    try:
        assert s(NULL, good, n_good, P1) == -1
        assert s(h, good, n_good, NULL) == -1                                          # no lengths
        assert s(h, good, 0, P1) == -1 and s(h, good, 5, P1) == -1
        for label, rows in _bad_arrays():
            ptr, nb, k = _buckets(*rows)
            assert s(h, ptr, nb, P1) == -1, label
        assert s(h, NULL, 0, NULL) == 0                                                # unbinding nothing is fine
        assert s(h, good, n_good, P1) == 0 and s(h, one, n_one, P1) == 0 and s(h, good, n_good, P1) == 0
        # one form at a time: no spectra next to the half rows ...
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra16(h, P1, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra16_rows(h, P1, P1, 5) == -1
        # ... and every other bank call replaces them: the spectral bindings work again
        assert lib.ss_ctx_set_rir_bank(h, NULL, P1, 0, 0, 1, 16000) == 0
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == 0
        assert s(h, good, n_good, P1) == 0                                             # replaces any earlier binding (fp32 spectra here)
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
        assert lib.ss_ctx_set_rir_bank16(h, P1, P1, P1, 16000) == 0 and s(h, good, n_good, P1) == 0     # half rows of either kind
        rb = (_lib.SsRirBucket * 1)()
        rb[0].rir, rb[0].hspec, rb[0].first, rb[0].n_entries, rb[0].cap = ONE, None, 0, 3, 16000
        assert lib.ss_ctx_set_rir_buckets(h, ctypes.cast(rb, ctypes.c_void_p), 1, P1) == 0              # fp32 length buckets replace them
        assert lib.ss_ctx_set_rir_spectra(h, P1, 1) == 0
        assert s(h, good, n_good, P1) == 0 and s(h, NULL, 0, NULL) == 0                # NULL unbinds
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_context_plans_at_the_deepest_bucket_and_flags_the_first_bucket(lib):
    """the planner alone (host only): depth = the deepest bucket's blocks; SS_FLAG_FIRST_BUCKET when every index sits in bucket 0"""
    from ss_amd.context import AudioContext
    ctx = AudioContext(16000)
    try:
        ctx.add_source_len("a", 16000)
        good, n_good, keep = _buckets(*GOOD)
        assert lib.ss_ctx_set_rir16_buckets(ctx._h, good, n_good, P1) == 0
        assert ctx.stats()["slots_per_key"] == 5 + 1 - 1                               # 70 000 samples: five partition blocks
        zeros = np.asarray([0, 0], np.int32)
        plan = ctx.plan(zeros, zeros, np.asarray([0, 2], np.int32))
        assert plan[1] == ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET
        plan = ctx.plan(zeros, zeros, np.asarray([0, 3], np.int32))
        assert plan[1] == ops.FLAG_NO_DISTRACTOR
    finally:
        ctx.close()


def test_in_call_file_loader_answers_not_served(lib):
    h = _ctx(lib, 16000)
    try:
        good, n_good, keep = _buckets(*GOOD)
        assert lib.ss_ctx_set_rir16_buckets(h, good, n_good, P1) == 0
        ld = _lib.SsMissLoader()
        paths = (ctypes.c_char_p * 1)(b"/nonexistent.wav")
        assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 4, NULL) == 1
        assert ld.n_loaded == 0
    finally:
        lib.ss_ctx_destroy(h)


BUCKETS = [(3, 16000), (2, 40000)]


def test_store_and_engine_value_errors():
    from ss_amd.renderer import AudioEngine, BucketedRirStore
    with pytest.raises(ValueError, match="rows must be None or 'half'"):
        BucketedRirStore([3, 2], [16000, 40000], "cpu", rows="quarter")
    with pytest.raises(ValueError, match="GPU"):
        BucketedRirStore([3, 2], [16000, 40000], "cpu", rows="half")
    with pytest.raises(ValueError, match="does not go with spectral"):
        BucketedRirStore([3, 2], [16000, 40000], "cuda", rows="half", spectral=True)
    with pytest.raises(ValueError, match="does not go with spectral"):
        BucketedRirStore([3, 2], [16000, 40000], "cuda", rows="half", spectral="half", spectral_buckets=True)
    with pytest.raises(ValueError, match="16 partition blocks"):
        BucketedRirStore([3, 2], [16000, 40000], "cuda", rows="half", max_cap=16 * KB + 2)
    for sr in (16000, 44100, 48000):
        for spectral in (True, "only", "half"):
            with pytest.raises(ValueError, match="does not go with rir_spectral"):
                AudioEngine(sr, device="cuda", rir_rows="half", rir_buckets=BUCKETS, rir_spectral=spectral)
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(sr, device="cuda", rir_rows="half", rir_buckets=BUCKETS, step_time=0.25)
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(sr, device="cuda", rir_rows="half", rir_buckets=BUCKETS, wrap=True)
        with pytest.raises(ValueError, match="fused row kernels do not read bucketed half rows"):
            AudioEngine(sr, device="cuda", rir_rows="half", rir_buckets=BUCKETS, rir_rows16_fused=True)
        with pytest.raises(ValueError, match="GPU"):                                   # the combination itself: only the device is missing
            AudioEngine(sr, device="cpu", rir_rows="half", rir_buckets=BUCKETS)
    with pytest.raises(ValueError, match="three partition blocks"):
        AudioEngine(96000, device="cuda", rir_rows="half", rir_buckets=BUCKETS)


def test_engine_hands_the_form_to_the_bucketed_store(monkeypatch):
    """the constructor's plumbing, without a device: the combination that used to raise builds a BucketedRirStore(rows="half")
    with rir_max_cap clamped to 16 partition blocks"""
    import types
    from ss_amd import renderer as Rn
    seen = {}

    class Store:
        def __init__(self, slots, caps, device, **kw):
            seen.update(kw, slots=list(slots), caps=list(caps))
            self.bank = types.SimpleNamespace(cap=max(caps))

    class Renderer:
        rows16_fused = False

        def __init__(self, sr, device="cuda", **kw):
            self.sr = self.n_valid = self.out_len = int(sr)
            self.wrap, self.device = False, "cuda"

        def set_rir_bank(self, bank):
            self.rirs = bank

    monkeypatch.setattr(Rn, "BucketedRirStore", Store)
    monkeypatch.setattr(Rn, "BatchedAudioRenderer", Renderer)
    for sr in (16000, 44100, 48000):
        seen.clear()
        eng = Rn.AudioEngine(sr, device="cuda", rir_rows="half", rir_buckets=BUCKETS)
        assert seen["rows"] == "half" and seen["spectral"] is False and "spectral_buckets" not in seen
        assert seen["slots"] == [3, 2] and seen["caps"] == [16000, 40000] and seen["max_cap"] == 16 * KB
        assert eng.rir_rows_half and not eng.rir_spectral and eng.renderer.rirs is eng.store.bank
        seen.clear()
        Rn.AudioEngine(sr, device="cuda", rir_rows="half", rir_buckets=BUCKETS, rir_max_cap=50000)
        assert seen["max_cap"] == 50000
    seen.clear()
    Rn.AudioEngine(16000, device="cuda", rir_buckets=BUCKETS, rir_spectral=False)
    assert "rows" not in seen and seen["max_cap"] == 1 << 18                          # every other engine: the store as it was
