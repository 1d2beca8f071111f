"""Spectral length buckets (include/ss_hip.h ``ss_spec_bucket``): every refusal of the three entry points is SS_EINVAL (-1) from
the argument checks, before a device is touched (this file runs without a GPU: a call that got past the checks would come back
with a HIP error, not -1), the entries that refused buckets before keep their answers, and the Python layers raise ValueError
before they allocate anything - with and without the opt-in keyword."""
import ctypes

import pytest

from ss_amd import _lib, ops, planning as P

KB = P.KB
ONE = 16                            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
TWO = 4096
ODD8 = 24                           # 8-byte but not 16-byte aligned
ODD = 20                            # not 8-byte aligned
NULL = None
P1 = ctypes.c_void_p(ONE)
XF = ops.FLAG_CROSSFADE
CAPS = (16000, 20000, 40000, 70000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _bk(*rows):
    """ss_spec_bucket array from (hspec, hscale, first, n_entries, cap) rows"""
    arr = (_lib.SsSpecBucket * max(1, len(rows)))()
    for b, (hspec, hscale, first, n, cap) in enumerate(rows):
        arr[b].hspec, arr[b].hscale, arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = hspec, hscale, first, n, cap, 0
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _good(half, n=4):
    return [(ONE + 64 * b, (TWO + 64 * b) if half else NULL, 3 * b, 3, CAPS[b]) for b in range(n)]


def _bad_bucket_sets(half):
    """(label, rows) of every bucket array the checks refuse"""
    g = _good(half)
    sc = TWO if half else NULL

    def with_(b, **kw):
        rows = [list(r) for r in g]
        for k, v in kw.items():
            rows[b][("hspec", "hscale", "first", "n", "cap").index(k)] = v
        return [tuple(r) for r in rows]

    out = [("null hspec", with_(2, hspec=NULL)),
           ("misaligned hspec", with_(1, hspec=ODD)),
           ("mixed forms", with_(3, hscale=NULL if half else TWO)),
           ("five buckets", g + [(ONE, sc, 12, 3, 80000)]),
           ("first descending", with_(2, first=2)),
           ("overlapping ranges", with_(1, first=2)),
           ("bucket 0 does not start at 0", [(ONE, sc, 1, 3, 16000)]),
           ("odd cap", with_(1, cap=20001)),
           ("cap < 2", with_(0, cap=0)),
           ("negative count", with_(0, n=-1)),
           ("17 blocks", with_(3, cap=16 * KB + 2))]
    if not half:
        out.append(("fp32 spectra not 16-byte aligned", with_(1, hspec=ODD8)))
    return out


def test_declared_and_exported(lib):
    for name in ("ss_fftconv_binaural_spec_buckets_f32", "ss_audio_obs_spec_buckets_f32", "ss_ctx_set_rir_spec_buckets"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.SsSpecBucket) == 2 * ctypes.sizeof(ctypes.c_void_p) + 16
    assert hasattr(ops, "spec_bucket_array") and hasattr(ops, "fftconv_binaural_spec_buckets_into")
    assert hasattr(ops, "audio_obs_spec_buckets_into")


@pytest.mark.parametrize("half", [False, True], ids=["only", "half"])
def test_conv_entry_refusals(lib, half):
    f = lib.ss_fftconv_binaural_spec_buckets_f32
    ok, _k = _bk(*_good(half))
    #        spec buckets n_b rir_len desc out n  n_valid out_len flags stream
    assert f(P1, ok, 4, P1, P1, P1, 0, 16000, 16000, 0, NULL) == 0                     # no units: nothing to do
    assert f(P1, NULL, 4, P1, P1, P1, 0, 16000, 16000, 0, NULL) == 0
    for label, rows in _bad_bucket_sets(half):
        bad, _k2 = _bk(*rows)
        assert f(P1, bad, len(rows), P1, P1, P1, 2, 16000, 16000, 0, NULL) == -1, label
    assert f(P1, ok, 0, P1, P1, P1, 2, 16000, 16000, 0, NULL) == -1
    assert f(P1, NULL, 4, P1, P1, P1, 2, 16000, 16000, 0, NULL) == -1
    assert f(P1, ok, 4, P1, P1, P1, 2, 16000, 16000, XF, NULL) == -1                   # cross-fade
    assert f(P1, ok, 4, P1, P1, NULL, 2, 16000, 16000, 0, NULL) == -1                  # no output
    assert f(P1, ok, 4, P1, P1, P1, -1, 16000, 16000, 0, NULL) == -1
    assert f(NULL, ok, 4, P1, P1, P1, 2, 16000, 16000, 0, NULL) == -1                  # null window spectra
    assert f(P1, ok, 4, NULL, P1, P1, 2, 16000, 16000, 0, NULL) == -1                  # null lengths
    assert f(P1, ok, 4, P1, NULL, P1, 2, 16000, 16000, 0, NULL) == -1                  # null descriptors
    assert f(P1, ok, 4, P1, P1, P1, 2, 16001, 16000, 0, NULL) == -1                    # n_valid > out_len
    assert f(P1, ok, 4, P1, P1, P1, 2, 3 * KB + 1, 4 * KB, 0, NULL) == -1              # more than three output blocks


@pytest.mark.parametrize("half", [False, True], ids=["only", "half"])
def test_fused_entry_refusals(lib, half):
    f = lib.ss_audio_obs_spec_buckets_f32
    ok, _k = _bk(*_good(half))
    #        spec buckets n_b rir_len desc ag sgram n n_valid out_len pad flags stream
    assert f(P1, ok, 4, P1, P1, NULL, P1, 0, 16000, 16000, 0, 0, NULL) == 0
    for label, rows in _bad_bucket_sets(half):
        bad, _k2 = _bk(*rows)
        assert f(P1, bad, len(rows), P1, P1, NULL, P1, 2, 16000, 16000, 0, 0, NULL) == -1, label
    assert f(P1, ok, 4, P1, P1, NULL, P1, 2, 16000, 16000, 0, XF, NULL) == -1          # cross-fade
    assert f(P1, ok, 4, P1, P1, NULL, NULL, 2, 16000, 16000, 0, 0, NULL) == -1         # no spectrogram
    assert f(P1, ok, 4, P1, P1, NULL, P1, 2, 16000, 16000, 7, 0, NULL) == -1           # unknown pad mode
    assert f(P1, ok, 4, P1, P1, NULL, P1, 2, 256, 256, 0, 0, NULL) == -1               # shorter than the reflect padding
    assert f(P1, ok, 4, P1, P1, NULL, P1, 2, 16001, 16000, 0, 0, NULL) == -1
    assert f(NULL, ok, 4, P1, P1, NULL, P1, 2, 16000, 16000, 0, 0, NULL) == -1
    if half:                                                                          # half: rows of one partition block
        for out_len in (KB + 1, 44100, 48000):
            assert f(P1, ok, 4, P1, P1, P1, P1, 2, out_len, out_len, 0, 0, NULL) == -1
            assert f(P1, ok, 4, P1, P1, NULL, P1, 2, out_len, out_len, 0, 0, NULL) == -1


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


@pytest.mark.parametrize("half", [False, True], ids=["only", "half"])
def test_context_binding(lib, half):
    s = lib.ss_ctx_set_rir_spec_buckets
    ok, _k = _bk(*_good(half))
    h = _ctx(lib, 16000)
    try:
        for label, rows in _bad_bucket_sets(half):
            bad, _k2 = _bk(*rows)
            assert s(h, bad, len(rows), P1) == -1, label
        assert s(h, ok, 4, NULL) == -1                                                # no lengths
        assert s(h, NULL, 4, P1) == -1
        assert s(NULL, ok, 4, P1) == -1
        assert s(h, ok, 4, P1) == 0
        # one form at a time: nothing binds next to the spectral buckets ...
        assert lib.ss_ctx_set_rir_spectra16(h, P1, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra16_rows(h, P1, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra(h, NULL, 0) == 0                            # (unbinding nothing stays a no-op)
        assert s(h, ok, 4, P1) == 0                                                   # ... rebinding (a bucket was reallocated) is fine,
        assert lib.ss_ctx_set_rir_bank(h, NULL, P1, 0, 0, 1, 16000) == 0              # and a new bank replaces them
        assert lib.ss_ctx_set_rir_spectra16(h, P1, P1, 1) == 0
        assert s(h, ok, 4, P1) == 0                                                   # replaces any earlier binding (a half bank here)
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
    finally:
        lib.ss_ctx_destroy(h)
    for sr in (44100, 48000):                                                         # rows longer than one partition block
        h = _ctx(lib, sr)
        try:
            assert s(h, ok, 4, P1) == (-1 if half else 0)
        finally:
            lib.ss_ctx_destroy(h)


def test_old_entries_keep_their_answers(lib):
    """what refused length buckets (or rows-less buckets) before still does"""
    rb = (_lib.SsRirBucket * 2)()
    for b in range(2):
        rb[b].rir, rb[b].hspec, rb[b].first, rb[b].n_entries, rb[b].cap, rb[b].reserved = ONE, ONE, 3 * b, 3, CAPS[b], 0
    rbp = ctypes.cast(rb, ctypes.c_void_p)
    h = _ctx(lib, 16000)
    try:
        assert lib.ss_ctx_set_rir_buckets(h, rbp, 2, P1) == 0
        assert lib.ss_ctx_set_rir_spectra16(h, P1, P1, 2) == -1                       # a half bank on a bucketed context
        assert lib.ss_ctx_set_rir_spectra16_rows(h, P1, P1, 2) == -1
        rb[1].rir = NULL                                                              # buckets without rows are not ss_rir_bucket's
        assert lib.ss_ctx_set_rir_buckets(h, rbp, 2, P1) == -1
        rb[0].rir = NULL
        assert lib.ss_ctx_set_rir_buckets(h, rbp, 2, P1) == -1
        assert lib.ss_fftconv_binaural_buckets_f32(P1, rbp, 2, P1, P1, P1, 2, 16000, 16000, 0, NULL) == -1
        assert lib.ss_audio_obs_buckets_f32(P1, rbp, 2, P1, P1, NULL, P1, 2, 16000, 16000, 0, 0, NULL) == -1
    finally:
        lib.ss_ctx_destroy(h)
    # the single-allocation half entries take no bucket descriptors; their own refusals stand (tests/test_spec_half_args.py)
    assert lib.ss_fftconv_binaural_spec16_f32(P1, P1, NULL, P1, P1, P1, 2, 1, 16000, 16000, 0, NULL) == -1
    assert lib.ss_audio_obs_rows_spec16_f32(P1, P1, P1, P1, P1, NULL, P1, 2, 17, 44100, 44100, 0, 0, NULL) == -1


def test_store_and_engine_value_errors():
    from ss_amd.renderer import AudioEngine, BucketedRirStore
    bk = [(8, 16000), (4, 2 * KB)]
    for form in ("only", "half"):
        # without the keyword: refused as before
        with pytest.raises(ValueError, match="not supported with length buckets"):
            BucketedRirStore([8, 4], [16000, 2 * KB], "cpu", spectral=form)
        with pytest.raises(ValueError, match="length-bucketed"):
            AudioEngine(16000, device="cpu", rir_spectral=form, rir_buckets=bk)
        # with it: no CPU path; the SoundSpaces 2.0 and policy refusals stand
        with pytest.raises(ValueError, match="GPU"):
            BucketedRirStore([8, 4], [16000, 2 * KB], "cpu", spectral=form, spectral_buckets=True)
        with pytest.raises(ValueError, match="GPU"):
            AudioEngine(16000, device="cpu", rir_spectral=form, rir_buckets=bk, rir_spectral_buckets=True)
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(16000, device="cpu", rir_spectral=form, rir_buckets=bk, rir_spectral_buckets=True, step_time=0.25)
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(16000, device="cpu", rir_spectral=form, rir_buckets=bk, rir_spectral_buckets=True, wrap=True)
        with pytest.raises(ValueError, match="spectral_max_units"):
            AudioEngine(16000, device="cpu", rir_spectral=form, rir_buckets=bk, rir_spectral_buckets=True, spectral_max_units=64)
        with pytest.raises(ValueError, match="rir_spectral_buckets goes with"):
            AudioEngine(16000, device="cpu", rir_spectral=form, rir_spectral_buckets=True)            # no buckets
        with pytest.raises(ValueError, match="16 partition blocks"):
            BucketedRirStore([8, 4], [16000, 2 * KB], "cuda", spectral=form, spectral_buckets=True, max_cap=16 * KB + 2)
    for sr in (44100, 48000):
        with pytest.raises(ValueError, match="fused row kernels do not read half bucketed banks yet"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True)
        with pytest.raises(ValueError, match="fused row kernels do not read half bucketed banks yet"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_rows=True)
        with pytest.raises(ValueError, match="GPU"):                     # "only" at these rates is served: only the device is wrong
            AudioEngine(sr, device="cpu", rir_spectral="only", rir_buckets=bk, rir_spectral_buckets=True)
    for spectral in (None, False, True):
        with pytest.raises(ValueError, match="rir_spectral_buckets goes with"):
            AudioEngine(16000, device="cpu", rir_spectral=spectral, rir_buckets=bk, rir_spectral_buckets=True)
    with pytest.raises(ValueError, match="spectral_buckets goes with"):
        BucketedRirStore([8, 4], [16000, 2 * KB], "cpu", spectral=True, spectral_buckets=True)



@pytest.mark.parametrize("half", [False, True], ids=["only", "half"])
def test_context_plans_like_a_bucketed_context(lib, half):
    """the planner alone (host only): planning depth = the longest bucket's blocks, SS_FLAG_FIRST_BUCKET for steps inside bucket 0,
    descriptors and new windows equal to those of a context bound with ss_ctx_set_rir_buckets over the same ranges"""
    import numpy as np
    from ss_amd.context import AudioContext
    ok, _k = _bk(*_good(half))
    rb = (_lib.SsRirBucket * 4)()
    for b in range(4):
        rb[b].rir, rb[b].hspec, rb[b].first, rb[b].n_entries, rb[b].cap, rb[b].reserved = ONE, NULL, 3 * b, 3, CAPS[b], 0
    plans = []
    for which in ("spec", "rows"):
        ctx = AudioContext(16000)
        try:
            ctx.add_source_len("a", 16000)
            ctx.add_source_len("b", 48000)
            if which == "spec":
                assert lib.ss_ctx_set_rir_spec_buckets(ctx._h, ok, 4, P1) == 0
            else:
                assert lib.ss_ctx_set_rir_buckets(ctx._h, ctypes.cast(rb, ctypes.c_void_p), 4, P1) == 0
            assert ctx.stats()["slots_per_key"] == 5                       # 5 blocks in the longest bucket, one output block
            inside = ctx.plan(np.asarray([0, 1, 0], np.int32), np.asarray([0, 16000, 0], np.int32), np.asarray([0, 2, -1], np.int32))
            across = ctx.plan(np.asarray([0, 1, 0], np.int32), np.asarray([0, 16000, 0], np.int32), np.asarray([0, 9, 3], np.int32),
                              dis_sound=np.asarray([0, 0, 0], np.int32), dis_rir=np.asarray([-1, 4, -1], np.int32))
            assert inside[1] == ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET and across[1] == 0
            plans.append((inside, across))
        finally:
            ctx.close()
    for a, b in zip(plans[0], plans[1]):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("form", ["only", "half"])
def test_engine_hands_the_form_to_the_bucketed_store(monkeypatch, form):
    """the constructor's plumbing, without a device: the store is built with the form's name (not its truth value) and the keyword"""
    import types
    from ss_amd import renderer as Rn
    seen = {}

    class Store:
        def __init__(self, slots, caps, device, **kw):
            seen.update(kw, slots=list(slots), caps=list(caps))
            self.bank = types.SimpleNamespace(cap=max(caps))

    class Renderer:
        def __init__(self, sr, device="cuda", **kw):
            self.sr = self.n_valid = self.out_len = int(sr)
            self.wrap, self.device = False, "cuda"

        def set_rir_bank(self, bank):
            self.rirs = bank

    monkeypatch.setattr(Rn, "BucketedRirStore", Store)
    monkeypatch.setattr(Rn, "BatchedAudioRenderer", Renderer)
    eng = Rn.AudioEngine(16000, device="cuda", rir_buckets=[(3, 16000), (2, 40000)], rir_spectral=form, rir_spectral_buckets=True)
    assert seen["spectral"] == form and seen["spectral_buckets"] is True and seen["slots"] == [3, 2] and seen["caps"] == [16000, 40000]
    assert eng.rir_spectral_only and eng.rir_spectral_half == (form == "half") and eng.renderer.rirs is eng.store.bank
    assert seen["max_cap"] == 1 << 18                                   # the default: 16 blocks, handed on as it is
    seen.clear()                                                        # a larger rir_max_cap is clamped to 16 blocks per row
    Rn.AudioEngine(16000, device="cuda", rir_buckets=[(3, 16000), (2, 40000)], rir_spectral=form, rir_spectral_buckets=True,
                   rir_max_cap=1 << 19)
    assert seen["max_cap"] == 16 * KB
    seen.clear()
    Rn.AudioEngine(16000, device="cuda", rir_buckets=[(3, 16000), (2, 40000)], rir_spectral=True, rir_max_cap=1 << 19)
    assert seen["spectral"] is True and "spectral_buckets" not in seen and seen["max_cap"] == 1 << 19      # the both-forms store: as before


@pytest.mark.parametrize("half", [False, True], ids=["only", "half"])
def test_in_call_file_loader_is_not_served_on_a_spectral_bucket_context(lib, half):
    """ss_ctx_load_rir_files with the ss_miss_loader of a spectral-only store (bank = NULL): 1 = not served, nothing changed - the
    answer it gives on a context bound by ss_ctx_set_rir_buckets too (whose rows are not the loader's bank)"""
    ok, _k = _bk(*_good(half))
    rb = (_lib.SsRirBucket * 2)()
    for b in range(2):
        rb[b].rir, rb[b].hspec, rb[b].first, rb[b].n_entries, rb[b].cap, rb[b].reserved = ONE, NULL, 3 * b, 3, CAPS[b], 0
    ld = _lib.SsMissLoader()
    for name, ctype in _lib.SsMissLoader._fields_:
        if ctype is ctypes.c_void_p and name != "bank":
            setattr(ld, name, ONE)                                      # lent, never dereferenced on this path
    ld.cap, ld.n_free, ld.stage_rows, ld.loaded_cap, ld.n_loaded, ld.n_evicted = 16000, 2, 4, 4, 7, 7
    paths = (ctypes.c_char_p * 1)(b"/nonexistent/0_0.wav")
    for which in ("spec", "rows"):
        h = _ctx(lib, 16000)
        try:
            if which == "spec":
                assert lib.ss_ctx_set_rir_spec_buckets(h, ok, 4, P1) == 0
            else:
                assert lib.ss_ctx_set_rir_buckets(h, ctypes.cast(rb, ctypes.c_void_p), 2, P1) == 0
            ld.n_loaded = ld.n_evicted = 7
            assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 6, NULL) == 1
            assert ld.n_loaded == 0 and ld.n_evicted == 0 and ld.n_free == 2
        finally:
            lib.ss_ctx_destroy(h)
