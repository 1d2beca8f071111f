"""Half spectral length buckets under rows of 2 or 3 partition blocks (include/ss_hip.h ``ss_audio_obs_rows_spec16_buckets_f32``,
``ss_audio_obs_logmel_rows_spec16_buckets_f32``, ``ss_ctx_set_rir_spec_buckets_rows``): every refusal is SS_EINVAL (-1) from the
argument checks, before a device is touched (this file runs without a GPU: a call that got past the checks would come back with a
HIP error, not -1); the binding is accepted on 44.1 / 48 kHz contexts and refused on 16 kHz ones; and the engine raises
ValueError before it allocates anything - with and without the opt-in keyword."""
import ctypes

import pytest

from ss_amd import _lib, ops, planning as P

KB = P.KB
ONE = 16                            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
TWO = 4096
ODD = 20                            # not 8-byte aligned
NULL = None
P1 = ctypes.c_void_p(ONE)
XF = ops.FLAG_CROSSFADE
CAPS = (16384, 49152, 81920)
SRS = (44100, 48000, 22050)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _bk(*rows):
    """ss_spec_bucket array from (hspec, hscale, first, n_entries, cap) rows"""
    arr = (_lib.SsSpecBucket * max(1, len(rows)))()
    for b, (hspec, hscale, first, n, cap) in enumerate(rows):
        arr[b].hspec, arr[b].hscale, arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = hspec, hscale, first, n, cap, 0
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _good(half=True, n=3):
    return [(ONE + 64 * b, (TWO + 64 * b) if half else NULL, 3 * b, 3, CAPS[b]) for b in range(n)]


def _bad_bucket_sets():
    """(label, rows) of every bucket array the checks refuse: spec_buckets_check's refusals, and anything but the half form"""
    g = _good()

    def with_(b, **kw):
        rows = [list(r) for r in g]
        for k, v in kw.items():
            rows[b][("hspec", "hscale", "first", "n", "cap").index(k)] = v
        return [tuple(r) for r in rows]

    return [("fp32 buckets", _good(half=False)),
            ("mixed forms", with_(2, hscale=NULL)),
            ("mixed forms, bucket 0 fp32", with_(0, hscale=NULL)),
            ("null hspec", with_(2, hspec=NULL)),
            ("misaligned hspec", with_(1, hspec=ODD)),
            ("five buckets", g + [(ONE, TWO, 9, 3, 90000), (ONE, TWO, 12, 3, 100000)]),
            ("first descending", with_(2, first=2)),
            ("overlapping ranges", with_(1, first=2)),
            ("bucket 0 does not start at 0", [(ONE, TWO, 1, 3, 16384)]),
            ("odd cap", with_(1, cap=20001)),
            ("cap < 2", with_(0, cap=0)),
            ("negative count", with_(0, n=-1)),
            ("17 blocks", with_(2, cap=16 * KB + 2))]


def test_declared_and_exported(lib):
    for name in ("ss_audio_obs_rows_spec16_buckets_f32", "ss_audio_obs_logmel_rows_spec16_buckets_f32", "ss_ctx_set_rir_spec_buckets_rows"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert hasattr(ops, "audio_obs_rows_spec16_buckets_into") and hasattr(ops, "audio_obs_logmel_rows_spec16_buckets_into")


def test_obs_entry_refusals(lib):
    f = lib.ss_audio_obs_rows_spec16_buckets_f32
    ok, _k = _bk(*_good())
    #        spec buckets n_b rir_len desc ag sgram n n_valid out_len pad flags stream
    assert f(P1, ok, 3, P1, P1, NULL, P1, 0, 44100, 44100, 0, 0, NULL) == 0            # no units: nothing to do
    assert f(P1, NULL, 3, P1, P1, NULL, NULL, 0, 44100, 44100, 0, 0, NULL) == 0
    for sr in SRS:
        for label, rows in _bad_bucket_sets():
            bad, _k2 = _bk(*rows)
            assert f(P1, bad, len(rows), P1, P1, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1, label
        assert f(P1, ok, 0, P1, P1, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1
        assert f(P1, NULL, 3, P1, P1, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1
        assert f(P1, ok, 3, P1, P1, NULL, P1, 2, sr, sr, 0, XF, NULL) == -1            # cross-fade
        assert f(P1, ok, 3, P1, P1, P1, P1, 2, sr, sr, 0, XF, NULL) == -1
        assert f(P1, ok, 3, P1, P1, NULL, NULL, 2, sr, sr, 0, 0, NULL) == -1           # no spectrogram
        assert f(P1, ok, 3, P1, P1, P1, NULL, 2, sr, sr, 0, 0, NULL) == -1
        assert f(P1, ok, 3, P1, P1, NULL, P1, 2, sr, sr, 7, 0, NULL) == -1             # unknown pad mode
        assert f(P1, ok, 3, P1, P1, NULL, P1, 2, sr + 1, sr, 0, 0, NULL) == -1         # n_valid > out_len
        assert f(P1, ok, 3, P1, P1, NULL, P1, 2, -1, sr, 0, 0, NULL) == -1
        assert f(P1, ok, 3, P1, P1, NULL, P1, -1, sr, sr, 0, 0, NULL) == -1
        assert f(NULL, ok, 3, P1, P1, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1           # null window spectra
        assert f(P1, ok, 3, NULL, P1, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1           # null lengths
        assert f(P1, ok, 3, P1, NULL, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1           # null descriptors
    for out_len in (257, 16000, KB, 3 * KB + 1, 4 * KB):                              # rows of one block, or of more than three
        assert f(P1, ok, 3, P1, P1, NULL, P1, 2, min(out_len, 3 * KB), out_len, 0, 0, NULL) == -1, out_len
        assert f(P1, ok, 3, P1, P1, P1, P1, 2, min(out_len, 3 * KB), out_len, 0, 0, NULL) == -1, out_len


def test_logmel_entry_refusals(lib):
    f = lib.ss_audio_obs_logmel_rows_spec16_buckets_f32
    ok, _k = _bk(*_good())

    def call(spec=P1, bk=ok, nb=3, lens=P1, desc=P1, ag=NULL, sg=NULL, lm=P1, ms=P1, mw=P1, n_mels=64, max_len=32, eps=1e-6, n=2,
             n_valid=44100, out_len=44100, pad=0, flags=0):
        return f(spec, bk, nb, lens, desc, ag, sg, lm, ms, mw, n_mels, max_len, eps, n, n_valid, out_len, pad, flags, NULL)

    assert call(n=0) == 0 and call(n=0, bk=NULL, lm=NULL) == 0
    for sr in SRS:
        for label, rows in _bad_bucket_sets():
            bad, _k2 = _bk(*rows)
            assert call(bk=bad, nb=len(rows), n_valid=sr, out_len=sr) == -1, label
        for ag, sg in ((NULL, NULL), (P1, NULL), (NULL, P1), (P1, P1)):               # any combination of the optional outputs
            assert call(ag=ag, sg=sg, lm=NULL, n_valid=sr, out_len=sr) == -1           # ... but the log-mel output is required
            assert call(ag=ag, sg=sg, flags=XF, n_valid=sr, out_len=sr) == -1
            assert call(ag=ag, sg=sg, pad=7, n_valid=sr, out_len=sr) == -1
            assert call(ag=ag, sg=sg, n_valid=sr + 1, out_len=sr) == -1
            assert call(ag=ag, sg=sg, n_valid=-1, out_len=sr) == -1
        # the mel limits of ss_audio_features_f32
        assert call(ms=NULL, n_valid=sr, out_len=sr) == -1 and call(mw=NULL, n_valid=sr, out_len=sr) == -1
        assert call(n_mels=0, n_valid=sr, out_len=sr) == -1 and call(n_mels=65, n_valid=sr, out_len=sr) == -1
        assert call(max_len=0, n_valid=sr, out_len=sr) == -1 and call(max_len=30, n_valid=sr, out_len=sr) == -1
        assert call(max_len=68, n_valid=sr, out_len=sr) == -1
        assert call(eps=0.0, n_valid=sr, out_len=sr) == -1
        assert call(mw=ctypes.c_void_p(ODD), n_valid=sr, out_len=sr) == -1
        assert call(spec=NULL, n_valid=sr, out_len=sr) == -1 and call(lens=NULL, n_valid=sr, out_len=sr) == -1
        assert call(desc=NULL, n_valid=sr, out_len=sr) == -1
        assert call(nb=0, n_valid=sr, out_len=sr) == -1 and call(bk=NULL, n_valid=sr, out_len=sr) == -1
        assert call(n=-1, n_valid=sr, out_len=sr) == -1
    for out_len in (257, 16000, KB, 3 * KB + 1, 4 * KB):
        assert call(n_valid=min(out_len, 3 * KB), out_len=out_len) == -1, out_len


def test_pinned_refusals_of_the_existing_entries_still_hold(lib):
    """half buckets with out_len > kB stay refused by the entries and the binding that refused them before"""
    ok, _k = _bk(*_good())
    for sr in (KB + 1, 44100, 48000):
        assert lib.ss_audio_obs_spec_buckets_f32(P1, ok, 3, P1, P1, NULL, P1, 2, sr, sr, 0, 0, NULL) == -1
        assert lib.ss_audio_obs_spec_buckets_f32(P1, ok, 3, P1, P1, P1, P1, 2, sr, sr, 0, 0, NULL) == -1
        assert lib.ss_audio_obs_logmel_spec_buckets_f32(P1, ok, 3, P1, P1, NULL, NULL, P1, P1, P1, 64, 32, 1e-6, 2, sr, sr, 0, 0, NULL) == -1
        assert lib.ss_audio_obs_logmel_spec_buckets_f32(P1, ok, 3, P1, P1, P1, P1, P1, P1, P1, 64, 32, 1e-6, 2, sr, sr, 0, 0, NULL) == -1


def _ctx(lib, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    return h


@pytest.mark.parametrize("sr", [44100, 48000, 22050, 3 * KB])
def test_context_binding_is_accepted_on_rows_of_two_or_three_blocks(lib, sr):
    s = lib.ss_ctx_set_rir_spec_buckets_rows
    ok, _k = _bk(*_good())
    h = _ctx(lib, sr)
    try:
        for label, rows in _bad_bucket_sets():
            bad, _k2 = _bk(*rows)
            assert s(h, bad, len(rows), P1) == -1, label
        assert s(h, ok, 3, NULL) == -1                                                # no lengths
        assert s(h, NULL, 3, P1) == -1
        assert s(NULL, ok, 3, P1) == -1
        assert lib.ss_ctx_set_rir_spec_buckets(h, ok, 3, P1) == -1                    # the plain binding still refuses half buckets here
        assert s(h, ok, 3, P1) == 0
        # one form at a time: nothing binds next to the spectral buckets ...
        assert lib.ss_ctx_set_rir_spectra16(h, P1, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra16_rows(h, P1, P1, 5) == -1
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
        assert s(h, ok, 3, P1) == 0                                                   # ... rebinding (a bucket was reallocated) is fine,
        assert lib.ss_ctx_set_rir_bank(h, NULL, P1, 0, 0, 1, sr) == 0                 # and a new bank replaces them
        assert lib.ss_ctx_set_rir_spectra16_rows(h, P1, P1, P.ceil_div(sr, KB)) == 0
        assert s(h, ok, 3, P1) == 0                                               # replaces any earlier binding (a half bank here)
        assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
        fp32, _k3 = _bk(*_good(half=False))
        assert lib.ss_ctx_set_rir_spec_buckets(h, fp32, 3, P1) == 0                   # fp32 buckets through the plain binding: as before
        assert s(h, fp32, 3, P1) == -1
    finally:
        lib.ss_ctx_destroy(h)


@pytest.mark.parametrize("sr", [16000, KB])
def test_context_binding_is_refused_on_one_block_rows(lib, sr):
    ok, _k = _bk(*_good())
    h = _ctx(lib, sr)
    try:
        assert lib.ss_ctx_set_rir_spec_buckets_rows(h, ok, 3, P1) == -1
        if sr <= KB:                                                                  # ... where the plain binding serves half buckets
            assert lib.ss_ctx_set_rir_spec_buckets(h, ok, 3, P1) == 0
            assert lib.ss_ctx_set_rir_spec_buckets_rows(h, ok, 3, P1) == -1           # (and stays bound: nothing changed)
            assert lib.ss_ctx_set_rir_spectra(h, P1, 5) == -1
    finally:
        lib.ss_ctx_destroy(h)


def test_context_plans_at_the_deepest_buckets_depth(lib):
    """the planner alone (host only): planning depth = the longest bucket's blocks + the row's blocks - 1, SS_FLAG_FIRST_BUCKET for
    steps inside bucket 0"""
    import numpy as np
    from ss_amd.context import AudioContext
    ok, _k = _bk(*_good())
    ctx = AudioContext(44100)
    try:
        ctx.add_source_len("a", 44100)
        assert lib.ss_ctx_set_rir_spec_buckets_rows(ctx._h, ok, 3, P1) == 0
        assert ctx.stats()["slots_per_key"] == 5 + 3 - 1
        inside = ctx.plan(np.asarray([0, 0], np.int32), np.asarray([0, 0], np.int32), np.asarray([0, 2], np.int32))
        across = ctx.plan(np.asarray([0, 0], np.int32), np.asarray([0, 0], np.int32), np.asarray([0, 7], np.int32))
        assert inside[1] == ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET and across[1] == ops.FLAG_NO_DISTRACTOR
    finally:
        ctx.close()


def test_engine_value_errors():
    from ss_amd.renderer import AudioEngine
    bk = [(8, 16384), (4, 3 * KB)]
    for sr in (44100, 48000):
        # without the keyword: today's refusal and its wording
        with pytest.raises(ValueError, match="fused row kernels do not read half bucketed banks yet"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True)
        with pytest.raises(ValueError, match="fused row kernels do not read half bucketed banks yet"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_rows=True)
        # the keyword without the other three
        for kw in (dict(rir_spectral="half", rir_buckets=bk), dict(rir_spectral="half", rir_spectral_buckets=True),
                   dict(rir_spectral="only", rir_buckets=bk, rir_spectral_buckets=True), dict(rir_buckets=bk), dict(),
                   dict(rir_spectral="half", rir_half_rows=True), dict(rir_spectral=True, rir_buckets=bk)):
            with pytest.raises(ValueError, match="rir_half_bucket_rows goes with"):
                AudioEngine(sr, device="cpu", rir_half_bucket_rows=True, **kw)
        # with all four: served - on a GPU
        with pytest.raises(ValueError, match="GPU"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_bucket_rows=True)
        # the SoundSpaces 2.0 and policy refusals stand
        with pytest.raises(ValueError, match="SoundSpaces 2.0"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_bucket_rows=True,
                        step_time=0.25)
        with pytest.raises(ValueError, match="spectral_max_units"):
            AudioEngine(sr, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_bucket_rows=True,
                        spectral_max_units=8)
    with pytest.raises(ValueError, match="three partition blocks"):
        AudioEngine(96000, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_bucket_rows=True)
    with pytest.raises(ValueError, match="GPU"):                             # one-block rows: the keyword changes nothing
        AudioEngine(16000, device="cpu", rir_spectral="half", rir_buckets=bk, rir_spectral_buckets=True, rir_half_bucket_rows=True)


def test_engine_hands_the_half_form_to_the_bucketed_store(monkeypatch):
    """the constructor's plumbing, without a device"""
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
    eng = Rn.AudioEngine(44100, device="cuda", rir_buckets=[(3, 16384), (2, 49152)], rir_spectral="half", rir_spectral_buckets=True,
                         rir_half_bucket_rows=True)
    assert seen["spectral"] == "half" and seen["spectral_buckets"] is True and seen["caps"] == [16384, 49152]
    assert eng.rir_spectral_only and eng.rir_spectral_half and eng.renderer.rirs is eng.store.bank
