"""Log-mel entries of the length-bucketed banks (include/ss_hip.h ``ss_audio_obs_logmel_buckets_f32`` /
``ss_audio_obs_logmel_spec_buckets_f32`` / ``ss_ctx_set_logmel_buckets_policy``): the three exports exist, every refusal is
SS_EINVAL (-1) from the argument checks, before a device is touched (this file runs without a GPU: a call that got past the checks
would come back with a HIP error, not -1), and a launch of no units returns 0."""
import ctypes

import pytest

from ss_amd import _lib, ops, planning as P
from ss_amd.context import AudioContext

KB = P.KB
ONE = 16                            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
TWO = 4096
ODD8 = 24                           # 8-byte but not 16-byte aligned
ODD = 20                            # not 8-byte aligned
NULL = None
P1 = ctypes.c_void_p(ONE)
XF = ops.FLAG_CROSSFADE
FB = ops.FLAG_FIRST_BUCKET
CAPS = (16000, 20000, 40000, 70000)
MEL = (P1, P1, 64, 32, 1e-6)        # mel_start, mel_w, n_mels, max_len, eps: inside ss_audio_features_f32's limits


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _rows_bk(*rows):
    """ss_rir_bucket array from (rir, hspec, first, n_entries, cap) rows"""
    arr = (_lib.SsRirBucket * max(1, len(rows)))()
    for b, (rir, hspec, first, n, cap) in enumerate(rows):
        arr[b].rir, arr[b].hspec, arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = rir, hspec, first, n, cap, 0
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _spec_bk(*rows):
    """ss_spec_bucket array from (hspec, hscale, first, n_entries, cap) rows"""
    arr = (_lib.SsSpecBucket * max(1, len(rows)))()
    for b, (hspec, hscale, first, n, cap) in enumerate(rows):
        arr[b].hspec, arr[b].hscale, arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = hspec, hscale, first, n, cap, 0
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _good_rows(spectra, n=4):
    return [(ONE + 64 * b, (TWO + 64 * b) if spectra else NULL, 3 * b, 3, CAPS[b]) for b in range(n)]


def _good_spec(half, n=4):
    return [(ONE + 64 * b, (TWO + 64 * b) if half else NULL, 3 * b, 3, CAPS[b]) for b in range(n)]


def _with(good, names, b, **kw):
    rows = [list(r) for r in good]
    for k, v in kw.items():
        rows[b][names.index(k)] = v
    return [tuple(r) for r in rows]


def _bad_rows_sets(spectra):
    """every ss_rir_bucket array fill_buckets refuses"""
    g = _good_rows(spectra)
    names = ("rir", "hspec", "first", "n", "cap")
    return [("null rows", _with(g, names, 2, rir=NULL)),
            ("five buckets", g + [(ONE, TWO if spectra else NULL, 12, 3, 80000)]),
            ("first descending", _with(g, names, 2, first=2)),
            ("overlapping ranges", _with(g, names, 1, first=2)),
            ("negative first", _with(g, names, 1, first=-1)),
            ("bucket 0 does not start at 0", [(ONE, TWO if spectra else NULL, 1, 3, 16000)]),
            ("odd cap", _with(g, names, 1, cap=20001)),
            ("cap < 2", _with(g, names, 0, cap=0)),
            ("negative count", _with(g, names, 0, n=-1))]


def _bad_spec_sets(half):
    """every ss_spec_bucket array spec_buckets_check refuses"""
    g = _good_spec(half)
    names = ("hspec", "hscale", "first", "n", "cap")
    sc = TWO if half else NULL
    out = [("null hspec", _with(g, names, 2, hspec=NULL)),
           ("misaligned hspec", _with(g, names, 1, hspec=ODD)),
           ("mixed forms", _with(g, names, 3, hscale=NULL if half else TWO)),
           ("five buckets", g + [(ONE, sc, 12, 3, 80000)]),
           ("first descending", _with(g, names, 2, first=2)),
           ("overlapping ranges", _with(g, names, 1, first=2)),
           ("bucket 0 does not start at 0", [(ONE, sc, 1, 3, 16000)]),
           ("odd cap", _with(g, names, 1, cap=20001)),
           ("cap < 2", _with(g, names, 0, cap=0)),
           ("negative count", _with(g, names, 0, n=-1)),
           ("17 blocks", _with(g, names, 3, cap=16 * KB + 2))]
    if not half:
        out.append(("fp32 spectra not 16-byte aligned", _with(g, names, 1, hspec=ODD8)))
    return out


def test_declared_and_exported(lib):
    for name in ("ss_audio_obs_logmel_buckets_f32", "ss_audio_obs_logmel_spec_buckets_f32", "ss_ctx_set_logmel_buckets_policy"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert hasattr(ops, "audio_obs_logmel_buckets_into") and hasattr(ops, "audio_obs_logmel_spec_buckets_into")
    assert hasattr(AudioContext, "set_logmel_buckets_policy")


def _call(f, bk, nb, *, spec=P1, rir_len=P1, desc=P1, ag=NULL, sg=NULL, logmel=P1, mel=MEL, n=2, n_valid=16000, out_len=16000,
          pad=0, flags=0):
    start, w, n_mels, max_len, eps = mel
    return f(spec, bk, nb, rir_len, desc, ag, sg, logmel, start, w, n_mels, max_len, eps, n, n_valid, out_len, pad, flags, NULL)


def _common_refusals(f, ok, out_lens):
    """the refusals both entries share, on a good bucket array"""
    for out_len in out_lens:
        kw = dict(out_len=out_len, n_valid=out_len)
        assert _call(f, ok, 4, n=0, **kw) == 0                                         # no units: nothing to do
        assert _call(f, ok, 4, n=-1, **kw) == -1
        assert _call(f, ok, 4, flags=XF, **kw) == -1                                   # cross-fade
        assert _call(f, ok, 4, flags=XF | FB, **kw) == -1
        assert _call(f, ok, 4, pad=7, **kw) == -1                                      # unknown pad mode
        assert _call(f, ok, 4, pad=-1, **kw) == -1
        assert _call(f, ok, 4, logmel=NULL, **kw) == -1                                # log-mel is the required output
        assert _call(f, ok, 4, spec=NULL, **kw) == -1
        assert _call(f, ok, 4, rir_len=NULL, **kw) == -1
        assert _call(f, ok, 4, desc=NULL, **kw) == -1
        assert _call(f, ok, 0, **kw) == -1
        assert _call(f, NULL, 4, **kw) == -1
        assert _call(f, ok, 4, out_len=out_len, n_valid=out_len + 1) == -1             # n_valid outside [0, out_len]
        assert _call(f, ok, 4, out_len=out_len, n_valid=-1) == -1
        # the mel limits (ss_audio_features_f32's)
        for label, mel in (("no bands table", (NULL, P1, 64, 32, 1e-6)), ("no weights", (P1, NULL, 64, 32, 1e-6)),
                           ("misaligned weights", (P1, ctypes.c_void_p(ODD), 64, 32, 1e-6)), ("no bands", (P1, P1, 0, 32, 1e-6)),
                           ("too many bands", (P1, P1, 65, 32, 1e-6)), ("max_len not a multiple of 4", (P1, P1, 64, 30, 1e-6)),
                           ("max_len < 4", (P1, P1, 64, 0, 1e-6)), ("max_len > 64", (P1, P1, 8, 68, 1e-6)),
                           ("eps = 0", (P1, P1, 64, 32, 0.0)), ("eps < 0", (P1, P1, 64, 32, -1e-6))):
            assert _call(f, ok, 4, mel=mel, **kw) == -1, label
    assert _call(f, ok, 4, out_len=256, n_valid=256) == -1                             # shorter than the reflect padding
    assert _call(f, ok, 4, out_len=3 * KB + 1, n_valid=3 * KB + 1) == -1               # more than three blocks
    assert _call(f, ok, 4, out_len=3 * KB + 1, n_valid=KB) == -1


@pytest.mark.parametrize("spectra", [False, True], ids=["rows", "rows+spectra"])
def test_rows_buckets_entry_refusals(lib, spectra):
    f = lib.ss_audio_obs_logmel_buckets_f32
    ok, _k = _rows_bk(*_good_rows(spectra))
    _common_refusals(f, ok, (16000, 44100))
    for out_len in (16000, 44100):
        for label, rows in _bad_rows_sets(spectra):
            bad, _k2 = _rows_bk(*rows)
            assert _call(f, bad, len(rows), out_len=out_len, n_valid=out_len) == -1, (label, out_len)
    # rows of 2 or 3 blocks: at most 16 RIR blocks in the deepest bucket
    deep, _k3 = _rows_bk(*_with(_good_rows(spectra), ("rir", "hspec", "first", "n", "cap"), 3, cap=16 * KB + 2))
    assert _call(f, deep, 4, out_len=44100, n_valid=44100) == -1
    assert _call(f, deep, 4, out_len=44100, n_valid=44100, flags=FB) == -1


@pytest.mark.parametrize("half", [False, True], ids=["only", "half"])
def test_spec_buckets_entry_refusals(lib, half):
    f = lib.ss_audio_obs_logmel_spec_buckets_f32
    ok, _k = _spec_bk(*_good_spec(half))
    _common_refusals(f, ok, (16000,) if half else (16000, 44100))
    for label, rows in _bad_spec_sets(half):
        bad, _k2 = _spec_bk(*rows)
        assert _call(f, bad, len(rows)) == -1, label
    if half:                                                                          # half: rows of one partition block
        for out_len in (KB + 1, 44100, 48000):
            for flags in (0, FB):
                assert _call(f, ok, 4, out_len=out_len, n_valid=out_len, flags=flags) == -1
                assert _call(f, ok, 4, out_len=out_len, n_valid=out_len, flags=flags, ag=P1, sg=P1) == -1
                assert _call(f, ok, 4, out_len=out_len, n_valid=KB, flags=flags) == -1
        one, _k3 = _spec_bk(*_good_spec(True, 1))
        assert _call(f, one, 1, out_len=44100, n_valid=44100) == -1


def test_policy_setter(lib):
    s = lib.ss_ctx_set_logmel_buckets_policy
    assert s(NULL, 1, 2 ** 31 - 1) == -1
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), 16000, 16000, 0, 0, 0) == 0
    try:
        assert s(h, 1, 2 ** 31 - 1) == 0
        assert s(h, 1, 0) == 0                                                        # never (the default)
        assert s(h, -1, 4) == -1 and s(h, 1, -4) == -1
    finally:
        lib.ss_ctx_destroy(h)
