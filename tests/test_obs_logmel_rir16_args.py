"""The one-launch log-mel entries over half-precision time-domain rows (include/ss_hip.h: ``ss_audio_obs_logmel_rir16_f32``,
``ss_audio_obs_logmel_rows_rir16_f32``, ``ss_audio_obs_logmel_rir16_buckets_f32``, ``ss_ctx_set_logmel_rir16_policy``): every
refusal is SS_EINVAL (-1) from the argument checks, before a device is touched (this file runs without a GPU: a call that got past
the checks would come back with a HIP error, not -1); n_units == 0 returns 0; the exports and the Python layer are there.

Route (tests/route_rir16_logmel_host.cpp, a stand-alone program built with -fsanitize=address,undefined): with the new range at
its default the three rir16 bindings print what their own programs print - and tests/golden/route_rir16_buckets_table.txt and
route_table.txt - line for line; with the range set, the grid pinned in tests/golden/route_rir16_logmel_table.txt."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

from ss_amd import _lib, ops, planning as P

KB = P.KB
HERE = os.path.dirname(os.path.abspath(__file__))
NULL = None
P1 = ctypes.c_void_p(16)            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
ONE, ODD2, AL4, AL8 = 16, 18, 20, 24
XF = ops.FLAG_CROSSFADE
EPS = ctypes.c_float(1e-6)
BAD_CAPS = (0, 1, 15999, -2, 16 * KB + 2)       # < 2, odd, negative, more than 16 partition blocks
# (label, overrides) of the mel arguments the limits of ss_audio_features_f32 refuse
BAD_MEL = [("null logmel", dict(mel=NULL)), ("null starts", dict(start=NULL)), ("null weights", dict(w=NULL)),
           ("weights not 16-byte aligned", dict(w=ctypes.c_void_p(AL8))), ("no bands", dict(n_mels=0)), ("65 bands", dict(n_mels=65)),
           ("table of 64 x 52", dict(max_len=52)), ("max_len 0", dict(max_len=0)), ("max_len 6", dict(max_len=6)), ("max_len 68", dict(max_len=68)),
           ("eps 0", dict(eps=ctypes.c_float(0.0))), ("eps < 0", dict(eps=ctypes.c_float(-1e-6)))]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_and_exported(lib):
    for name in ("ss_audio_obs_logmel_rir16_f32", "ss_audio_obs_logmel_rows_rir16_f32", "ss_audio_obs_logmel_rir16_buckets_f32",
                 "ss_ctx_set_logmel_rir16_policy"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    for name in ("audio_obs_logmel_rir16_into", "audio_obs_logmel_rows_rir16_into", "audio_obs_logmel_rir16_buckets_into"):
        assert hasattr(ops, name)
    from ss_amd.context import AudioContext
    assert list(inspect.signature(AudioContext.set_logmel_rir16_policy).parameters) == ["self", "min_units", "max_units"]
    with open(os.path.join(HERE, "..", "include", "ss_hip.h")) as f:
        header = f.read()
    for name in ("ss_audio_obs_logmel_rir16_f32(", "ss_audio_obs_logmel_rows_rir16_f32(", "ss_audio_obs_logmel_rir16_buckets_f32(",
                 "ss_ctx_set_logmel_rir16_policy("):
        assert "int " + name in header


def _single(f, lo, hi):
    """the refusals the two single-allocation entries share; [lo, hi]: the entry's out_len range"""
    def call(spec=P1, q=P1, s=P1, lens=P1, desc=P1, ag=NULL, sg=NULL, mel=P1, start=P1, w=P1, n_mels=64, max_len=32, eps=EPS, n=2,
             cap=16000, n_valid=None, out_len=lo, pad=0, flags=0):
        return f(spec, q, s, lens, desc, ag, sg, mel, start, w, n_mels, max_len, eps, n, cap, out_len if n_valid is None else n_valid,
                 out_len, pad, flags, NULL)

    assert call(n=0) == 0 and call(n=0, q=NULL, s=NULL, mel=NULL) == 0                  # no units: nothing to do
    for ag in (NULL, P1):
        for sg in (NULL, P1):                                                          # both optional, everything else is not
            kw = dict(ag=ag, sg=sg)
            assert call(q=NULL, **kw) == -1 and call(s=NULL, **kw) == -1 and call(q=ctypes.c_void_p(ODD2), **kw) == -1
            for cap in BAD_CAPS:
                assert call(cap=cap, **kw) == -1, cap
            assert call(flags=XF, **kw) == -1 and call(flags=XF | ops.FLAG_NO_DISTRACTOR, **kw) == -1
            for label, bad in BAD_MEL:
                assert call(**bad, **kw) == -1, label
            assert call(pad=7, **kw) == -1 and call(pad=-1, **kw) == -1
            assert call(spec=NULL, **kw) == -1 and call(lens=NULL, **kw) == -1 and call(desc=NULL, **kw) == -1
            assert call(n=-1, **kw) == -1
            assert call(n_valid=hi + 1, out_len=hi, **kw) == -1 and call(n_valid=-1, **kw) == -1
            for out_len in (1, 256, lo - 1, hi + 1, 4 * KB):
                assert call(out_len=out_len, n_valid=min(out_len, lo), **kw) == -1, out_len
    return call


def test_logmel_rir16_refusals(lib):
    call = _single(lib.ss_audio_obs_logmel_rir16_f32, 257, KB)
    assert call(out_len=44100) == -1 and call(out_len=KB + 1) == -1                     # longer rows: the rows entry


def test_logmel_rows_rir16_refusals(lib):
    call = _single(lib.ss_audio_obs_logmel_rows_rir16_f32, KB + 1, 3 * KB)
    assert call(out_len=16000) == -1 and call(out_len=KB) == -1                         # one-block rows: the other entry
    assert call(out_len=44100, cap=16 * KB + 2) == -1                                   # more than 16 RIR blocks
    assert call(out_len=44100, n_valid=44101) == -1


def _buckets(*rows):
    arr = (_lib.SsRir16Bucket * max(1, len(rows)))()
    for b, (q, s, first, n, cap) in enumerate(rows):
        arr[b].rir16, arr[b].rscale, arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = q, s, first, n, cap, 0
    return ctypes.cast(arr, ctypes.c_void_p), len(rows), arr


GOOD = ((ONE, ONE, 0, 3, 16000), (AL4, ONE, 3, 2, 20000), (ONE, ONE, 5, 3, 40000), (ONE, ONE, 8, 2, 70000))


def _bad_arrays():
    out = [("null halves", ((None, ONE, 0, 3, 16000),)), ("2-byte aligned halves", ((ODD2, ONE, 0, 3, 16000),)),
           ("null scales", ((ONE, None, 0, 3, 16000),)), ("null halves in bucket 2", GOOD[:2] + ((None, ONE, 5, 3, 40000),)),
           ("null scales in bucket 3", GOOD[:3] + ((ONE, None, 8, 2, 70000),)),
           ("unordered", (GOOD[0], GOOD[2], GOOD[1])), ("overlapping", (GOOD[0], (ONE, ONE, 2, 2, 20000))),
           ("bucket 0 not at 0", ((ONE, ONE, 1, 3, 16000),)), ("negative entries", ((ONE, ONE, 0, -1, 16000),)),
           ("five buckets", GOOD + ((ONE, ONE, 10, 1, 80000),))]
    for cap in BAD_CAPS:
        out.append((f"cap {cap}", ((ONE, ONE, 0, 3, cap),)))
        out.append((f"cap {cap} in bucket 1", (GOOD[0], (ONE, ONE, 3, 2, cap))))
    return out


def test_logmel_rir16_buckets_refusals(lib):
    f = lib.ss_audio_obs_logmel_rir16_buckets_f32

    def call(rows=GOOD, spec=P1, lens=P1, desc=P1, ag=NULL, sg=NULL, mel=P1, start=P1, w=P1, n_mels=64, max_len=32, eps=EPS, n=2,
             n_valid=None, out_len=16000, pad=0, flags=0, n_buckets=None, null=False):
        ptr, nb, keep = _buckets(*rows)
        return f(spec, NULL if null else ptr, nb if n_buckets is None else n_buckets, lens, desc, ag, sg, mel, start, w, n_mels, max_len,
                 eps, n, out_len if n_valid is None else n_valid, out_len, pad, flags, NULL)

    assert call(n=0) == 0 and call(n=0, null=True, n_buckets=0, mel=NULL) == 0
    for ag in (NULL, P1):
        for sg in (NULL, P1):
            kw = dict(ag=ag, sg=sg)
            for label, rows in _bad_arrays():
                assert call(rows=rows, **kw) == -1, label
            assert call(null=True, **kw) == -1 and call(n_buckets=0, **kw) == -1 and call(n_buckets=5, **kw) == -1
            assert call(flags=XF, **kw) == -1 and call(flags=XF | ops.FLAG_NO_DISTRACTOR | ops.FLAG_FIRST_BUCKET, **kw) == -1
            for label, bad in BAD_MEL:
                assert call(**bad, **kw) == -1, label
            assert call(pad=7, **kw) == -1 and call(pad=-1, **kw) == -1
            assert call(spec=NULL, **kw) == -1 and call(lens=NULL, **kw) == -1 and call(desc=NULL, **kw) == -1
            assert call(n=-1, **kw) == -1
            assert call(n_valid=16001, **kw) == -1 and call(n_valid=-1, **kw) == -1
            for out_len in (1, 256, KB + 1, 20000, 44100, 48000, 4 * KB):              # rows longer than kB: never on the buckets entry
                assert call(out_len=out_len, n_valid=min(out_len, KB), **kw) == -1, out_len


def test_policy_setter_arguments(lib):
    s = lib.ss_ctx_set_logmel_rir16_policy
    assert s(NULL, 1, 0) == -1
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), 16000, 16000, 0, 0, 0) == 0
    try:
        assert s(h, -1, 5) == -1 and s(h, 1, -1) == -1
        assert s(h, 1, 0) == 0 and s(h, 1, 2 ** 31 - 1) == 0 and s(h, 0, 0) == 0
    finally:
        assert lib.ss_ctx_destroy(h) == 0


# ---- route --------------------------------------------------------------------------------------------------------------------
WAVE, SGRAM, BOTH, MEL, MEL_SGRAM, MEL_WITH_WAVE = range(6)
ROWS16, ROWS16_ROWS, ROWS16_BK = range(3)


def _build(tmp_path_factory, name):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, name + ".cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def route_prog(tmp_path_factory):
    return _build(tmp_path_factory, "route_rir16_logmel_host")


def _lines(prog, mode):
    r = subprocess.run([prog, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return [ln for ln in f.read().splitlines() if not ln.startswith("#")]


def test_route_fields_clear_print_the_recorded_table(route_prog):
    golden = _golden("route_table.txt")
    assert len(golden) == 10 * 9 * 3 * 4 + 10 * 4 * 3 * 4 and _lines(route_prog, "table") == golden


@pytest.mark.parametrize("sibling,mode,count", [("route_rir16_host", "rows16", 9 * 3 * 4 * 5 * 2 * 3),
                                                ("route_rir16_rows_host", "rows16_rows", 9 * 3 * 4 * 5 * 2 * 3),
                                                ("route_rir16_buckets_host", "rows16bk", 9 * 3 * 8 * 5 * 2 * 3)])
def test_default_range_prints_todays_tables(route_prog, tmp_path_factory, sibling, mode, count):
    """the range at its default (never): line for line what the binding's own program prints - no m / r route anywhere"""
    lines = _lines(route_prog, mode)
    assert len(lines) == count and lines == _lines(_build(tmp_path_factory, sibling), mode)
    assert not any(ln.split()[-1][0] in "mrs" for ln in lines)
    if mode == "rows16bk":
        assert lines == _golden("route_rir16_buckets_table.txt")


def test_route_with_the_range_set(route_prog):
    lines = _lines(route_prog, "logmel")
    assert len(lines) == 3 * 9 * 3 * 4 * 6 * 2 and lines == _golden("route_rir16_logmel_table.txt")
    seen = {b: set() for b in range(3)}
    for ln in lines:
        binding, out_len, n_valid, depth, flags, w, n, code = ln.split()
        binding, out_len, n_valid, depth, flags, w, n = (int(x) for x in (binding, out_len, n_valid, depth, flags, w, n))
        if flags & 2:                                                    # a cross-fade: refused, whatever is asked for
            assert code == "-8", ln
            continue
        one_block = 257 <= out_len <= KB
        rows_shape = KB < out_len <= 3 * KB and n_valid <= out_len and depth <= 16
        if w in (MEL, MEL_SGRAM) and n == 1 and one_block:
            assert code == "m0", ln                                      # every binding: one launch, no scratch
        elif w in (MEL, MEL_SGRAM) and n == 1 and binding == ROWS16_ROWS and rows_shape:
            assert code == "r0", ln                                      # only the binding made for the row kernels
        elif w in (MEL, MEL_SGRAM, MEL_WITH_WAVE):
            assert code[0] in "CFRT" and code[1] == "2", ln              # outside the range, long bucketed rows, with a waveform buffer: scratch
            if binding != ROWS16_ROWS:
                assert code[0] != "R", ln
        else:
            assert code[0] in "CFRT" and code[1] in "04", ln             # no log-mel asked: nothing changed
        seen[binding].add(code)
    assert "r0" in seen[ROWS16_ROWS] and "r0" not in seen[ROWS16] and "r0" not in seen[ROWS16_BK]
    assert all("m0" in s and "C2" in s for s in seen.values())
