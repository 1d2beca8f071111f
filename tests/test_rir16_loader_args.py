"""The in-call loaders on half-precision time-domain rows, the parts that need no GPU (include/ss_hip.h:
``ss_bank_scatter_rows16_max_f32``, ``ss_wav_read_rirs_max_f32``, ``ss_miss_loader.stage_max``):

  * the reader's maxima (``ss_wav_read_rirs_max_f32``, csrc/ss_wavio.hpp) against ``np.abs(x[:kept]).max(0)``, exactly: a plain
    file, a clipped read whose file's peak lies behind ``keep`` (it must not count), an empty file, an int16 file (status 1, maxima
    0) and a missing one; rows, kept, frames and statuses are those of ``ss_wav_read_rirs_f32``;
  * every refusal of the new scatter entry is SS_EINVAL (-1) from the argument checks, before a device is touched (a call that got
    past them would come back with a HIP error here, not -1); n == 0 returns 0;
  * ``ss_ctx_load_rir_files`` on both half bindings answers 1 ("not served", n_loaded == 0) to a loader without ``stage_max`` and to
    one whose ``cap`` is not the binding's;
  * tests/wav_max_main.cpp, a stand-alone program built with -fsanitize=address,undefined: three tiny wav files through
    ``sswav::read_many`` with maxima (host code only; never loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import wavfile

from ss_amd import _lib, ops, planning as P

HERE = os.path.dirname(os.path.abspath(__file__))
KB = P.KB
NULL = None
P1 = ctypes.c_void_p(16)            # non-null, 16-byte aligned dummy pointer: never dereferenced on these paths
ODD2 = ctypes.c_void_p(18)
AL4 = ctypes.c_void_p(20)
BAD_CAPS = (0, 1, 15999, -2, 16 * KB + 2)       # < 2, odd, negative, more than 16 partition blocks


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_and_exported(lib):
    for name in ("ss_bank_scatter_rows16_max_f32", "ss_wav_read_rirs_max_f32"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert hasattr(ops, "scatter_rows16_max_into")
    fields = [f[0] for f in _lib.SsMissLoader._fields_]
    assert fields[-1] == "stage_max" and fields[-2] == "loaded_cap"          # ONE field, appended at the end
    text = open(os.path.join(HERE, "..", "include", "ss_hip.h")).read()
    body = text[text.index("typedef struct ss_miss_loader {"):text.index("} ss_miss_loader;")]
    assert "float* stage_max;" in body.split("int n_loaded, loaded_cap;")[1]          # ... in the header as well


# ---- the reader -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("rir16_loader_wavs")
    rng = np.random.default_rng(7)
    files, data = {}, {}
    plain = rng.standard_normal((3000, 2)).astype(np.float32)
    late = rng.uniform(-1, 1, (5000, 2)).astype(np.float32)
    late[4000] = [40.0, -50.0]                                           # the file's peak, behind keep = 3500
    late[3499] = [-2.0, 3.0]                                             # ... and the kept part's, on its last frame
    for name, x in (("plain", plain), ("late", late), ("empty", np.zeros((0, 2), np.float32))):
        files[name] = str(d / f"{name}.wav")
        wavfile.write(files[name], 16000, x)
        data[name] = x
    files["i16"] = str(d / "i16.wav")
    wavfile.write(files["i16"], 16000, (rng.standard_normal((100, 2)) * 1000).astype(np.int16))
    files["missing"] = str(d / "missing.wav")
    return files, data


def _read_max(lib, paths, cap, keep, threads, stride=None):
    n = len(paths)
    stride = 2 * cap if stride is None else stride
    dst = np.full((n, stride), 7.0, np.float32)
    kept, frames, status = (np.full((n,), -9, np.int32) for _ in range(3))
    mx = np.full((n, 2), -1.0, np.float32)
    arr = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    rc = lib.ss_wav_read_rirs_max_f32(ctypes.cast(arr, ctypes.c_void_p), n, dst.ctypes.data, stride, cap, keep, kept.ctypes.data,
                                      frames.ctypes.data, status.ctypes.data, threads, mx.ctypes.data)
    assert rc == 0
    return dst, kept, frames, status, mx


@pytest.mark.parametrize("threads", [1, 3])
def test_reader_maxima_are_those_of_the_kept_frames(lib, wavs, threads):
    files, data = wavs
    names = ["plain", "late", "empty", "i16", "missing", "plain"]
    paths = [files[n] for n in names]
    cap, keep = 5008, 3500
    dst, kept, frames, status, mx = _read_max(lib, paths, cap, keep, threads)
    ref = np.full((len(paths), cap, 2), 7.0, np.float32)
    k0, f0, s0 = _lib.wav_read_rirs(paths, ref, cap, keep=keep, threads=threads)          # ss_wav_read_rirs_f32
    assert dst.tobytes() == ref.tobytes() and kept.tolist() == k0.tolist() and frames.tolist() == f0.tolist()
    assert status.tolist() == s0.tolist() == [_lib.WAV_OK, _lib.WAV_OK, _lib.WAV_EMPTY, _lib.WAV_UNSUPPORTED, _lib.WAV_MISSING, _lib.WAV_OK]
    assert kept.tolist() == [3000, 3500, 0, 0, 0, 3000] and frames[1] == 5000
    for i, n in enumerate(names):
        want = np.abs(data[n][:kept[i]]).max(0) if status[i] == _lib.WAV_OK else np.zeros(2, np.float32)
        assert mx[i].tobytes() == np.asarray(want, np.float32).tobytes(), n
    assert mx[1].tolist() == [2.0, 3.0]                                  # the peak behind keep (40, 50) does not count
    # whole files: now it does; rows further apart than they are long
    dst, kept, frames, status, mx = _read_max(lib, paths[:2], cap, -1, threads, stride=2 * cap + 10)
    assert kept.tolist() == [3000, 5000] and mx[1].tolist() == [40.0, 50.0]
    assert (dst[:, 2 * cap:] == 7.0).all()
    # a row too short for what is to be kept: reported, nothing read, no maxima
    dst, kept, frames, status, mx = _read_max(lib, [files["plain"]], 1000, -1, threads)
    assert status[0] == _lib.WAV_TOO_LONG and not dst.any() and mx.tolist() == [[0.0, 0.0]]


def test_reader_refusals(lib):
    f = lib.ss_wav_read_rirs_max_f32
    #        paths n dst stride cap keep kept frames status threads max
    assert f(NULL, 0, NULL, 0, 0, 0, NULL, NULL, NULL, 1, NULL) == 0
    assert f(NULL, 1, P1, 32, 16, -1, P1, P1, P1, 1, P1) == -1
    assert f(P1, 1, NULL, 32, 16, -1, P1, P1, P1, 1, P1) == -1
    assert f(P1, 1, P1, 32, 16, -1, NULL, P1, P1, 1, P1) == -1
    assert f(P1, 1, P1, 32, 16, -1, P1, NULL, P1, 1, P1) == -1
    assert f(P1, 1, P1, 32, 16, -1, P1, P1, NULL, 1, P1) == -1
    assert f(P1, 1, P1, 32, 16, -1, P1, P1, P1, 1, NULL) == -1                           # the maxima are what the entry is for
    assert f(P1, -1, P1, 32, 16, -1, P1, P1, P1, 1, P1) == -1
    assert f(P1, 1, P1, 32, 0, -1, P1, P1, P1, 1, P1) == -1 and f(P1, 1, P1, 30, 16, -1, P1, P1, P1, 1, P1) == -1


# ---- the scatter entry ------------------------------------------------------------------------------------------------------------
def test_scatter_rows16_max_refusals(lib):
    f = lib.ss_bank_scatter_rows16_max_f32
    #        staged stride slots lens row_max n rir16 rscale cap bank_len stream
    assert f(P1, 32000, P1, P1, P1, 0, P1, P1, 16000, P1, NULL) == 0                     # no rows: no launch
    assert f(NULL, 0, NULL, NULL, NULL, 0, NULL, NULL, 0, NULL, NULL) == 0
    assert f(NULL, 32000, P1, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 32000, NULL, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 32000, P1, NULL, P1, 2, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 32000, P1, P1, NULL, 2, P1, P1, 16000, P1, NULL) == -1                  # no maxima
    assert f(P1, 32000, P1, P1, ODD2, 2, P1, P1, 16000, P1, NULL) == -1                  # maxima not 4-byte aligned
    assert f(P1, 32000, P1, P1, P1, 2, NULL, P1, 16000, P1, NULL) == -1                  # null halves
    assert f(P1, 32000, P1, P1, P1, 2, P1, NULL, 16000, P1, NULL) == -1                  # null scales
    assert f(P1, 32000, P1, P1, P1, 2, ODD2, P1, 16000, P1, NULL) == -1                  # misaligned halves
    assert f(P1, 32000, P1, P1, P1, -1, P1, P1, 16000, P1, NULL) == -1
    assert f(P1, 31998, P1, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1                    # rows shorter than the capacity
    assert f(P1, 32001, P1, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1                    # odd stride
    assert f(AL4, 32000, P1, P1, P1, 2, P1, P1, 16000, P1, NULL) == -1                   # staged not 8-byte aligned
    for cap in BAD_CAPS:
        assert f(P1, 1 << 20, P1, P1, P1, 2, P1, P1, cap, P1, NULL) == -1, cap
    # pageable host memory - for the maxima as for the other staged arrays: refused, not dereferenced
    staged = np.zeros((2, 16000, 2), np.float32)
    idx, lens, mx = np.zeros((2,), np.int32), np.zeros((2,), np.int32), np.zeros((2, 2), np.float32)
    assert f(staged.ctypes.data, 32000, idx.ctypes.data, lens.ctypes.data, mx.ctypes.data, 2, P1, P1, 16000, NULL, NULL) == -1


# ---- the loaders' third bank kind: when it does NOT apply ---------------------------------------------------------------------------
def _loader(cap, stage_max):
    """a struct with every array the file loader asks for (dummy pointers: a loader that is not served reads none of them)"""
    ld = _lib.SsMissLoader()
    for name in ("free_slots", "dev_len", "host_len", "clipped", "stage", "stage_slot", "stage_len", "loaded_slot", "loaded_frames",
                 "loaded_key", "pair_keys", "pair_slots"):
        setattr(ld, name, 16)
    ld.n_free, ld.stage_rows, ld.loaded_cap, ld.threads, ld.keep = 4, 4, 4, 1, -1
    ld.bank, ld.cap, ld.stage_max = None, cap, stage_max
    ld.n_loaded = 5                                                      # (the call resets it)
    return ld


@pytest.mark.parametrize("binding", ["ss_ctx_set_rir_bank16", "ss_ctx_set_rir_bank16_rows"])
@pytest.mark.parametrize("sr", [16000, 44100])
def test_file_loader_answers_not_served_without_maxima_or_with_another_capacity(lib, binding, sr):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), sr, sr, 0, 0, 0) == 0
    try:
        assert getattr(lib, binding)(h, P1, P1, P1, sr) == 0
        paths = (ctypes.c_char_p * 1)(b"/nonexistent.wav")
        for ld in (_loader(sr, None), _loader(sr - 2, 16), _loader(sr + 2, 16)):
            assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 4, NULL) == 1
            assert ld.n_loaded == 0 and ld.n_evicted == 0 and ld.n_free == 4
        ld = _loader(sr, 16)                                             # a loader that lends ROWS is not this kind either
        ld.bank = 16
        assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 4, NULL) == 1
        assert ld.n_loaded == 0
    finally:
        lib.ss_ctx_destroy(h)


def test_bucketed_half_rows_stay_not_served(lib):
    h = ctypes.c_void_p()
    assert lib.ss_ctx_create(ctypes.byref(h), 16000, 16000, 0, 0, 0) == 0
    try:
        bk = (_lib.SsRir16Bucket * 1)(_lib.SsRir16Bucket(16, 16, 0, 8, 16000, 0))
        assert lib.ss_ctx_set_rir16_buckets(h, ctypes.cast(bk, ctypes.c_void_p), 1, P1) == 0
        ld = _loader(16000, 16)
        paths = (ctypes.c_char_p * 1)(b"/nonexistent.wav")
        assert lib.ss_ctx_load_rir_files(h, ctypes.byref(ld), ctypes.cast(paths, ctypes.c_void_p), 1, NULL, 0, 4, NULL) == 1
        assert ld.n_loaded == 0
    finally:
        lib.ss_ctx_destroy(h)


# ---- the stand-alone sanitised program ----------------------------------------------------------------------------------------------
def test_reader_with_maxima_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    prog = str(tmp_path / "wav_max_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", os.path.join(HERE, "wav_max_main.cpp"), "-o", prog])
    work = tmp_path / "wavs"
    work.mkdir()
    r = subprocess.run([prog, str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    assert sorted(os.listdir(work)) == ["a.wav", "b.wav", "c.wav"]
    rate, a = wavfile.read(str(work / "a.wav"))                          # (what it wrote is what scipy reads)
    assert rate == 16000 and a.dtype == np.float32 and a.shape == (700, 2) and a[699, 0] == -3.5
