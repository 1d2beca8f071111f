"""Captured steps, the parts that need no GPU (include/ss_hip.h "Captured steps"):

  * ss_stream_reserve / ss_stream_replay_epoch return SS_EINVAL (-1) from the argument checks alone - no device is touched
    (dummy stream handles, CPU-only machine);
  * the pure rules of csrc/ss_launch.hpp through a stand-alone host program (tests/stream_reserve_host.cpp, built with the
    sanitizers as the other host programs are): a launch USES a scratch that is large enough, capturing or not; one that would
    have to allocate or grow does so on a plain stream and is REFUSED on a capturing one (what get_stash and get_block_sync do
    about the k_obs_rows stash and the k_obs_blocks hand-off area); ss_stream_reserve's argument rule; the hand-off area's size
    with the replay epoch word behind the flags."""
import ctypes
import os
import shutil
import subprocess

import pytest

from ss_amd import _lib
from ss_amd import planning as P

HERE = os.path.dirname(os.path.abspath(__file__))
STREAM = ctypes.c_void_p(16)           # a non-null dummy handle: never dereferenced on these paths
PER_THREAD = ctypes.c_void_p(2)        # hipStreamPerThread


def test_stream_reserve_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    good = dict(out_len=44100, rir_cap=2048, n_terms=2)

    def rc(stream=STREAM, **kw):
        a = dict(good, **kw)
        return lib.ss_stream_reserve(stream, a["out_len"], a["rir_cap"], a["n_terms"])

    assert rc(stream=PER_THREAD) == -1                                  # one handle for a different stream on every thread
    assert rc(out_len=P.KB) == -1                                       # one partition block: no scratch, no hand-off area
    assert rc(out_len=16000) == -1
    assert rc(out_len=0) == -1
    assert rc(out_len=3 * P.KB + 1) == -1                               # more than three
    assert rc(rir_cap=0) == -1
    assert rc(rir_cap=-5) == -1
    assert rc(n_terms=0) == -1
    assert rc(n_terms=3) == -1
    assert rc(stream=PER_THREAD, out_len=P.KB + 1, rir_cap=1, n_terms=1) == -1      # (the smallest shape: still the stream)


def test_stream_replay_epoch_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    out = ctypes.c_int(123)
    assert lib.ss_stream_replay_epoch(PER_THREAD, ctypes.byref(out)) == -1
    assert lib.ss_stream_replay_epoch(STREAM, None) == -1
    assert out.value == 123


def test_exports_are_listed():
    for name in ("ss_stream_reserve", "ss_stream_replay_epoch"):
        assert name in _lib.EXPORTS


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("stream_reserve") / "stream_reserve_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "stream_reserve_host.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_scratch_decision_use_allocate_refuse(lines):
    rows = [ln[1:] for ln in lines if ln[0] == "scratch"]
    assert len(rows) == 2 * 4 * 4
    seen = set()
    for cap, have, need, got in rows:
        cap, have, need = int(cap), int(have), int(need)
        want = "U" if have >= need else ("R" if cap else "A")          # enough: use; else allocate - never inside a capture
        assert got == want, (cap, have, need, got)
        seen.add((cap, got))
    assert seen == {(0, "U"), (0, "A"), (1, "U"), (1, "R")}


def test_reserve_argument_rule_and_handoff_size(lines):
    rows = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "reserve"]
    assert len(rows) == 2 * 7 * 4 * 4
    for ok, out_len, cap, terms, got in rows:
        want = bool(ok) and P.KB < out_len <= 3 * P.KB and cap >= 1 and terms in (1, 2)
        assert got == int(want), (ok, out_len, cap, terms)
    assert sum(r[-1] for r in rows) == 4 * 2 * 2                        # (kB + 1, 22 050, 44 100, 3 kB) x caps (1, 2048) x terms (1, 2)
    (_, n_rows, nbytes), = [ln for ln in lines if ln[0] == "handoff"]
    # [rows][2] tails of 640 floats + as many flag words + the replay epoch word
    assert int(n_rows) == 512 and int(nbytes) == 512 * 2 * 640 * 4 + 512 * 2 * 4 + 4
