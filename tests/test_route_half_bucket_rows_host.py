"""The route of a step on a context bound by ss_ctx_set_rir_spec_buckets_rows (csrc/ss_route.hpp, Bank::spec_buckets_half_rows), on
its own, without HIP: tests/route_half_bucket_rows_host.cpp, built with AddressSanitizer and UBSan and run directly.

With the field set, at 44 100 / 48 000: spectrogram steps take the rows chain from the spectra, log-mel steps inside
ss_ctx_set_logmel_buckets_policy's range the log-mel form of the row kernels, outside it the waveform scratch, waveform-only steps
the convolution, and a cross-fade is refused.  With the field clear the program prints the grid of tests/route_host.cpp: it equals
tests/golden/route_table.txt, line for line."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KB = 16384
SPECTRAL, SCRATCH, HANDOVER, REFUSED = 1, 2, 4, 8
# wants: waveform only, spectrogram only, both, log-mel only, log-mel + spectrogram
WAVE, SGRAM, BOTH, MEL, MEL_SGRAM = range(5)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("route_hbr") / "route_half_bucket_rows_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "route_half_bucket_rows_host.cpp"), "-o", out])
    return out


def _run(prog, mode):
    r = subprocess.run([prog, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def test_field_clear_prints_the_recorded_table(prog):
    with open(os.path.join(HERE, "golden", "route_table.txt")) as f:
        golden = [ln for ln in f.read().splitlines() if not ln.startswith("#")]
    table = _run(prog, "table")
    assert len(golden) == 10 * 9 * 3 * 4 + 10 * 4 * 3 * 4 and table == golden      # (the fixed grid + the n_valid seam rows)


def test_routes_with_the_field_set(prog):
    lines = _run(prog, "rows")
    assert len(lines) == 4 * 3 * 4 * 5 * 2 * 2
    seen = set()
    for ln in lines:
        out_len, n_valid, depth, flags, w, n, pol, code = ln.split()
        out_len, n_valid, depth, flags, w, n, pol = (int(x) for x in (out_len, n_valid, depth, flags, w, n, pol))
        launch, bits = code[0], int(code[1], 16)
        assert out_len in (44100, 48000) and depth in (1, 5, 16)
        if flags & 2:                                                    # a cross-fade has no rows to read: refused
            assert code == "-8", ln
            continue
        assert bits & SPECTRAL and not bits & REFUSED, ln                # every launch reads the spectra
        full = n_valid == out_len
        in_policy = pol == 1 and n <= 100
        if w == WAVE:
            assert code == "C1", ln
        elif w in (SGRAM, BOTH):
            # the rows chain; a step of one rendered block with a waveform buffer (the caller's, or the hand-over one) goes to the
            # convolution + k_spectrogram, as on every spectral bank
            assert code == ("R1" if full else ("T5" if w == SGRAM else "T1")), ln
        elif in_policy:
            assert code == "r1", ln                                      # the log-mel form of the row kernels (kMelRows)
        else:                                                            # outside the policy: the waveform scratch
            assert bits == SPECTRAL | SCRATCH, ln
            assert launch == ("C" if w == MEL else ("R" if full else "T")), ln
        seen.add((w, launch))
    assert seen >= {(WAVE, "C"), (SGRAM, "R"), (BOTH, "R"), (MEL, "r"), (MEL_SGRAM, "r"), (MEL, "C"), (MEL_SGRAM, "R")}
