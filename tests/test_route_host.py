"""The routing of a context's step (csrc/ss_route.hpp) on its own, without HIP: tests/route_host.cpp - a stand-alone program that
prints the Route of every case of a fixed grid (ten bank forms x nine (out_len, n_valid) x 1 / 3 / 17 RIR blocks x the planner's
flags x five sets of wanted outputs x n in {1, 200} x three policy sets; appended to it: three-block rows with n_valid on the
block seam, kB and kB + 1, at 44 100 and 48 000), built with AddressSanitizer and UBSan and run directly.  Its output is
compared with tests/golden/route_table.txt, whose fixed grid was recorded from the verbatim extraction of the expressions
ss_ctx_observe used to carry inline, before anything in them was simplified (the appended seam rows: from ss_route.hpp as it
stands); and every route is checked against the properties a route must have."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KB = 16384
GRID, SEAMS = 10 * 9 * 3 * 4, 10 * 4 * 3 * 4               # lines of the fixed grid, of the appended seam rows
SPECTRAL, SCRATCH, HANDOVER, REFUSED = 1, 2, 4, 8
LAUNCHES = "-CFWRTmsr"
SPECTRAL_ONLY = {"spec", "half", "half-rows", "specbk", "specbk-half"}
WANTS = [dict(waveform=True, spectrogram=False, mel=False), dict(waveform=False, spectrogram=True, mel=False),
         dict(waveform=True, spectrogram=True, mel=False), dict(waveform=False, spectrogram=False, mel=True),
         dict(waveform=False, spectrogram=True, mel=True)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("route") / "route_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "route_host.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _golden():
    with open(os.path.join(HERE, "golden", "route_table.txt")) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("#") and "verbatim" in lines[0]
    return [ln for ln in lines if not ln.startswith("#")]


def _cases(lines):
    """-> (bank, out_len, n_valid, blocks, flags, wants, launch, bits) of every route of the table"""
    for ln in lines:
        head, *groups = ln.split(" | ")
        bank, out_len, n_valid, blocks, flags = head.split()
        assert len(groups) == len(WANTS), ln
        for w, grp in zip(WANTS, groups):
            codes = grp.split()
            assert len(codes) in (1, 6), ln
            for code in codes * (6 if len(codes) == 1 else 1):
                assert len(code) == 2 and code[0] in LAUNCHES, ln
                yield bank, int(out_len), int(n_valid), int(blocks), int(flags), w, code[0], int(code[1], 16)


def test_every_route_of_the_grid_is_the_recorded_one(table):
    golden = _golden()
    assert len(golden) == GRID + SEAMS
    diff = [(a, b) for a, b in zip(golden, table) if a != b]
    assert len(table) == len(golden) and not diff, diff[:5]


def test_properties_of_every_route(table):
    assert table == _golden()                       # (the properties hold on the recorded table itself)
    n = 0
    for bank, out_len, n_valid, blocks, flags, w, launch, bits in _cases(table):
        n += 1
        case = (bank, out_len, n_valid, blocks, flags, w, launch, bits)
        # at most one launch family, and none exactly for the refused steps
        assert (launch == "-") == bool(bits & REFUSED), case
        # refused: spectral-only banks with a cross-fade, and only those
        assert bool(bits & REFUSED) == (bank in SPECTRAL_ONLY and bool(flags & 2)), case
        if bits & REFUSED:
            assert bits == REFUSED, case
        # the waveform scratch: log-mel-only steps, exactly those no log-mel form serves
        assert not (bits & SCRATCH) or w["mel"], case
        if w["mel"] and not bits & REFUSED:
            assert bool(bits & SCRATCH) == (launch not in "msr"), case
        # the hand-over buffer: rows longer than one block, no waveform buffer given - and then the two launches that need it
        if bits & HANDOVER:
            assert out_len > KB and not w["waveform"] and not bits & SCRATCH and launch == "T", case
        # a cross-faded step reads the time-domain rows
        assert not (bits & SPECTRAL and flags & 2), case
        # without a spectrogram nothing but the convolution (or a log-mel form) runs
        if not w["spectrogram"] and not bits & REFUSED:
            assert launch in "Cmsr", case
    assert n == (GRID + SEAMS) * 5 * 6


def test_seam_rows_switch_between_the_wide_kernel_and_the_row_kernels(table):
    """n_valid = kB is the wide kernel's last step, kB + 1 the first of k_obs_rows (plain) / of two launches (cross-faded, or
    - past 16 RIR blocks - everything), with and without a waveform buffer"""
    seams = table[GRID:]
    assert len(seams) == SEAMS and {(c[1], c[2]) for c in _cases(seams)} == {(o, v) for o in (44100, 48000) for v in (KB, KB + 1)}
    seen = set()
    for bank, out_len, n_valid, blocks, flags, w, launch, bits in _cases(seams):
        if not w["spectrogram"] or w["mel"] or bits & REFUSED:
            continue
        case = (bank, out_len, n_valid, blocks, flags, w, launch, bits)
        if n_valid == KB and not bits & SPECTRAL:
            assert launch == "W", case                   # time-domain rows: the wide kernel, buffer or not, cross-faded or not
        elif n_valid == KB:
            assert launch in "TR", case                  # no wide kernel reads spectra
        elif flags & 2 or blocks > 16:
            assert launch == "T" and bool(bits & HANDOVER) == (not w["waveform"]), case
        else:
            assert launch == "R", case
        seen.add(launch)
    assert seen == set("WRT")
