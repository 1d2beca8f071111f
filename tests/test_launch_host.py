"""The launch geometry (csrc/ss_launch.hpp) on its own, without HIP: tests/launch_host.cpp - a stand-alone program that prints the
plan of every launcher (the convolution launches of every bank form, k_obs_blocks, k_obs_rows, the feature kernels, the shape
fields of ConvParams) over a fixed grid of the smallest values at which each rule flips - is built with AddressSanitizer and
UBSan and run directly.  Its output is compared with tests/golden/launch_table.txt, recorded when the arithmetic moved into the
header verbatim from the launchers of ss_hip.hip; and every plan is checked against the properties a plan must have."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KB, SPEC_COMPLEX, TAIL_FLOATS = 16384, 16384, 640


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("launch") / "launch_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "launch_host.cpp"), "-o", out])
    return out


def _run(program, *args):
    r = subprocess.run([program] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def table(program):
    return _run(program)


def _golden(name="launch_table.txt"):
    with open(os.path.join(HERE, "golden", name)) as f:
        return [ln for ln in f.read().splitlines() if not ln.startswith("#")]


def test_every_log_mel_plan_is_the_recorded_one(program):
    """plan_conv_mel over every bank form, flags, one RIR block and beyond, one and two buckets, the SoundSpaces 2.0 shapes and the
    cross-fade ramp at its limits: tests/golden/launch_mel_table.txt, recorded from the inline rules of the five log-mel launchers
    (and the tail of render()) of ss_hip.hip before they became this plan."""
    got, golden = _run(program, "mel"), _golden("launch_mel_table.txt")
    assert got == golden, [(a, b) for a, b in zip(golden, got) if a != b][:3]
    assert len(got) == 30 and not any("?" in ln for ln in got)
    plans = [p for ln in got for p in _plans(ln)[1]]
    assert {p[0] for p in plans} == set("SLXWYE")                  # every variant and the refusal occur
    assert all(p == ["E"] or (p[1] in "01" and int(p[2]) in (2, 10, 514)) for p in plans)


UNITS = [1, 2, 5, 16, 32, 33, 64, 128, 129, 256, 257]
FLAGS5 = [0, 1, 2, 3, 1 | 8]                                # (8: SS_FLAG_FIRST_BUCKET)


def _plans(ln):
    head, tail = ln.split(" |")
    out = []
    for tok in tail.split():
        plan, _, n = tok.partition("*")
        out += [plan.split("/")] * int(n or 1)
    return head.split(), out


def _cases(lines, kind):
    """-> (inputs, plan fields, line) of every case of `kind` (conv, blocks, rows, frames, features): a line's plans in the order
    of the loops tests/launch_host.cpp names"""
    for ln in lines:
        key, plans = _plans(ln) if " |" in ln else ([""], [])
        k, args = key[0], key[1:]
        if kind == "conv" and k == "conv-shape":
            form, fuse, out_len, n_valid = args
            grid = [(form, fuse, out_len, n_valid, f, 1, 1, 5, 256, 1, -1) for f in FLAGS5]
        elif kind == "conv" and k == "conv-units":
            form, fuse, n_cus, share, forced = args
            grid = [(form, fuse, 16000, 16000, f, 1, 1, u, n_cus, share, forced) for u in UNITS for f in (0, 1) for _ in (0, 1)]
        elif kind == "conv" and k == "conv-depth":
            form, fuse, depth = args
            grid = [(form, fuse, 16000, 16000, f, depth, b, 5, 256, 1, -1) for b in (1, 2) for f in FLAGS5]
        elif kind == "blocks" and k == "blocks":
            out_len, n_valid, n_cus, share = args
            grid = [(out_len, n_valid, f, u, n_cus, share) for f in range(4) for u in UNITS]
        elif kind == "rows" and k == "rows":
            spectral, out_len, n_valid, flags, n_cus = args
            grid = [(spectral, out_len, n_valid, flags, 3, 1, u, n_cus, sh, fo) for u in UNITS for sh, fo in ((1, -1), (2, -1), (1, 2))]
        elif kind == "rows" and k == "rows-depth":
            spectral, depth = args
            grid = [(spectral, 44100, 44100, f, depth, b, 5, 256, 1, -1) for b in (1, 2) for f in range(4)]
        elif kind == k and k in ("frames", "features"):
            grid = [tuple(args)] * len(plans)
        else:
            continue
        assert len(grid) == len(plans), ln
        for inputs, plan in zip(grid, plans):
            yield tuple(str(x) for x in inputs), plan, ln


def test_every_plan_of_the_grid_is_the_recorded_one(table):
    golden = _golden()
    diff = [(a, b) for a, b in zip(golden, table) if a != b]
    assert len(table) == len(golden) and not diff, diff[:5]
    assert "blocks-off 0 0 0" in table and "rows-refused 1 1 0" in table


def test_a_refused_plan_carries_nothing_else(table):
    """rc != 0: the program prints E and reads no other field (the caller pattern of ss_hip.hip and hostsim.cpp)"""
    n = 0
    for kind in ("conv", "rows"):
        for _, plan, ln in _cases(table, kind):
            if plan[0] == "E":
                assert plan == ["E"], ln
                n += 1
    assert n > 100
    # what is refused: more than three output blocks, a fused launch of more than one, a cross-fade on anything but fp32 rows
    # or with a ramp the kernels cannot keep (and in k_obs_rows on spectra or without its second term)
    for (form, fuse, out_len, n_valid, flags, *_), plan, ln in _cases(table, "conv"):
        nb_y = max(1, -(-int(n_valid) // KB))
        wide = plan[0] in "WY"
        fade = int(0.05 * int(out_len))                    # (the ramp the cross-fade kernels keep: 2 kPrevPairs - 2 samples)
        refused = nb_y > 3 or (int(fuse) and nb_y != 1 and not wide) or (int(flags) & 2 and (form != "rows" or not 1 <= fade <= 2414))
        assert (plan[0] == "E") == bool(refused), ln
    for (spectral, _, _, flags, *_), plan, ln in _cases(table, "rows"):
        assert (plan[0] == "E") == bool(int(flags) & 2 and (int(spectral) or int(flags) & 1)), ln


def test_every_grid_is_at_least_one_workgroup(table):
    n = 0
    for _, plan, ln in _cases(table, "conv"):
        if plan[0] != "E":
            assert int(plan[3]) >= 1 and int(plan[4]) >= 1 and 0 <= int(plan[5]) <= 3 and 1 <= int(plan[6]) <= 3, ln
            n += 1
    for _, plan, ln in _cases(table, "blocks"):
        if plan[0] != "-":
            assert int(plan[2]) >= 1, ln
            n += 1
    for _, plan, ln in _cases(table, "rows"):
        if plan[0] != "E":
            assert int(plan[1]) >= 1, ln
            n += 1
    for kind in ("frames", "features"):
        for _, plan, ln in _cases(table, kind):
            assert int(plan[-1]) >= 1, ln
            n += 1
    assert n > 5000


def test_the_stash_is_what_the_grid_indexes(table):
    """stash_bytes = grid x stash_terms x stash_nbh block spectra of kSpecComplex complex values; none on a spectral bank"""
    seen = 0
    for (spectral, *_), plan, ln in _cases(table, "rows"):
        if plan[0] == "E":
            continue
        parts, grid, nb_y, n_terms, nbh, terms, nbytes = map(int, plan)
        assert nbytes == grid * terms * nbh * SPEC_COMPLEX * 8, ln
        assert (nbytes == 0) == bool(int(spectral)) and (int(spectral) or terms == n_terms), ln
        seen += nbytes > 0
    assert seen > 1000


def test_an_obs_blocks_launch_fits_its_share_of_the_chip(table):
    """rows * nb << k <= n_cus / share: one workgroup per CU is what makes the hand-off between workgroups safe"""
    ok = 0
    for (out_len, n_valid, flags, n_units, n_cus, share), plan, ln in _cases(table, "blocks"):
        rows, nb = 2 * int(n_units), -(-int(out_len) // KB)
        budget = int(n_cus) // int(share)
        fits = not int(flags) & 2 and n_valid == out_len and 2 <= nb <= 3 and rows * nb <= budget
        assert (plan[0] != "-") == fits, ln
        if plan[0] == "-":
            continue
        k, p_nb, grid, n_terms, floats, words = map(int, plan)
        assert p_nb == nb and grid == (rows * nb) << k and grid <= budget, ln
        assert k == 3 or (rows * nb) << (k + 1) > budget, ln           # the spare CUs are used
        assert floats == rows * 2 * TAIL_FLOATS and words == rows * 2 and n_terms == (1 if int(flags) & 1 else 2), ln
        ok += 1
    assert ok > 20
