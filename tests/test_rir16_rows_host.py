"""The half-precision time-domain RIR rows under the fused row kernels of 2 or 3 partition blocks, on the host-compiled kernels
(tests/rir16_rows_host.cpp on the host-sim fibers), and the route of a context bound by ss_ctx_set_rir_bank16_rows
(tests/route_rir16_rows_host.cpp).

A/B: k_obs_blocks<false, false, false, false, ROWS16> and k_obs_rows<false, false, false, false, false, ROWS16> against the fp32
time-domain instantiations of the same templates fed float(q) * scale, on identical parameters.  Bound 2e-6 of the reference's
peak (the project's A/B bound: each fp32 path is held to <= 1e-6 of peak against float64 and the inputs are identical); 0.0 is
what the construction gives (the dequantised sample is exact in fp32, everything behind the load is the same instructions).
Silent units and units on the empty entry are bit-exact +0.

Model: the live units against the float64 convolution of the dequantised rows (rir16_ref.model_audiogoal, WITH the quantiser),
<= 1e-4 of peak (the project's parity budget) on the waveform and the pooled spectrogram.

k_obs_blocks against k_obs_rows on the same inputs: the same arithmetic per output sample and pooled column - equal to the A/B
bound.  Measured: 0.0 at two blocks; 1.9e-7 (waveform) / 1.2e-7 (spectrogram) at three blocks with a distractor term, where one
kernel sums the block spectra in registers and the other reads them back from its stash in another order, as the fp32 pair does.

Banks, sources, plan and model are those of tests/test_rir16_host.py (imported, never written to): two blocks = 20 000-sample rows
over the 16 000-capacity bank (16 000 / 0 / 9 000 / 15 999 taps, the ears of entry 2 a factor 2^35 apart); three blocks =
44 100-sample rows over the 40 000-capacity bank (40 000 / 16 385 taps), t0 on the steady branch of the 3-s clip so that every
RIR block has a window.  Every output is pre-filled with NaN, the stash too."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
import test_rir16_host as T
hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = T.BOUND
BUDGET = T.BUDGET
WAVE, SGRAM, BOTH, MEL, MEL_SGRAM = range(5)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("rir16_rows", tmp_path_factory.mktemp("rir16_rows"))
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hs_obs_rows_rir16_ab.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    return lib


@pytest.fixture(scope="module")
def banks():
    return T.make_banks()


# live | silent | the empty entry | the entry whose ears are 2^35 apart | the odd length | a distractor of another entry
UNITS2 = [dict(sound=0, t0=0, rir=0), dict(rir=-1), dict(sound=1, t0=0, rir=1), dict(sound=1, t0=0, rir=2),
          dict(sound=0, t0=0, rir=3), dict(sound=0, t0=0, rir=3, dis_sound=1, dis_rir=2)]
LIVE2, ZERO2 = [0, 3, 4, 5], [1, 2]


def units3(sr):
    """three-block rows: the 3-s clip on its steady branch | a distractor of another entry | silent"""
    t0 = P.window_start_sim(3 * sr, sr, 2)
    return [dict(sound=2, t0=t0, rir=0), dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=0), dict(rir=-1)]


LIVE3, ZERO3 = [0, 1], [2]


def run(lib, b, sr, units, *, blocks, halves=(1, 0), n_valid=None, parts_log2=0, wgs=8, no_distractor=False, want_wave=True):
    """the ROWS16 instantiation (1) and / or the fp32 one over the dequantised rows (0) -> {name: [outputs in `halves` order]}"""
    n_valid = sr if n_valid is None else n_valid
    srcs = T.sources(sr)
    wd, desc = T.plan(srcs, units, b["cap"], n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    n = len(units)
    t4 = P.spectrogram_shape(sr)[1]
    res = {}
    for half in halves:
        wave = np.full((n, 2, sr), np.nan, np.float32) if want_wave else None
        sg = np.full((n, 65, t4, 2), np.nan, np.float32)
        bankp = b["q"].ctypes.data if half else b["deq"].ctypes.data
        rc = lib.hs_obs_rows_rir16_ab(half, int(blocks), spec.ctypes.data, bankp, b["s"].ctypes.data if half else None,
                                      b["lens"].ctypes.data, desc.ctypes.data, wave.ctypes.data if want_wave else None, sg.ctypes.data,
                                      n, b["cap"], n_valid, sr, 0, wgs, parts_log2, int(no_distractor))
        assert rc == 0, rc
        for name, a in (("wave", wave), ("sgram", sg)):
            if a is not None:
                assert not np.isnan(a).any(), (name, half)
                res.setdefault(name, []).append(a)
    return res


def check(res, label, live, zero, ref=None):
    """A/B bound on every output, bit-exact +0 where named, and - given the model's waveform - the model bound on the live units"""
    for name, (h, f) in res.items():
        peak = np.abs(f).max()
        err = np.abs(h.astype(np.float64) - f.astype(np.float64)).max() / peak
        print(f"[rir16_rows_host] {label} {name}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        assert err <= BOUND, (label, name, err)
        assert peak > 0 and all(np.abs(f[k]).max() > 0 for k in live), (label, name)
        for k in zero:
            assert not h[k].view(np.uint32).any(), (label, name, k)     # bit-exact +0
    if ref is not None:
        for k in live:
            if "wave" in res:
                err = O.relerr(res["wave"][0][k], ref[k])
                print(f"[rir16_rows_host] {label} unit {k} wave: half kernel vs quantised float64 model = {err:.3e}")
                assert err <= BUDGET, (label, k, err)
            err = O.relerr(res["sgram"][0][k], R.model_spectrogram(ref[k]))
            print(f"[rir16_rows_host] {label} unit {k} sgram: half kernel vs quantised float64 model = {err:.3e}")
            assert err <= BUDGET, (label, k, err)


_MODELS = {}


def model_of(b, name, sr, units, n_valid=None, no_distractor=False):
    """the quantised float64 model of a unit list, computed once per (bank, rate, n_valid, flag) and shared"""
    key = (name, sr, n_valid, no_distractor)
    if key not in _MODELS:
        us = [{k: v for k, v in u.items() if not k.startswith("dis_")} for u in units] if no_distractor else units
        m = T.model(T.sources(sr), b, us, sr, sr if n_valid is None else n_valid)
        m.setflags(write=False)
        _MODELS[key] = m
    return _MODELS[key]


# ---- k_obs_rows ---------------------------------------------------------------------------------------------------------------
def test_obs_rows_two_blocks_two_workgroups(lib, banks):
    """20 000-sample rows over the 9 000-tap bank, every kind of unit; 2 persistent workgroups walk the 12 rows (row loop, the
    stash reused from row to row)"""
    b = banks["small"]
    res = run(lib, b, 20000, UNITS2, blocks=False, wgs=2)
    check(res, "rows 20000 wgs 2", LIVE2, ZERO2, ref=model_of(b, "small", 20000, UNITS2))


def test_obs_rows_three_blocks_two_workgroups(lib, banks):
    """44 100-sample rows, three RIR blocks each with a window: 2 workgroups over the 6 rows"""
    sr = 44100
    b = banks["long"]
    res = run(lib, b, sr, units3(sr), blocks=False, wgs=2)
    check(res, "rows 44100 wgs 2", LIVE3, ZERO3, ref=model_of(b, "long", sr, units3(sr)))


def test_obs_rows_split_rows(lib, banks):
    """parts_log2 = 1: two workgroups per row, each renders the row and its share of the pooled STFT blocks"""
    sr = 44100
    b = banks["long"]
    res = run(lib, b, sr, units3(sr), blocks=False, parts_log2=1)
    check(res, "rows 44100 parts 1", LIVE3, ZERO3, ref=model_of(b, "long", sr, units3(sr)))


def test_obs_rows_no_distractor(lib, banks):
    """SS_FLAG_NO_DISTRACTOR (n_terms = 1, half the stash): term 1 of the distractor unit is ignored by both forms"""
    sr = 44100
    b = banks["long"]
    res = run(lib, b, sr, units3(sr), blocks=False, no_distractor=True, wgs=3)
    check(res, "rows 44100 no-distractor", LIVE3, ZERO3, ref=model_of(b, "long", sr, units3(sr), no_distractor=True))
    both = model_of(b, "long", sr, units3(sr))
    assert np.abs(both[1] - res["wave"][0][1]).max() > 1e-3 * np.abs(both[1]).max()      # (the flag did change the unit's waveform)


def test_obs_rows_n_valid_11025_of_44100(lib, banks):
    """one rendered block (nb_y = 1 of 3), zeros behind n_valid in the waveform and in the spectrogram's dead columns"""
    sr = 44100
    b = banks["long"]
    res = run(lib, b, sr, units3(sr), blocks=False, n_valid=11025, wgs=3)
    check(res, "rows 44100 n_valid 11025", LIVE3, ZERO3, ref=model_of(b, "long", sr, units3(sr), n_valid=11025))
    assert not res["wave"][0][:, :, 11025:].view(np.uint32).any()


@pytest.mark.parametrize("sr", [20000, 44100])
def test_obs_rows_spectrogram_only(lib, banks, sr):
    """out = NULL: the waveform never leaves the workgroup"""
    b, units, live, zero = (banks["small"], UNITS2, LIVE2, ZERO2) if sr == 20000 else (banks["long"], units3(sr), LIVE3, ZERO3)
    res = run(lib, b, sr, units, blocks=False, want_wave=False, wgs=3)
    assert set(res) == {"sgram"}
    check(res, f"rows {sr} no waveform", live, zero, ref=model_of(b, "small" if sr == 20000 else "long", sr, units))


# ---- k_obs_blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_wave", [True, False], ids=["wave", "no-wave"])
@pytest.mark.parametrize("parts_log2", [0, 1])
@pytest.mark.parametrize("sr", [20000, 44100])
def test_obs_blocks(lib, banks, sr, parts_log2, want_wave):
    """one workgroup per output block (and part), ascending block order; with and without the waveform buffer"""
    b, units, live, zero = (banks["small"], UNITS2, LIVE2, ZERO2) if sr == 20000 else (banks["long"], units3(sr), LIVE3, ZERO3)
    res = run(lib, b, sr, units, blocks=True, parts_log2=parts_log2, want_wave=want_wave)
    check(res, f"blocks {sr} parts {parts_log2} wave {int(want_wave)}", live, zero,
          ref=model_of(b, "small" if sr == 20000 else "long", sr, units))


@pytest.mark.parametrize("sr", [20000, 44100])
def test_obs_blocks_equals_obs_rows(lib, banks, sr):
    """the two ROWS16 kernels share the arithmetic per output sample and per pooled column"""
    b, units = (banks["small"], UNITS2) if sr == 20000 else (banks["long"], units3(sr))
    blk = run(lib, b, sr, units, blocks=True, halves=(1,), parts_log2=1)
    row = run(lib, b, sr, units, blocks=False, halves=(1,), wgs=2)
    for name in ("wave", "sgram"):
        x, y = blk[name][0], row[name][0]
        err = np.abs(x.astype(np.float64) - y.astype(np.float64)).max() / np.abs(y).max()
        print(f"[rir16_rows_host] {sr} {name}: max |k_obs_blocks - k_obs_rows| / peak = {err:.3e}")
        assert err <= BOUND, (sr, name, err)


# ---- route --------------------------------------------------------------------------------------------------------------------
def _build_route(tmp_path_factory, name):
    """a stand-alone host program, built with the sanitizers as the other route programs are"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, name + ".cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def route_prog(tmp_path_factory):
    return _build_route(tmp_path_factory, "route_rir16_rows_host")


@pytest.fixture(scope="module")
def route_rir16_prog(tmp_path_factory):
    return _build_route(tmp_path_factory, "route_rir16_host")


def _run(prog, mode):
    r = subprocess.run([prog, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def test_route_fields_clear_print_the_recorded_table(route_prog):
    with open(os.path.join(HERE, "golden", "route_table.txt")) as f:
        golden = [ln for ln in f.read().splitlines() if not ln.startswith("#")]
    table = _run(route_prog, "table")
    assert len(golden) == 10 * 9 * 3 * 4 + 10 * 4 * 3 * 4 and table == golden      # (the fixed grid + the n_valid seam rows)


def test_route_of_a_plain_half_rows_binding_is_unchanged(route_prog, route_rir16_prog):
    """rows16 alone: what tests/route_rir16_host.cpp prints (two launches for every longer row)"""
    lines = _run(route_prog, "rows16")
    assert len(lines) == 9 * 3 * 4 * 5 * 2 * 3 and lines == _run(route_rir16_prog, "rows16")
    assert not any(ln.split()[-1][0] == "R" for ln in lines)


SHAPES_FULL = {(44100, 44100), (16385, 16385), (48000, 48000)}
SHAPES_ONE_BLOCK_RENDERED = {(44100, 11025), (48000, 12000)}
SHAPES_TOO_LONG = {(49153, 49153)}
WANT_ROWS = {
    WAVE: ("C0", "C0", "C0"),
    SGRAM: ("R0", "R0", "T4"),
    BOTH: ("R0", "T0", "T0"),
    MEL: ("C2", "C2", "C2"),
    MEL_SGRAM: ("R2", "T2", "T2"),
}


def test_route_of_a_half_rows_bank_bound_for_the_row_kernels(route_prog):
    lines = _run(route_prog, "rows16_rows")
    assert len(lines) == 9 * 3 * 4 * 5 * 2 * 3
    seen, shapes = set(), set()
    for ln in lines:
        out_len, n_valid, depth, flags, w, n, pol, code = ln.split()
        out_len, n_valid, flags, w = int(out_len), int(n_valid), int(flags), int(w)
        if flags & 2:                                                    # a cross-fade: refused, whatever is asked for
            assert code == "-8", ln
            continue
        shapes.add((out_len, n_valid))
        if out_len <= T.KB_ROWS and (1 + out_len // 160 + 3) // 4 <= 26:     # one-block shapes: as the plain binding
            want = {WAVE: "C0", SGRAM: "F0", BOTH: "F0", MEL: "C2", MEL_SGRAM: "F2"}[w]
        else:
            col = 0 if (out_len, n_valid) in SHAPES_FULL else 1 if (out_len, n_valid) in SHAPES_ONE_BLOCK_RENDERED else 2
            assert col < 2 or (out_len, n_valid) in SHAPES_TOO_LONG, ln
            want = WANT_ROWS[w][col]
        assert code == want, ln
        seen.add(code)
    assert SHAPES_FULL | SHAPES_ONE_BLOCK_RENDERED | SHAPES_TOO_LONG <= shapes
    assert {"R0", "R2"} <= seen and "W0" not in seen
    assert seen == {"C0", "C2", "F0", "F2", "R0", "R2", "T0", "T2", "T4"}
