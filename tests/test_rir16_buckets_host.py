"""Half-precision time-domain rows in length buckets on the host-compiled loop kernel (tests/rir16_buckets_host.cpp on the
host-sim fibers), the route of a context bound to such a bank and the launch plan of its convolution.

Scene: tests/spec_buckets_ref.py - four buckets of 16 000 / 20 000 / 40 000 / 70 000 samples (1 / 2 / 3 / 5 partition blocks), one
launch of 12 units over the first and last entry of each, full-capacity entries followed by a neighbour, a 9000-tap entry in the
5-block bucket, a two-bucket distractor unit, an empty entry, a silent unit and entries scaled by 32 768 and 1e-6.  Each bucket is
quantised by tests/rir16_ref.quantise.  Half rows are NOT padded to whole partition blocks (20 000, 40 000 and 70 000 are no
multiples of 16 384): a row stride or load bound taken from another bucket reads the neighbour's halves.

A/B: k_conv<.., HALF, RBK> against the fp32 bucketed k_conv fed float(q) * scale - unfused at out_len 16 000 and 44 100 (three
output blocks), fused at 16 000 (waveform and pooled spectrogram).  Bound 2e-6 of the reference's peak, the project's A/B bound
(tests/test_spec_half_host.py): each fp32 path is held to <= 1e-6 of peak against float64 and the inputs are identical.
Model: units 1, 3, 4, 6, 7, 8 and 9 against the float64 convolution of the bank's own halves and scales
(tests/rir16_ref.model_audiogoal), 1e-4, the project's parity budget; a row read from the wrong bucket is ~1e-1.
Bucket-0 launches (SS_FLAG_FIRST_BUCKET, through the unit table and through the descriptors) are bit-identical to the
single-allocation half launch on bucket 0's arrays."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
import spec_buckets_ref as B

hs = pytest.importorskip("hostsim.hs")

from test_spec_half_host import _plan  # noqa: E402  (the planner of the half-bank host test)

HERE = os.path.dirname(os.path.abspath(__file__))
SR = B.SR
BOUND = 2e-6
BUDGET = 1e-4
MODEL_UNITS = (1, 3, 4, 6, 7, 8, 9)      # every bucket, both scaled entries, the 9000-tap entry, the two-bucket unit


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("rir16_buckets", tmp_path_factory.mktemp("rir16_buckets"))
    L = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.hs_conv_rir16_buckets.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci]
    L.hs_source_windows.argtypes = [vp, vp, vp, ci]
    return L


@pytest.fixture(scope="module")
def world():
    """the scene, per bucket its halves, scales and dequantised rows"""
    sc = B.scene()
    qs = [R.quantise(rows) for rows in sc["rows"]]
    sc["q"] = [np.ascontiguousarray(q) for q, _ in qs]
    sc["s"] = [np.ascontiguousarray(s, np.float32) for _, s in qs]
    sc["deq"] = [np.ascontiguousarray(R.dequantise(q, s)) for q, s in qs]
    assert all(q.dtype == np.float16 and q.shape == rows.shape for q, rows in zip(sc["q"], sc["rows"]))
    # the scale of a wrong bucket or entry cannot hide inside a tolerance: the scaled entries' scales are far from every other
    # (the empty entry aside: its scale is 1 and every one of its halves is +0)
    big, small = sc["s"][0][B.BIG - B.FIRST[0]], sc["s"][2][B.SMALL - B.FIRST[2]]
    plain = np.concatenate([sc["s"][B.bucket_of(g)][g - B.FIRST[B.bucket_of(g)]] for g in range(len(sc["lens"]))
                            if g not in (B.BIG, B.SMALL, B.EMPTY)])
    assert big.min() >= 2.0 ** 10 * plain.max() and small.max() <= 2.0 ** -10 * plain.min()
    return sc


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _run(lib, sc, form, fuse, out_len, n_valid, units=None, bucket0=0, n_buckets=4):
    """form: 'half' | 'deq' (the fp32 bucketed kernel on the dequantised rows) -> (waveform, pooled spectrogram or None);
    n_buckets = 1: the single-allocation launch on bucket 0's arrays"""
    srcs = sc["srcs"]
    units = sc["units"] if units is None else units
    wd, desc = _plan(srcs, units, max(B.CAPS[:n_buckets]), n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    n = len(units)
    wave = np.full((n, 2, out_len), np.nan, np.float32)
    sg = np.full((n,) + P.spectrogram_shape(out_len), np.nan, np.float32) if fuse else None
    bank = _ptrs((sc["q"] if form == "half" else sc["deq"])[:n_buckets])
    scales = _ptrs(sc["s"][:n_buckets]) if form == "half" else None
    first, caps = np.asarray(B.FIRST, np.int32), np.asarray(B.CAPS, np.int32)
    rc = lib.hs_conv_rir16_buckets(int(form == "half"), int(fuse), bucket0, spec.ctypes.data, bank, scales, first.ctypes.data,
                                   caps.ctypes.data, n_buckets, sc["lens"].ctypes.data, desc.ctypes.data, wave.ctypes.data,
                                   sg.ctypes.data if fuse else None, n, n_valid, out_len, 0)
    assert rc == 0, rc
    assert not np.isnan(wave).any() and (sg is None or not np.isnan(sg).any()), form
    return wave, sg


def _ab(got, ref, label):
    peak = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / peak
    print(f"[rir16_buckets_host] {label}: max |half - fp32(dequantised)| / peak = {err:.3e}")
    assert peak > 0 and err <= BOUND, (label, err)


def _zeros_and_live(wave, sg, units):
    for n, u in enumerate(units):
        dead = u.get("rir", -1) < 0 or u["rir"] == B.EMPTY
        if dead:                                                       # the empty entry and the silent unit: bit-exact +0
            assert not wave[n].view(np.uint32).any(), n
            assert sg is None or not sg[n].view(np.uint32).any(), n
        else:
            assert wave[n].any() and (sg is None or sg[n].any()), n


def _model(sc, u, out_len, n_valid=None):
    """float64 convolution of unit u with the halves and scales the bank holds (both terms of a distractor unit)"""
    out = np.zeros((2, out_len))
    for snd, t0, g in [(u["sound"], u["t0"], u["rir"])] + ([(u["dis_sound"], 0, u["dis_rir"])] if u.get("dis_rir", -1) >= 0 else []):
        b = B.bucket_of(g)
        row = sc["deq"][b][g - B.FIRST[b]][:, :int(sc["lens"][g])]
        out += R.model_audiogoal(sc["srcs"][snd], row, t0, out_len, quant=False, n_valid=n_valid)
    return out


@pytest.fixture(scope="module")
def models(world):
    """the float64 model waveforms, computed once per (unit, out_len)"""
    cache = {}

    def get(n, out_len):
        if (n, out_len) not in cache:
            cache[(n, out_len)] = _model(world, world["units"][n], out_len)
        return cache[(n, out_len)]
    return get


@pytest.mark.parametrize("out_len,fuse", [(16000, False), (44100, False), (16000, True)],
                         ids=["unfused-16000", "unfused-44100-three-output-blocks", "fused-16000"])
def test_half_row_buckets_equal_fp32_buckets_fed_dequantised_rows(lib, world, models, out_len, fuse):
    half_w, half_s = _run(lib, world, "half", fuse, out_len, out_len)
    ref_w, ref_s = _run(lib, world, "deq", fuse, out_len, out_len)
    label = f"{'fused' if fuse else 'unfused'} out_len {out_len}"
    _ab(half_w, ref_w, label + " waveform")
    if fuse:
        _ab(half_s, ref_s, label + " spectrogram")
    _zeros_and_live(half_w, half_s, world["units"])
    for n in MODEL_UNITS:
        err = O.relerr(half_w[n], models(n, out_len))
        print(f"[rir16_buckets_host] {label} unit {n}: half kernel vs float64 model fed the bank's halves = {err:.3e}")
        assert err <= BUDGET, (n, err)


@pytest.mark.parametrize("fuse", [False, True], ids=["unfused", "fused"])
def test_first_bucket_launch_is_the_single_allocation_half_launch_bit_for_bit(lib, world, fuse):
    units = [dict(sound=0, t0=0, rir=0), dict(sound=1, t0=0, rir=2), dict(sound=0, t0=0, rir=B.EMPTY), dict(rir=-1),
             dict(sound=1, t0=4000, rir=0)]
    one_w, one_s = _run(lib, world, "half", fuse, SR, SR, units=units, bucket0=1, n_buckets=1)      # the existing loop-free launch
    loop_w, loop_s = _run(lib, world, "half", fuse, SR, SR, units=units, bucket0=0)                 # the bucketed loop kernel
    for mode, name in ((1, "descriptors"), (2, "unit table")):
        w, s = _run(lib, world, "half", fuse, SR, SR, units=units, bucket0=mode)
        assert w.tobytes() == one_w.tobytes(), name
        if fuse:
            assert s.tobytes() == one_s.tobytes(), name
        _zeros_and_live(w, s, units)
        _ab(w, loop_w, f"first bucket ({name}) against the bucketed loop kernel, waveform")
        if fuse:
            _ab(s, loop_s, f"first bucket ({name}) against the bucketed loop kernel, spectrogram")


def test_n_valid_4000_of_16000_fused(lib, world):
    n_valid = 4000
    half_w, half_s = _run(lib, world, "half", True, SR, n_valid)
    ref_w, ref_s = _run(lib, world, "deq", True, SR, n_valid)
    _ab(half_w, ref_w, "n_valid 4000 waveform")
    _ab(half_s, ref_s, "n_valid 4000 spectrogram")
    assert not half_w[:, :, n_valid:].view(np.uint32).any()            # samples at and beyond n_valid: zero
    for n in MODEL_UNITS:
        ref = _model(world, world["units"][n], SR, n_valid=n_valid)
        err = O.relerr(half_w[n], ref)
        print(f"[rir16_buckets_host] n_valid 4000 unit {n}: half kernel vs float64 model = {err:.3e}")
        assert err <= BUDGET, (n, err)


# ---- route and launch plan ----------------------------------------------------------------------------------------------------
WAVE, SGRAM, BOTH, MEL, MEL_SGRAM = range(5)
KB = 16384
FIRST_BUCKET = 4


def _build(tmp_path_factory, name):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, name + ".cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def route_prog(tmp_path_factory):
    return _build(tmp_path_factory, "route_rir16_buckets_host")


@pytest.fixture(scope="module")
def launch_prog(tmp_path_factory):
    return _build(tmp_path_factory, "launch_rir16_buckets_host")


def _lines(prog, mode):
    r = subprocess.run([prog, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return [ln for ln in f.read().splitlines() if not ln.startswith("#")]


def test_route_field_clear_prints_the_recorded_table(route_prog):
    golden = _golden("route_table.txt")
    assert len(golden) == 10 * 9 * 3 * 4 + 10 * 4 * 3 * 4 and _lines(route_prog, "table") == golden


def test_launch_program_prints_the_recorded_table(launch_prog):
    assert _lines(launch_prog, "table") == _golden("launch_table.txt")


def test_route_of_half_rows_in_length_buckets(route_prog):
    lines = _lines(route_prog, "rows16bk")
    assert len(lines) == 9 * 3 * 8 * 5 * 2 * 3
    seen = set()
    for ln in lines:
        out_len, n_valid, depth, flags, w, n, pol, code = ln.split()
        out_len, flags, w = int(out_len), int(flags), int(w)
        if flags & 2:                                                    # a cross-fade: refused, whatever is asked for
            assert code == "-8", ln
            continue
        fused = out_len <= KB and (1 + out_len // 160 + 3) // 4 <= 26
        if w == WAVE:
            want = "C0"
        elif w == SGRAM:
            want = "F0" if fused else "T4"                               # no waveform buffer: the context's hand-over buffer
        elif w == BOTH:
            want = "F0" if fused else "T0"
        elif w == MEL:
            want = "C2"                                                  # log-mel: always the waveform scratch
        else:
            want = "F2" if fused else "T2"
        assert code == want, ln                                          # (never R: the row kernels do not read bucketed half rows)
        seen.add(code)
    assert seen == {"C0", "F0", "T4", "T0", "C2", "F2", "T2"}
    assert lines == _golden("route_rir16_buckets_table.txt")


def test_launch_plan_of_half_rows_in_length_buckets(launch_prog):
    lines = _lines(launch_prog, "rows16bk")
    assert lines == _golden("launch_rir16_buckets_table.txt")
    n_seen = 0
    for ln in lines:
        key, plans = ln.split(" | ")
        _, fuse, depth, n_buckets, out_len, n_valid = key.split()
        fuse, depth, n_buckets, out_len, n_valid = int(fuse), int(depth), int(n_buckets), int(out_len), int(n_valid)
        flat = []
        for tok in plans.split():
            plan, _, rep = tok.partition("*")
            flat += [plan] * int(rep or 1)
        assert len(flat) == 5 * 3
        nb_y = -(-n_valid // KB)
        for k, plan in enumerate(flat):
            flags = (0, 1, 2, 3, 1 | FIRST_BUCKET)[k // 3]
            if flags & 2 or (fuse and nb_y != 1):                        # a cross-fade; a fused launch of more than one block
                assert plan == "E", ln
                continue
            variant, tab, bucket0 = plan.split("/")[:3]
            assert int(bucket0) == int(n_buckets == 1 or bool(flags & FIRST_BUCKET)), ln
            simple = bool(flags & 1) and nb_y == 1 and depth == 1 and bool(int(bucket0))
            assert variant == ("S" if simple else "L") and int(tab) == int(simple), ln      # never P: no persistent variant
            n_seen += 1
    assert n_seen > 0
