"""The half-precision time-domain RIR rows on the host-compiled kernels (tests/rir16_host.cpp on the host-sim fibers).

Producers: k_rows_half and k_scatter_rows16 against the numpy rule (tests/rir16_ref.py), bit for bit - wav staging, rows with
NaN behind their length, scattered slots, the empty entry (+0 halves, scale 1), entries not named untouched.

A/B: every k_conv<.., HALF> instantiation against the fp32 instantiation of the same template fed float(q) * scale, on identical
parameters.  Bound 2e-6 of the reference's peak (the project's A/B bound: each fp32 path is held to <= 1e-6 of peak against
float64 and the inputs are identical).  Measured: 0.0 on every case and output (the dequantised sample is exact in fp32, the
arithmetic behind the load is the same instructions) - profiles/r7/NOTES.md.

Model: the half kernels against the float64 convolution of the dequantised rows (rir16_ref.model_audiogoal), <= 1e-4 of peak (the
project's parity budget); the model's own distance to oracle.compute_audiogoal on the unquantised rows is asserted first.  The
format's loss - the quantised model against the unquantised oracle at 16 kHz and 44.1 kHz - is printed, not asserted
(INTEGRATION.md "Half-precision time-domain rows").

Route: tests/route_rir16_host.cpp - a context with a half-rows bank takes the fused launch for one-block rows, two launches for
every longer row, the waveform scratch for log-mel steps, and refuses a cross-fade; with the field clear the recorded table.

Banks: cap 16 000 with 16 000 / 0 / 9 000 / 15 999 taps, ear 0 of entry 2 scaled by 32 768 and its ear 1 by 1e-6; cap 40 000 with
40 000 / 16 385 taps, every partition block audible.  Every output is pre-filled with NaN."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

import rir16_ref as R
hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 2e-6
BUDGET = 1e-4
SPECTRAL, SCRATCH, HANDOVER, REFUSED = 1, 2, 4, 8
WAVE, SGRAM, BOTH, MEL, MEL_SGRAM = range(5)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("rir16", tmp_path_factory.mktemp("rir16"))
    lib = ctypes.CDLL(so)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.hs_rows_half.argtypes = [vp, vp, vp, ci, ll, ci, ci]
    lib.hs_scatter_rows16.argtypes = [vp, ll, vp, vp, ci, vp, vp, ci, vp]
    lib.hs_conv_rir16_ab.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci]
    lib.hs_source_windows.argtypes = [vp, vp, vp, ci]
    return lib


def make_banks():
    """the two banks of the issue as planar fp32 rows, their lengths, the numpy half form and its dequantisation"""
    rng = np.random.default_rng(16)
    small = np.zeros((4, 2, 16000), np.float32)
    for i, n in enumerate((16000, 0, 9000, 15999)):
        if n:
            small[i, :, :n] = O.synth_rir(rng, 16000, length=n, n=1)[0]
    small[2, 0] *= np.float32(32768.0)
    small[2, 1] *= np.float32(1e-6)
    long = np.zeros((2, 2, 40000), np.float32)
    long[0] = O.synth_rir_blocks(rng, 16000, 40000, n=1)[0]
    long[1, :, :16385] = O.synth_rir_blocks(rng, 16000, 16385, n=1)[0]
    out = {}
    for name, rows, lens in (("small", small, (16000, 0, 9000, 15999)), ("long", long, (40000, 16385))):
        q, s = R.quantise(rows)
        out[name] = dict(cap=rows.shape[2], rows=rows, lens=np.asarray(lens, np.int32), q=np.ascontiguousarray(q),
                         s=np.ascontiguousarray(s), deq=np.ascontiguousarray(R.dequantise(q, s)))
        for a in out[name].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def banks():
    return make_banks()


# ---- producers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "long"])
def test_rows_half_equals_the_numpy_rule(lib, banks, name):
    b = banks[name]
    n, cap = b["rows"].shape[0], b["cap"]
    q = np.full((n, 2, cap), np.nan, np.float16)
    s = np.full((n, 2), np.nan, np.float32)
    assert lib.hs_rows_half(b["rows"].ctypes.data, q.ctypes.data, s.ctypes.data, n, 2 * cap, cap, cap) == 0
    assert q.tobytes() == b["q"].tobytes() and s.tobytes() == b["s"].tobytes()
    assert np.abs(b["q"].astype(np.float32)).max() <= 32768.0           # the scaled maximum lies in [2^14, 2^15]
    if name == "small":
        assert not q[1].view(np.uint16).any() and (s[1] == 1.0).all()   # the empty entry: +0 halves, scale 1
        assert s[2, 0] / s[2, 1] > 1e9                                  # one scale per EAR: 32 768 against 1e-6


@pytest.mark.parametrize("name", ["small", "long"])
def test_scatter_rows16_equals_rows_half(lib, banks, name):
    b = banks[name]
    n, cap = b["rows"].shape[0], b["cap"]
    stride = 2 * cap + 6                                                # rows further apart than they are long
    staged = np.full((n, stride), np.nan, np.float32)                   # NaN behind every row's length and behind the row
    for i, ln in enumerate(b["lens"]):
        staged[i, :2 * ln] = b["rows"][i, :, :ln].T.reshape(-1)         # wav layout: (L, R) per frame
    slots = np.asarray([2 * i + 1 for i in range(n)], np.int32)[::-1].copy()      # scattered, out of order
    entries = int(slots.max()) + 2
    q = np.zeros((entries, 2, cap), np.float16)                         # a bank's arrays are zero-initialised
    s = np.zeros((entries, 2), np.float32)
    bank_len = np.full((entries,), -5, np.int32)
    lens_arg = b["lens"].copy()
    lens_arg[lens_arg == cap] = cap + 7                                 # a length beyond the capacity is clamped
    assert lib.hs_scatter_rows16(staged.ctypes.data, stride, slots.ctypes.data, lens_arg.ctypes.data, n, q.ctypes.data, s.ctypes.data,
                                 cap, bank_len.ctypes.data) == 0
    for i in range(n):
        assert q[slots[i]].tobytes() == b["q"][i].tobytes(), (name, i)
        assert s[slots[i]].tobytes() == b["s"][i].tobytes(), (name, i)
        assert bank_len[slots[i]] == b["lens"][i]
    others = np.setdiff1d(np.arange(entries), slots)
    assert not q[others].view(np.uint16).any() and not s[others].any() and (bank_len[others] == -5).all()


def test_row_quantiser_on_known_values():
    v = np.zeros((3, 8), np.float32)
    v[0, :3] = [1.0, -0.75, 2.0 ** -20]
    v[1, :3] = [32768.0 * 3, 2049.0 * 8, 2051.0 * 8]      # e = 17, q = v / 4: 24576, 4098 (a tie: to even 4096), 4102 (tie: 4104)
    q, s = R.quantise(v)
    assert s.tolist() == [2.0 ** -14, 4.0, 1.0]
    assert q[0, :3].astype(np.float64).tolist() == [16384.0, -12288.0, 2.0 ** -6]
    assert q[1, :3].astype(np.float64).tolist() == [24576.0, 4096.0, 4104.0]
    assert not q[2].view(np.uint16).any()
    assert np.array_equal(R.dequantise(q, s)[0, :2], v[0, :2])


# ---- consumer -----------------------------------------------------------------------------------------------------------------
_SOURCES = {}


def sources(sr):
    if sr not in _SOURCES:
        rng = np.random.default_rng(sr)
        _SOURCES[sr] = list(O.synth_sources(rng, sr, k=2, seconds=1)) + [O.synth_sources(rng, sr, k=1, seconds=3)[0]]
    return _SOURCES[sr]


def plan(srcs, units, cap, n_valid):
    """window descriptors + unit descriptors of a launch, as hostsim.hs.run plans them"""
    nbh_max = max(1, P.ceil_div(cap, P.KB))
    nby = max(1, P.ceil_div(n_valid, P.KB))
    offs = np.cumsum([0] + [len(s) for s in srcs])
    cache, rows = {}, []

    def slot_of(sound, t0):
        if (sound, t0) not in cache:
            ws = P.plan_window_set(len(srcs[sound]), t0, nbh_max, nby, False)
            cache[(sound, t0)] = (sum(len(r) for r in rows), ws)
            rows.append(P.window_desc_rows(ws, int(offs[sound]), len(srcs[sound]), False))
        return cache[(sound, t0)]

    desc = np.zeros((len(units), 8), np.int32)
    for n, u in enumerate(units):
        if u.get("rir", -1) < 0:
            desc[n] = P.unit_desc_row()
            continue
        s0, ws = slot_of(u["sound"], u["t0"])
        if u.get("dis_rir", -1) >= 0:
            d0, dws = slot_of(u["dis_sound"], 0)
            desc[n] = P.unit_desc_row(u["rir"], s0, ws, u["dis_rir"], d0, dws)
        else:
            desc[n] = P.unit_desc_row(u["rir"], s0, ws)
    wd = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), np.int32), np.int32)
    return wd, desc


def model(srcs, b, units, sr, n_valid, quant=True):
    """float64 [n, 2, sr] of rir16_ref's model: the unit's term plus its distractor's; silent units zero"""
    out = np.zeros((len(units), 2, sr), np.float64)
    for n, u in enumerate(units):
        if u.get("rir", -1) < 0:
            continue
        ln = int(b["lens"][u["rir"]])
        out[n] = R.model_audiogoal(srcs[u["sound"]], b["rows"][u["rir"], :, :ln], u["t0"], sr, quant, n_valid)
        if u.get("dis_rir", -1) >= 0:
            ln = int(b["lens"][u["dis_rir"]])
            out[n] += R.model_audiogoal(srcs[u["dis_sound"]], b["rows"][u["dis_rir"], :, :ln], 0, sr, quant, n_valid)
    return out


def ab(lib, b, sr, units, fuse, simple, use_tab=False, n_valid=None, parts_log2=0):
    """the HALF instantiation and the fp32 one over the dequantised rows -> {name: (half, fp32)} of every output"""
    n_valid = sr if n_valid is None else n_valid
    srcs = sources(sr)
    wd, desc = plan(srcs, units, b["cap"], n_valid)
    flat = np.concatenate([np.asarray(s, np.float32) for s in srcs]).astype(np.float32)
    spec = np.zeros((max(1, len(wd)), P.SPEC_FLOATS), np.float32)
    assert lib.hs_source_windows(flat.ctypes.data, wd.ctypes.data, spec.ctypes.data, len(wd)) == 0
    n = len(units)
    t4 = P.spectrogram_shape(sr)[1]
    res = {}
    for half in (1, 0):
        wave = np.full((n, 2, sr), np.nan, np.float32)
        sg = np.full((n, 65, t4, 2), np.nan, np.float32) if fuse else None
        bankp = b["q"].ctypes.data if half else b["deq"].ctypes.data
        rc = lib.hs_conv_rir16_ab(half, int(fuse), int(simple), int(use_tab), spec.ctypes.data, bankp,
                                  b["s"].ctypes.data if half else None, b["lens"].ctypes.data, desc.ctypes.data, wave.ctypes.data,
                                  sg.ctypes.data if fuse else None, n, b["cap"], n_valid, sr, 0, parts_log2)
        assert rc == 0, rc
        for name, a in (("wave", wave), ("sgram", sg)):
            if a is not None:
                assert not np.isnan(a).any(), (name, half)
                res.setdefault(name, []).append(a)
    return res


def check(res, label, live, zero=(), ref=None):
    """A/B bound on every output, exact zeros where named, and - given the model's waveform - the model bound"""
    for name, (h, f) in res.items():
        peak = np.abs(f).max()
        err = np.abs(h.astype(np.float64) - f.astype(np.float64)).max() / peak
        print(f"[rir16_host] {label} {name}: max |half - fp32(dequantised)| / peak = {err:.3e}")
        assert err <= BOUND, (label, name, err)
        assert peak > 0 and all(np.abs(f[k]).max() > 0 for k in live)
        for k in zero:
            assert not h[k].view(np.uint32).any(), (label, name, k)     # bit-exact +0
    if ref is not None:
        err = O.relerr(res["wave"][0], ref)
        print(f"[rir16_host] {label} wave: half kernel vs quantised float64 model = {err:.3e}")
        assert err <= BUDGET, (label, err)
        if "sgram" in res:
            sg_ref = np.stack([R.model_spectrogram(w) for w in ref])
            err = O.relerr(res["sgram"][0], sg_ref)
            print(f"[rir16_host] {label} sgram: half kernel vs quantised float64 model = {err:.3e}")
            assert err <= BUDGET, (label, err)


SR = 16000
# plain | silent | the empty entry | the entry whose ears are 2^35 apart | the odd length
SIMPLE_UNITS = [dict(sound=0, t0=0, rir=0), dict(rir=-1), dict(sound=1, t0=0, rir=1), dict(sound=1, t0=0, rir=2),
                dict(sound=0, t0=0, rir=3)]


@pytest.mark.parametrize("fuse", [False, True], ids=["conv", "fused"])
@pytest.mark.parametrize("use_tab", [False, True], ids=["desc", "unit_table"])
def test_half_rows_loop_free(lib, banks, fuse, use_tab):
    b = banks["small"]
    res = ab(lib, b, SR, SIMPLE_UNITS, fuse=fuse, simple=True, use_tab=use_tab)
    check(res, f"loop-free fuse={int(fuse)} tab={int(use_tab)}", live=[0, 3, 4], zero=[1, 2],
          ref=model(sources(SR), b, SIMPLE_UNITS, SR, SR))


@pytest.mark.parametrize("fuse", [False, True], ids=["conv", "fused"])
def test_half_rows_loop_with_a_distractor_of_another_entry(lib, banks, fuse):
    b = banks["small"]
    units = [dict(sound=0, t0=0, rir=3, dis_sound=1, dis_rir=2), dict(rir=-1), dict(sound=1, t0=0, rir=0)]
    res = ab(lib, b, SR, units, fuse=fuse, simple=False)
    check(res, f"loop + distractor fuse={int(fuse)}", live=[0, 2], zero=[1], ref=model(sources(SR), b, units, SR, SR))


def test_half_rows_loop_three_rir_blocks(lib, banks):
    b = banks["long"]
    t0 = P.window_start_sim(3 * SR, SR, 2)                 # steady branch of the 3-s clip: every RIR block has a window
    units = [dict(sound=2, t0=t0, rir=0), dict(sound=0, t0=0, rir=1, dis_sound=1, dis_rir=0), dict(rir=-1)]
    res = ab(lib, b, SR, units, fuse=True, simple=False)
    check(res, "loop, 3 RIR blocks, fused", live=[0, 1], zero=[2], ref=model(sources(SR), b, units, SR, SR))


def test_half_rows_n_valid_4000_of_16000(lib, banks):
    b = banks["small"]
    res = ab(lib, b, SR, SIMPLE_UNITS, fuse=True, simple=True, n_valid=4000)
    ref = model(sources(SR), b, SIMPLE_UNITS, SR, 4000)
    check(res, "n_valid 4000 of 16000", live=[0, 3, 4], zero=[1, 2], ref=ref)
    assert not res["wave"][0][:, :, 4000:].any()


def test_half_rows_split_over_workgroups(lib, banks):
    b = banks["small"]
    res = ab(lib, b, SR, SIMPLE_UNITS[:2], fuse=True, simple=True, parts_log2=2)
    check(res, "fused, 4 workgroups per row", live=[0], zero=[1], ref=model(sources(SR), b, SIMPLE_UNITS[:2], SR, SR))


def test_half_rows_44100_unfused_three_output_blocks(lib, banks):
    sr = 44100
    b = banks["long"]
    t0 = P.window_start_sim(3 * sr, sr, 2)
    units = [dict(sound=2, t0=t0, rir=0), dict(sound=0, t0=0, rir=1), dict(rir=-1)]
    res = ab(lib, b, sr, units, fuse=False, simple=False)
    check(res, "44100 unfused (3 output blocks)", live=[0, 1], zero=[2], ref=model(sources(sr), b, units, sr, sr))


# ---- model and format loss ----------------------------------------------------------------------------------------------------
def test_model_matches_the_oracle_unquantised_and_format_loss():
    """rir16_ref's model without its quantiser is the oracle's convolution; with it the waveform moves by the format's loss,
    which is printed for INTEGRATION.md (the scale of the entry does not change it: the scale is a power of two per row)"""
    worst = 0.0
    for sr, taps in ((16000, (9000, 16000)), (44100, (9000, 44100))):
        rng = np.random.default_rng(sr + 1)
        src = O.synth_sources(rng, sr, k=1, seconds=3)[0]
        for n in taps:
            rir = (O.synth_rir(rng, sr, length=n, n=1) if n <= sr and sr == 16000 else O.synth_rir_blocks(rng, sr, n, n=1))[0]
            ref = O.compute_audiogoal(src, np.ascontiguousarray(rir.T), sr, audio_index=2)
            t0 = O.window_start(len(src), n, sr, 2)
            worst = max(worst, O.relerr(R.model_audiogoal(src, rir, t0, sr, quant=False), ref))
            for scale in (1.0, 32768.0, 1e-6):
                scaled = (rir * np.float32(scale)).astype(np.float32)
                ref_s = O.compute_audiogoal(src, np.ascontiguousarray(scaled.T), sr, audio_index=2)
                got = R.model_audiogoal(src, scaled, t0, sr, quant=True)
                wave = O.relerr(got, ref_s)
                sg = O.relerr(R.model_spectrogram(got), O.compute_spectrogram(np.asarray(ref_s, np.float64)))
                print(f"[rir16_host] format loss sr {sr} taps {n} scale {scale:g}: waveform {wave:.2e} of peak, "
                      f"pooled log1p spectrogram {sg:.2e}")
                assert 1e-6 < wave < 1e-2                    # (a sanity window, not the figure: a lossless or broken rule)
    print(f"[rir16_host] model (unquantised) vs oracle.compute_audiogoal: {worst:.2e}")
    assert worst <= 1e-6


# ---- route --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route_prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("route_rir16") / "route_rir16_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "route_rir16_host.cpp"), "-o", out])
    return out


def _run(prog, mode):
    r = subprocess.run([prog, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def test_route_field_clear_prints_the_recorded_table(route_prog):
    with open(os.path.join(HERE, "golden", "route_table.txt")) as f:
        golden = [ln for ln in f.read().splitlines() if not ln.startswith("#")]
    table = _run(route_prog, "table")
    assert len(golden) == 10 * 9 * 3 * 4 + 10 * 4 * 3 * 4 and table == golden      # (the fixed grid + the n_valid seam rows)


def test_route_of_a_half_rows_bank(route_prog):
    lines = _run(route_prog, "rows16")
    assert len(lines) == 9 * 3 * 4 * 5 * 2 * 3
    seen = set()
    for ln in lines:
        out_len, n_valid, depth, flags, w, n, pol, code = ln.split()
        out_len, flags, w = int(out_len), int(flags), int(w)
        if flags & 2:                                                    # a cross-fade: refused, whatever is asked for
            assert code == "-8", ln
            continue
        fused = out_len <= KB_ROWS and (1 + out_len // 160 + 3) // 4 <= 26
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
        assert code == want, ln
        seen.add(code)
    assert seen == {"C0", "F0", "T4", "T0", "C2", "F2", "T2"}


KB_ROWS = 16384
