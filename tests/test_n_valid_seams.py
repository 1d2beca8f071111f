"""Short steps (only the first n_valid samples of an out_len-sample row are rendered) with n_valid ON the seams of a launch:

  * 0, 1, 2 and 255 .. 257 (nothing rendered; fewer samples than the left centre pad reads),
  * 640 k - 256 + d, the seam of ssk::live_blocks (csrc/ss_consts.hpp): pooled column k is written as zeros, not computed, up
    to d = 0 and computed from d = 1 on.  The Hann window's zero taps keep the column exactly 0 up to d = 57, so d = 1 proves
    nothing about a column dropped by mistake; d = 200 does (143 live taps, the sources are white noise right up to the last
    rendered sample: test_the_boundary_column_is_loud_at_d_200),
  * kB - 1, kB, kB + 1, 2 kB, 2 kB +- 1: the rendered output blocks nb_y = ceil(n_valid / kB) step, and the route moves between
    the wide loop kernel (n_valid <= kB; kB = 640 * 26 - 256 meets its 26-column limit with equality), k_obs_rows and two launches,
  * out_len - 512 / - 511: the last n_valid at which the right centre pad mirrors zeros only (the shortcut is on), the first at
    which it is off; out_len - 257 .. out_len: the right pad mirrors rendered samples and zeros.

Every kernel that honours n_valid is run over that grid, G(out_len), at out_len 16000 (one block), 20000 (two) and 44100 / 48000
(three), both pad modes, three units (one with a distractor term - or, cross-faded, a previous RIR -, one silent, one plain):
on the kernels compiled for the host (tests/hostsim and the four log-mel drivers tests/obs_*logmel*_host.cpp) and, marked gpu, through
the public layers, where the library's own route decision is what runs: the stateless ss_amd.ops entries of the bank forms fp32
rows, fp32 spectra, half spectra, half rows, length buckets (rows, spectra only, half spectra) and the 512-thread core, with and
without a waveform buffer, cross-faded where the form has rows, their log-mel entries, and every refusal (SS_EINVAL, outputs
untouched); a context per n_valid on a subset of the grid; BatchedAudioRenderer(step_time=...); 72 units for k_obs_rows' loop.

Reference: the float64 convolution of each unit, computed once for the whole row; every n_valid case is that row zeroed from
n_valid on, and O.compute_spectrogram / O.compute_logmel of it.

Bounds (none of them new).  TOL = 1e-4 of the reference's peak: the suite's bound against the float64 model; 1e-5 between the
fused routes and two launches (tests/test_handoff_pads.py).  The last rendered sample is compared relative to its OWN oracle value
in every (unit, ear) where that value is loud - at least LOUD = 1e-2 of the row's peak, the qualifying ratio
tests/test_feature_edges.py uses; a sample near zero cannot be accurate relative to itself in fp32 -: TOL x peak of absolute
error is at most TOL / LOUD = 1e-2 of such a value, a dropped sample is 1.0 of it; every launch must have such a sample.  The
last live pooled column is looked at on its own as check_columns of tests/test_handoff_pads.py does.  Exact checks: samples >=
n_valid are +0 bit for bit, and so is every pooled column from live_blocks on; the log-mel frames there hold ONE fp32 bit
pattern, the kernel's logf(eps) (within an ulp of numpy's)."""
import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

KB = P.KB
TOL = 1e-4
RTOL_ROUTES = 1e-5
LOUD = 1e-2
EPS = 1e-6
PADS = ("reflect", "constant")
OUT_LENS = (16000, 20000, 44100, 48000)
T0 = (40, 0, 333)                    # window starts of the three units
T0_DIS = 0                           # (a distractor is heard from its clip's start)


def seam(k):
    return 640 * k - 256


def seam_ks(out_len):
    k_last = (min(out_len, KB) + 256) // 640
    return sorted({1, k_last // 2, k_last})


def grid(out_len):
    g = [0, 1, 2, 255, 256, 257]
    g += [seam(k) + d for k in seam_ks(out_len) for d in (0, 1, 57, 200)]
    g += [KB - 1, KB, KB + 1, KB + 57, KB + 200, 2 * KB - 1, 2 * KB, 2 * KB + 1, 2 * KB + 200]
    g += [out_len - d for d in (513, 512, 511, 257, 256, 1, 0)]
    return sorted({v for v in g if 0 <= v <= out_len})


def test_grid_holds_the_seams():
    assert seam(26) == KB and seam_ks(44100) == [1, 13, 26] and seam_ks(16000) == [1, 12, 25]
    for out_len in OUT_LENS:
        g = grid(out_len)
        t4 = P.spectrogram_shape(out_len)[1]
        assert g[0] == 0 and g[-1] == out_len and len(g) == len(set(g))
        nby = {P.ceil_div(v, KB) for v in g}
        assert nby == set(range(0, P.ceil_div(out_len, KB) + 1))                       # every count of rendered blocks
        for k in seam_ks(out_len):                                # live_blocks steps right behind the seam (while the shortcut is on)
            if seam(k) + 1 <= out_len - 512:
                assert P.live_pooled_blocks(seam(k), out_len) == k and P.live_pooled_blocks(seam(k) + 1, out_len) == k + 1
            else:
                assert out_len == 16000 and k == 25 and P.live_pooled_blocks(seam(k), out_len) == t4
        assert P.live_pooled_blocks(out_len - 512, out_len) == min(t4, (out_len - 512 + 256 + 639) // 640)
        assert P.live_pooled_blocks(out_len - 511, out_len) == t4                      # the shortcut is off
        if out_len > KB:
            assert P.wide_one_block(out_len, KB) and not P.wide_one_block(out_len, KB + 1)
            assert P.live_pooled_blocks(KB, out_len) == 26


# ---- the scene and its float64 rows, computed once per out_len and never written to -------------------------------------------
_SCENES = {}


def scene(out_len, variant="fp32", rows_bank=None):
    """white-noise sources (energy right up to the last rendered sample), three decaying-noise RIRs; the float64 rows of the
    units in their three forms: 'dis' (unit 0 carries a distractor term), 'plain' (it does not), 'xf' (unit 0 is cross-faded from
    a previous RIR).  A `variant` is the same scene heard through another bank, `rows_bank` [3, 2, cap] (dequantised half rows:
    the quantised model)"""
    if (out_len, variant) not in _SCENES:
        from scipy.signal import fftconvolve
        rng = np.random.default_rng(out_len)
        srcs = [rng.standard_normal(out_len + 400).astype(np.float32) for _ in range(2)]
        # (44100: an RIR of two partition blocks, so that the row kernels' stash is in play)
        lens = [9000, 5001, 12000] if out_len <= KB else [9000, 20000 if out_len == 44100 else 15000, 12001]
        cap = max(lens) + (max(lens) & 1)
        bank = np.zeros((3, 2, cap), np.float32)
        for i, L in enumerate(lens):
            bank[i, :, :L] = (0.05 * rng.standard_normal((2, L)) * np.exp(-np.arange(L) / (0.3 * L))[None, :]).astype(np.float32)
        if variant != "fp32":
            assert rows_bank.shape == bank.shape and rows_bank.dtype == np.float32
            bank = rows_bank

        def row(s, t0, r):
            full = fftconvolve(srcs[s].astype(np.float64)[None, :], bank[r, :, :lens[r]].astype(np.float64), axes=1)
            return full[:, t0:t0 + out_len]

        a0, a2, dis, prev = row(0, T0[0], 0), row(1, T0[2], 2), row(1, T0_DIS, 1), row(0, T0[0], 1)
        zero = np.zeros((2, out_len))
        rows = {"plain": [a0, zero, a2], "dis": [a0 + dis, zero, a2], "xf": [O.crossfade(prev, a0, out_len), zero, a2]}
        base = [dict(sound=0, t0=T0[0], rir=0), dict(rir=-1), dict(sound=1, t0=T0[2], rir=2)]
        units = {"plain": base,
                 "dis": [dict(base[0], dis_sound=1, dis_t0=T0_DIS, dis_rir=1)] + base[1:],
                 "xf": [dict(base[0], last_rir=1, wrap=False, last_wrap=False)] + [base[1], dict(base[2], wrap=False)]}
        _SCENES[(out_len, variant)] = dict(srcs=srcs, bank=bank, lens=lens, rows=rows, units=units, refs={})
    return _SCENES[(out_len, variant)]


def reference(out_len, form, n_valid, pad, mel_sr=None, variant="fp32"):
    """-> per unit (waveform [2, out_len], pooled spectrogram, log-mel | None) of the row zeroed from n_valid on, float64"""
    sc = scene(out_len, variant)
    key = (form, n_valid, pad, mel_sr)
    if key not in sc["refs"]:
        out = []
        for full in sc["rows"][form]:
            a = full.copy()
            a[:, n_valid:] = 0.0
            out.append((a, O.compute_spectrogram(a, pad_mode=pad),
                        O.compute_logmel(a, mel_sr, 64, EPS, pad) if mel_sr else None))
        sc["refs"][key] = out
    return sc["refs"][key]


def test_the_boundary_column_is_loud_at_d_200():
    """what makes the live_blocks seam testable: with noise behind it, column k is exactly 0 up to d = 57 (zero taps) and at
    least LOUD of the peak at d = 200"""
    for out_len in (16000, 44100):
        for k in seam_ks(out_len):
            if seam(k) + 200 > out_len - 512:                # (16000, k = 25: the right pad mirrors rendered samples into the column)
                continue
            for pad in PADS:
                for d, loud in ((0, False), (1, False), (57, False), (200, True)):
                    for u in (0, 2):
                        sg = reference(out_len, "dis", seam(k) + d, pad)[u][1]
                        assert not sg[:, k + 1:].any()
                        assert (np.abs(sg[:, k]).max() >= LOUD * np.abs(sg).max()) == loud, (out_len, k, pad, d, u)
                        assert loud or not sg[:, k].any()


# ---- the checks of one launch ------------------------------------------------------------------------------------------------
def is_pos_zero(x):
    return not np.ascontiguousarray(x, np.float32).view(np.uint32).any()


def is_log_eps(x):
    """frames that are written, not computed: ONE fp32 bit pattern in every cell, the kernel's logf(eps) (within an ulp of ours)"""
    x = np.ascontiguousarray(x, np.float32)
    return x.size == 0 or (np.unique(x.view(np.uint32)).size == 1 and bool(np.allclose(x, np.log(EPS), rtol=1e-6, atol=0)))


def check_launch(what, out_len, form, n_valid, pad, ag=None, sg=None, mel=None, mel_sr=None, worst=None, variant="fp32"):
    """one launch of the three units against the float64 rows; `worst` collects the largest error / peak per output"""
    refs = reference(out_len, form, n_valid, pad, mel_sr, variant)
    live = P.live_pooled_blocks(n_valid, out_len)
    worst = {} if worst is None else worst

    def note(name, e):
        worst[name] = max(worst.get(name, 0.0), e)

    loud_last = False
    for u, (ref_a, ref_s, ref_m) in enumerate(refs):
        w = f"{what} unit {u}"
        peak_a, peak_s = float(np.abs(ref_a).max()), float(np.abs(ref_s).max())
        if ag is not None:
            got = ag[u]
            assert got.shape == ref_a.shape and np.isfinite(got).all(), w
            assert is_pos_zero(got[:, n_valid:]), f"{w}: samples >= n_valid are not +0"
            if peak_a == 0.0:
                assert is_pos_zero(got), f"{w}: a silent row"
            else:
                e = float(np.abs(got - ref_a).max()) / peak_a
                note("waveform", e)
                assert e <= TOL, f"{w}: waveform {e:.2e}"
                # the last rendered sample, relative to its own oracle value, in every ear where that value is loud: TOL x peak
                # of absolute error is at most TOL / LOUD of a value of at least LOUD x peak
                own = np.abs(ref_a[:, n_valid - 1])
                e_last = np.abs(got[:, n_valid - 1] - ref_a[:, n_valid - 1])
                for ear in np.nonzero(own >= LOUD * peak_a)[0]:
                    assert e_last[ear] <= (TOL / LOUD) * own[ear], f"{w} ear {ear}: sample n_valid-1 off by {e_last[ear] / own[ear]:.2e} of its own value"
                    note("last sample / its own value", float(e_last[ear] / own[ear]))
                    loud_last = True
        if sg is not None:
            got = sg[u]
            assert got.shape == ref_s.shape and np.isfinite(got).all(), w
            assert is_pos_zero(got[:, live:]), f"{w}: pooled columns from {live} on are not +0"
            if peak_s == 0.0:
                assert is_pos_zero(got), f"{w}: spectrogram of a silent row"
            else:
                e = float(np.abs(got - ref_s).max()) / peak_s
                note("spectrogram", e)
                assert e <= TOL, f"{w}: spectrogram {e:.2e}"
                last = int(np.nonzero(np.abs(ref_s).max(axis=(0, 2)))[0].max())           # the last live column, on its own
                e = float(np.abs(got[:, last] - ref_s[:, last]).max())
                assert e <= TOL * peak_s, f"{w}: pooled column {last} off by {e / np.abs(ref_s[:, last]).max():.2e} of its own peak"
        if mel is not None:
            got = mel[u]
            assert got.shape == ref_m.shape and np.isfinite(got).all(), w
            e = float(np.abs(got - ref_m).max() / np.abs(ref_m).max())
            note("logmel", e)
            assert e <= TOL, f"{w}: log-mel {e:.2e}"
            assert is_log_eps(got[:, 4 * live:]), f"{w}: frames from {4 * live} on are not log(eps)"
            if peak_a == 0.0:
                assert is_log_eps(got), w
    if ag is not None and n_valid > 0:
        assert loud_last, f"{what}: no loud last sample to look at"
    return worst


def check_routes(what, sg, two):
    """a fused route against two launches over the same units"""
    den = max(float(np.abs(two).max()), 1e-30)
    e = float(np.abs(np.asarray(sg, np.float64) - two).max()) / den
    assert e <= RTOL_ROUTES, f"{what} vs two launches: {e:.2e}"
    return e


def report(tag, out_len, pad, worst):
    print(f"[{tag}] out_len={out_len} {pad}: " + ", ".join(f"{k} worst {v:.1e}" for k, v in sorted(worst.items())))


# ---- 1. the host build ---------------------------------------------------------------------------------------------------------
# (tag, form of unit 0, knobs of hs.run, serves this n_valid?)
def host_routes(out_len):
    if out_len <= KB:
        every = lambda nv: True
        return [("k_conv FUSE simple", "plain", dict(fuse=True, simple=True), every),
                ("k_conv FUSE loop", "dis", dict(fuse=True, simple=False), every),
                ("k_conv FUSE cross-faded", "xf", dict(fuse=True, crossfade=True), every),
                ("k_conv_spec FUSE simple", "plain", dict(fuse=True, spectral=True, simple=True), every),
                ("k_conv_spec FUSE loop", "dis", dict(fuse=True, spectral=True, simple=False), every),
                ("k_conv32 FUSE", "plain", dict(fuse=True, core32=True), every),
                ("k_conv32 FUSE tab", "plain", dict(fuse=True, core32=True, tab=True), every)]
    wide = lambda nv: nv <= KB
    every = lambda nv: True
    return [("k_conv WIDE", "dis", dict(fuse=True, simple=False), wide),
            ("k_conv WIDE cross-faded", "xf", dict(fuse=True, crossfade=True), wide),
            ("k_obs_rows", "dis", dict(row_wgs=2), every),
            ("k_obs_rows no waveform", "dis", dict(row_wgs=3, want_audiogoal=False, row_stash=True), every),
            ("k_obs_rows spectral", "dis", dict(row_wgs=1, spectral=True), every),
            ("k_obs_rows cross-faded", "xf", dict(row_wgs=2, crossfade=True), every)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("out_len", OUT_LENS)
def test_hostsim_seam_grid(out_len, pad):
    from hostsim import hs
    sc = scene(out_len)
    pm = PADS.index(pad)
    routes = host_routes(out_len)
    forms = sorted({r[1] for r in routes} | {"dis"})
    worst = {tag: {} for tag, _, _, _ in routes}
    worst["k_conv + k_spectrogram"] = {}
    routes_err = 0.0
    for nv in grid(out_len):
        # two launches: the unfused loop kernel, then k_spectrogram told where the zeros begin (SpecParams::live) - via hs.run and,
        # over the same waveform in chunks of three frame groups per workgroup, via hs.spectrogram
        two = {}
        for form in forms:
            ag, sg = hs.run(sc["srcs"], sc["bank"], sc["lens"], sc["units"][form], nv, out_len, fuse=False, simple=False,
                            want_spectrogram=True, pad_mode=pm, crossfade=form == "xf")
            check_launch(f"two launches ({form}) n_valid={nv} {pad}", out_len, form, nv, pad, ag, sg,
                         worst=worst["k_conv + k_spectrogram"])
            if form == "dis":
                np.testing.assert_array_equal(hs.spectrogram(ag, pm, 3, n_valid=nv), sg)
            two[form] = sg.astype(np.float64)
        for tag, form, kw, serves in routes:
            if not serves(nv):
                continue
            ag, sg = hs.run(sc["srcs"], sc["bank"], sc["lens"], sc["units"][form], nv, out_len, pad_mode=pm, **kw)
            what = f"{tag} n_valid={nv} {pad}"
            check_launch(what, out_len, form, nv, pad, ag, sg, worst=worst[tag])
            routes_err = max(routes_err, check_routes(what, sg, two[form]))
    for tag, w in worst.items():
        report(tag, out_len, pad, w)
    print(f"[fused vs two launches] out_len={out_len} {pad}: worst {routes_err:.1e}")


def test_hostsim_n_valid_0_writes_zeros_on_every_route():
    """nothing rendered.  The library spells the rendered blocks of such a step twice - 0 in the persistent rows launch, 1 in the
    observation body - and so does the host build (hs_obs_rows / hs_conv): either way every output is +0, bit for bit"""
    from hostsim import hs
    for out_len in OUT_LENS:
        sc = scene(out_len)
        for pm in (0, 1):
            routes = host_routes(out_len) + [("k_conv + k_spectrogram", "dis", dict(fuse=False, simple=False, want_spectrogram=True), None)]
            for tag, form, kw, _ in routes:
                ag, sg = hs.run(sc["srcs"], sc["bank"], sc["lens"], sc["units"][form], 0, out_len, pad_mode=pm, **kw)
                assert (ag is None or is_pos_zero(ag)) and is_pos_zero(sg), (tag, out_len, pm)


# ---- 1b. the log-mel instantiations on the host build (the drivers of tests/test_obs_*logmel*_host.py) ----------------------------
from test_obs_logmel_host import _run as _run_mel_one_block, mel_lib as mel_one_block_lib          # noqa: E402
from test_obs_logmel_ss2_host import _run as _run_mel_ss2, ss2_lib as mel_ss2_lib                  # noqa: E402
from test_obs_rows_logmel_host import _run as _run_mel_rows, mel_lib as mel_rows_lib               # noqa: E402


def _mel_units(sc, form):
    return [dict(u, wrap=False, last_wrap=False) if u.get("rir", -1) >= 0 else u for u in sc["units"][form]]


@pytest.mark.parametrize("pad", PADS)
def test_hostsim_seam_grid_logmel_one_block(mel_one_block_lib, pad):
    """k_conv<.., MEL> (loop-free, time-domain rows) and k_conv_spec<.., MEL> (loop form, a distractor term) at 16 kHz"""
    out_len, sc, pm = 16000, scene(16000), PADS.index(pad)
    for tag, form, spectral, simple in (("k_conv MEL simple", "plain", False, True), ("k_conv_spec MEL loop", "dis", True, False)):
        worst = {}
        for nv in grid(out_len):
            mel, sg, ag = _run_mel_one_block(mel_one_block_lib, sc["srcs"], sc["bank"], sc["lens"], sc["units"][form], nv, spectral,
                                             simple, pm, 64, True, want_wave=True)
            check_launch(f"{tag} n_valid={nv} {pad}", out_len, form, nv, pad, ag, sg, mel, mel_sr=out_len, worst=worst)
        report(tag, out_len, pad, worst)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("out_len", [16000, 44100])
def test_hostsim_seam_grid_logmel_ss2(mel_ss2_lib, out_len, pad):
    """k_conv<.., XFADE, .., WIDE, MEL>: the cross-faded one-block row; block 0 of a 44.1 kHz row, plain and cross-faded"""
    sc, pm = scene(out_len), PADS.index(pad)
    for tag, form in (("k_conv MEL cross-faded", "xf"),) + ((("k_conv WIDE MEL", "dis"),) if out_len > KB else ()):
        worst = {}
        for nv in (v for v in grid(out_len) if v <= KB):
            mel, sg, ag = _run_mel_ss2(mel_ss2_lib, out_len, sc["srcs"], sc["bank"], sc["lens"], _mel_units(sc, form), nv, form == "xf",
                                       pm, 64, True, want_wave=True)
            check_launch(f"{tag} n_valid={nv} {pad}", out_len, form, nv, pad, ag, sg, mel, mel_sr=out_len, worst=worst)
        report(tag, out_len, pad, worst)


@pytest.mark.parametrize("pad", PADS)
def test_hostsim_seam_grid_logmel_rows(mel_rows_lib, pad):
    """k_obs_rows<.., MEL> at 44.1 kHz, from time-domain rows and from block spectra"""
    out_len, sc, pm = 44100, scene(44100), PADS.index(pad)
    for tag, spectral in (("k_obs_rows MEL", False), ("k_obs_rows MEL spectral", True)):
        worst = {}
        for nv in grid(out_len):
            mel, sg, ag = _run_mel_rows(mel_rows_lib, out_len, sc["srcs"], sc["bank"], sc["lens"], sc["units"]["dis"], n_valid=nv,
                                        spectral=spectral, pad_mode=pm, want_sg=True, want_wave=not spectral, wgs=2)
            check_launch(f"{tag} n_valid={nv} {pad}", out_len, "dis", nv, pad, ag, sg, mel, mel_sr=out_len, worst=worst)
        report(tag, out_len, pad, worst)


# ---- 1c. the bucketed log-mel instantiations (tests/obs_logmel_buckets_host.cpp) -----------------------------------------------------
from test_obs_logmel_buckets_host import (AB as AB_HOST, HALF, K_BLOCKS, K_CONV, K_ROWS, ROWS, SPEC, _fp32_spectra,     # noqa: E402
                                          _launch as _launch_mel_buckets, lib as mel_buckets_lib)
import spec_half_rows_ref as HR                                                                                       # noqa: E402


def _bucketed(sc, lib):
    """the scene's bank as two length buckets (entries keep their global order: bucket 0 holds the entries in front of the first
    one longer than 10000 taps), as rows, fp32 block spectra, halves + scales and the dequantised halves; built once per scene"""
    if "buckets" not in sc:
        lens = sc["lens"]
        split = next(i for i, n in enumerate(lens) if n > 10000)
        assert 0 < split < len(lens) and max(lens[:split]) <= 10000
        caps = [10000, sc["bank"].shape[2]]
        rows = [np.ascontiguousarray(sc["bank"][:split, :, :caps[0]]), np.ascontiguousarray(sc["bank"][split:])]
        f32 = [_fp32_spectra(lib, r) for r in rows]
        qs = [HR.quantise(f) for f in f32]
        sc["buckets"] = dict(firsts=[0, split], caps=caps, rows=rows, f32=f32, q=[np.ascontiguousarray(q) for q, _ in qs],
                             s=[np.ascontiguousarray(s) for _, s in qs],
                             deq=[np.ascontiguousarray(HR.dequantise(q, s)) for q, s in qs])
    return sc["buckets"]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("out_len", [16000, 44100])
def test_hostsim_seam_grid_logmel_buckets(mel_buckets_lib, out_len, pad):
    """Over two length buckets (a distractor term from the other bucket).  16 kHz: k_conv<loop, MEL> on rows, k_conv_spec<loop, MEL>
    on fp32 spectra - both against the oracle - and the half form k_conv_spec<.., MEL, HALF, HBK> against the fp32 one fed
    float(q) * hscale (the bounds of tests/test_obs_logmel_buckets_host.py: 2e-6 of peak on waveform and spectrogram, 1e-4 on
    log-mel) with the exact zeros and log(eps) frames of its own.  44.1 kHz: k_obs_rows<.., BUCKETS, MEL> on rows and on fp32
    spectra over the grid, k_obs_blocks<.., MEL> at n_valid = out_len (all it serves).  (The driver has no half form of the row
    kernels.)"""
    sc, pm = scene(out_len), PADS.index(pad)
    b = _bucketed(sc, mel_buckets_lib)
    units = sc["units"]["dis"]

    def launch(kernel, form, banks, nv, scales=None, **kw):
        mel, sg, ag = _launch_mel_buckets(mel_buckets_lib, kernel, form, sc["srcs"], units, banks, scales, b["firsts"], b["caps"],
                                          sc["lens"], out_len, n_valid=nv, pad_mode=pm, **kw)
        return ag, sg, mel
    kernel = K_CONV if out_len <= KB else K_ROWS
    for tag, form, banks in (("MEL over row buckets", ROWS, b["rows"]), ("MEL over spectral buckets", SPEC, b["f32"])):
        worst = {}
        for nv in grid(out_len):
            ag, sg, mel = launch(kernel, form, banks, nv, wgs=2)
            check_launch(f"{tag} n_valid={nv} {pad}", out_len, "dis", nv, pad, ag, sg, mel, mel_sr=out_len, worst=worst)
        if out_len > KB:
            ag, sg, mel = launch(K_BLOCKS, form, banks, out_len)
            check_launch(f"k_obs_blocks {tag} {pad}", out_len, "dis", out_len, pad, ag, sg, mel, mel_sr=out_len, worst=worst)
        report(("k_conv " if out_len <= KB else "k_obs_rows ") + tag, out_len, pad, worst)
    if out_len > KB:
        return
    worst = {}
    for nv in grid(out_len):
        what = f"half spectral buckets MEL n_valid={nv} {pad}"
        half = launch(K_CONV, HALF, b["q"], nv, scales=b["s"])
        full = launch(K_CONV, SPEC, b["deq"], nv)
        live = P.live_pooled_blocks(nv, out_len)
        for name, h, f, bound in (("waveform", half[0], full[0], AB_HOST), ("spectrogram", half[1], full[1], AB_HOST), ("logmel", half[2], full[2], TOL)):
            assert np.isfinite(h).all() and np.isfinite(f).all(), what
            den = float(np.abs(f).max())
            e = float(np.abs(h.astype(np.float64) - f).max()) / den if den > 0 else float(np.abs(h).max())
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= bound, f"{what}: {name} half vs fp32(dequantised) {e:.2e}"
        assert is_pos_zero(half[0][:, :, nv:]) and is_pos_zero(half[0][1]), what
        assert is_pos_zero(half[1][:, :, live:]) and is_pos_zero(half[1][1]), what
        assert is_log_eps(half[2][:, :, 4 * live:]) and is_log_eps(half[2][1]), what
    report("k_conv_spec MEL HALF over buckets, vs fp32(dequantised)", out_len, pad, worst)


# ---- 2. the MI355X: the public layers, the library's own route decision ----------------------------------------------------------
DEV = "cuda:0"
AB = 2e-6                            # half forms against their fp32 sibling fed the dequantised bank (tests/test_gpu_spec_half*.py)
_WORLDS = {}


def _requests(form, index_of=(0, 1, 2)):
    from ss_amd.renderer import UnitRequest
    i = index_of
    first = {"plain": UnitRequest(0, T0[0], i[0]), "dis": UnitRequest(0, T0[0], i[0], dis_sound=1, dis_rir=i[1]),
             "xf": UnitRequest(0, T0[0], i[0], last_rir=i[1])}[form]
    return [first, UnitRequest(silent=True), UnitRequest(1, T0[2], i[2])]


def world(out_len):
    """the scene on the device in every bank form, planned once (for the whole row: a short step uses fewer of the windows)"""
    if out_len not in _WORLDS:
        import types
        import torch
        from ss_amd import ops
        from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank
        sc = scene(out_len)
        rirs = [np.ascontiguousarray(sc["bank"][i, :, :L].T) for i, L in enumerate(sc["lens"])]

        def renderer(bank):
            r = BatchedAudioRenderer(out_len, device=DEV)
            for i, s in enumerate(sc["srcs"]):
                r.add_source(f"s{i}", s)
            r.set_rir_bank(bank)
            return r
        w = types.SimpleNamespace(out_len=out_len, rirs=rirs)
        w.r = renderer(RirBank.from_arrays(rirs, DEV))
        assert w.r.rirs.cap == sc["bank"].shape[2]
        w.plans = {f: w.r.plan(_requests(f)) for f in ("plain", "dis", "xf")}
        w.spectra = w.r.rirs.build_spectra()
        w.spectra16, w.hscale = ops.rir_spectra16(w.r.rirs.data)
        w.spectra_deq = (w.spectra16.float() * w.hscale[..., None]).contiguous()
        w.rows16, w.rscale = ops.rir_rows16(w.r.rirs.data)
        scene(out_len, "rows16", (w.rows16.float() * w.rscale[..., None]).cpu().numpy())          # the quantised model's rows
        bk = BucketedRirBank.from_arrays(rirs, DEV, caps=[10000, sc["bank"].shape[2]])
        w.rb = renderer(bk)
        w.bk_plans = {f: w.rb.plan(_requests(f, bk.index_of)) for f in ("dis", "xf")}
        bk.build_spectra()
        firsts, caps = bk.first, [b.cap for b in bk.banks]
        halves = [ops.rir_spectra16(b.data) for b in bk.banks]
        deq = [(q.float() * sc[..., None]).contiguous() for q, sc in halves]
        w.sbk_keep = (halves, deq)                                          # (the arrays below point into these)
        w.sbk = ops.spec_bucket_array([b.spectra for b in bk.banks], None, firsts, caps)
        w.sbk16 = ops.spec_bucket_array([q for q, _ in halves], [sc for _, sc in halves], firsts, caps)
        w.sbk_deq = ops.spec_bucket_array(deq, None, firsts, caps)
        if out_len <= KB:                                                   # the 512-thread core: window spectra in ITS order
            from ss_amd import _lib
            lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
            w.spec32 = torch.zeros_like(w.r._spec)
            for (sid, t0, wrap), (slot, ws) in w.r._windows.items():
                wd = torch.from_numpy(np.ascontiguousarray(P.window_desc_rows(ws, w.r.sources.offsets[sid], w.r.sources.lengths[sid], wrap))).to(DEV)
                assert slot + len(wd) <= w.spec32.shape[0]
                _lib.check(lib.ss_source_windows32_f32(w.r.sources.flat().data_ptr(), wd.data_ptr(), w.spec32[slot:slot + len(wd)].data_ptr(),
                                                       len(wd), stream), "ss_source_windows32_f32")
        ms, mw, _ = P.mel_filterbank_sparse(out_len, 64)
        w.mel = (torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(DEV))
        torch.cuda.synchronize()
        _WORLDS[out_len] = w
    return _WORLDS[out_len]


def gpu_launch(out_len, call, want_ag, want_sg=True, want_mel=False, n=3):
    """NaN-filled outputs, one call -> (audiogoal, spectrogram, logmel) as numpy, or None for a refusal (SS_EINVAL), which must
    have left every output untouched"""
    import torch
    ag = torch.full((n, 2, out_len), float("nan"), device=DEV) if want_ag else None
    sg = torch.full((n,) + P.spectrogram_shape(out_len), float("nan"), device=DEV) if want_sg else None
    lm = torch.full((n, 64, 1 + out_len // 160, 2), float("nan"), device=DEV) if want_mel else None
    try:
        call(ag, sg, lm)
    except RuntimeError as e:
        assert "failed: invalid argument" in str(e), e
        torch.cuda.synchronize()
        assert all(t is None or bool(torch.isnan(t).all()) for t in (ag, sg, lm)), "a refused call wrote to its outputs"
        return None
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (ag, sg, lm))


def gpu_entries(w, form_name):
    """-> [(tag, unit form, call(nv, pad) -> (ag, sg, lm) -> None, wants a waveform buffer, log-mel?, serves(nv)?, model variant)]"""
    from ss_amd import ops
    out_len, r = w.out_len, w.r
    spec, lens = r._spec, r.rirs.lengths
    one = out_len <= KB
    every, never, block0 = (lambda nv: True), (lambda nv: False), (lambda nv: nv <= KB)
    E = []

    def add(tag, form, fn, serves=every, mel=False, variant="fp32", plans=None):
        plan = (plans or w.plans)[form]
        for want_ag in (True, False):
            E.append((f"{tag}{'' if want_ag else ', no waveform'}", form,
                      (lambda nv, pad, fn=fn, plan=plan: (lambda ag, sg, lm: fn(plan, ag, sg, lm, nv, pad))), want_ag, mel, serves, variant))
    ms, mw = w.mel
    if form_name == "rows":
        bank = r.rirs.data
        obs = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_into(spec, bank, lens, p.desc, ag, sg, nv, out_len, pad, flags=p.flags)
        add("ss_audio_obs_f32", "dis", obs)
        add("ss_audio_obs_f32 cross-faded", "xf", obs)
        mel1 = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_into(spec, bank, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        ss2 = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_ss2_into(spec, bank, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        mrows = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_rows_into(spec, bank, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        add("ss_audio_obs_logmel_f32", "dis", mel1, every if one else never, mel=True)
        add("ss_audio_obs_logmel_f32 cross-faded", "xf", mel1, never, mel=True)
        add("ss_audio_obs_logmel_ss2_f32", "dis", ss2, never if one else block0, mel=True)
        add("ss_audio_obs_logmel_ss2_f32 cross-faded", "xf", ss2, every if one else block0, mel=True)
        add("ss_audio_obs_logmel_rows_f32", "dis", mrows, never if one else every, mel=True)
        add("ss_audio_obs_logmel_rows_f32 cross-faded", "xf", mrows, never, mel=True)
    elif form_name == "spectra":
        obs = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_spec_into(spec, w.spectra, lens, p.desc, ag, sg, nv, out_len, pad, flags=p.flags)
        add("ss_audio_obs_spec_f32", "dis", obs)
        add("ss_audio_obs_spec_f32 cross-faded", "xf", obs, never)
        mel1 = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_spec_into(spec, w.spectra, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        mrows = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_rows_spec_into(spec, w.spectra, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        add("ss_audio_obs_logmel_spec_f32", "dis", mel1, every if one else never, mel=True)
        add("ss_audio_obs_logmel_rows_spec_f32", "dis", mrows, never if one else every, mel=True)
    elif form_name == "half rows":
        fn = ops.audio_obs_rir16_into if one else ops.audio_obs_rows_rir16_into
        obs = lambda p, ag, sg, lm, nv, pad: fn(spec, w.rows16, w.rscale, lens, p.desc, ag, sg, nv, out_len, pad, flags=p.flags)
        add("ss_audio_obs_rir16_f32" if one else "ss_audio_obs_rows_rir16_f32", "dis", obs, variant="rows16")
        add("ss_audio_obs_*rir16_f32 cross-faded", "xf", obs, never, variant="rows16")
    elif form_name == "buckets":
        bk = w.rb.rirs
        obs = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_buckets_into(w.rb._spec, bk.c_array(False), len(bk.banks), bk.lengths, p.desc,
                                                                       ag, sg, nv, out_len, pad, flags=p.flags)
        add("ss_audio_obs_buckets_f32", "dis", obs, plans=w.bk_plans)
        add("ss_audio_obs_buckets_f32 cross-faded", "xf", obs, plans=w.bk_plans)
        mel = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_buckets_into(w.rb._spec, bk.c_array(False), len(bk.banks), bk.lengths, p.desc,
                                                                              ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        add("ss_audio_obs_logmel_buckets_f32", "dis", mel, mel=True, plans=w.bk_plans)
        add("ss_audio_obs_logmel_buckets_f32 cross-faded", "xf", mel, never, mel=True, plans=w.bk_plans)
    elif form_name == "spectral buckets":
        bk = w.rb.rirs
        obs = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_spec_buckets_into(w.rb._spec, w.sbk, len(bk.banks), bk.lengths, p.desc, ag, sg,
                                                                            nv, out_len, pad, flags=p.flags)
        mel = lambda p, ag, sg, lm, nv, pad: ops.audio_obs_logmel_spec_buckets_into(w.rb._spec, w.sbk, len(bk.banks), bk.lengths, p.desc,
                                                                                   ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags)
        add("ss_audio_obs_spec_buckets_f32", "dis", obs, plans=w.bk_plans)
        add("ss_audio_obs_spec_buckets_f32 cross-faded", "xf", obs, never, plans=w.bk_plans)
        add("ss_audio_obs_logmel_spec_buckets_f32", "dis", mel, mel=True, plans=w.bk_plans)
    elif form_name == "32-core":
        from ss_amd import _lib
        import torch
        bank = r.rirs.data
        cap = int(bank.shape[2])

        def obs32(p, ag, sg, lm, nv, pad):
            with torch.cuda.device(bank.device):
                _lib.check(_lib.load().ss_audio_obs32_f32(w.spec32.data_ptr() if one else spec.data_ptr(), bank.data_ptr(), lens.data_ptr(),
                                                          p.desc.data_ptr(), None if ag is None else ag.data_ptr(), sg.data_ptr(), 3, 2 * cap,
                                                          cap, 1, cap, nv, out_len, PADS.index(pad), torch.cuda.current_stream().cuda_stream),
                           "ss_audio_obs32_f32")
        add("ss_audio_obs32_f32", "plain", obs32, every if one else never)
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("form_name", ["rows", "spectra", "half rows", "buckets", "spectral buckets", "32-core"])
@pytest.mark.parametrize("out_len", OUT_LENS)
def test_gpu_stateless_entries_seam_grid(out_len, form_name):
    """the stateless ops.*_into entries of a bank form over G(out_len), both pad modes, with and without a waveform buffer,
    cross-faded where the form has rows to read; the log-mel entries; refusals are SS_EINVAL and touch nothing"""
    import torch
    from ss_amd import ops
    w = world(out_len)
    entries = gpu_entries(w, form_name)
    worst, routes_err, refused = {}, 0.0, set()
    for pad in PADS:
        for nv in grid(out_len):
            two = {}
            for tag, form, make, want_ag, mel, serves, variant in entries:
                what = f"{tag} n_valid={nv} {pad}"
                out = gpu_launch(out_len, make(nv, pad), want_ag, True, mel)
                if not serves(nv):
                    assert out is None, f"{what}: served, a refusal (SS_EINVAL) expected"
                    refused.add(tag)
                    continue
                assert out is not None, f"{what}: refused"
                ag, sg, lm = out
                check_launch(what, out_len, form, nv, pad, ag, sg, lm, mel_sr=out_len if mel else None,
                             worst=worst.setdefault(tag, {}), variant=variant)
                if ag is not None and not mel and form not in two:               # its waveform through k_spectrogram: two launches
                    two[form] = ops.spectrogram(torch.from_numpy(ag).to(DEV), pad).cpu().numpy().astype(np.float64)
                elif ag is None and not mel and form in two:
                    routes_err = max(routes_err, check_routes(what, sg, two[form]))
    for tag, wv in worst.items():
        report(f"gpu {tag}", out_len, "both pads", wv)
    print(f"[gpu {form_name}: one launch vs its waveform through k_spectrogram] out_len={out_len}: worst {routes_err:.1e}; "
          f"refused as expected: {sorted(refused)}")


@pytest.mark.gpu
@pytest.mark.parametrize("out_len", OUT_LENS)
def test_gpu_half_spectra_seam_grid(out_len):
    """ss_audio_obs_spec16_f32 (one block) / ss_audio_obs_rows_spec16_f32 (2 or 3), and half spectral length buckets
    (ss_audio_obs_spec_buckets_f32 / ss_audio_obs_rows_spec16_buckets_f32), and the log-mel entries of both: against the fp32 entry
    fed the dequantised spectra on identical arguments (the same route: AB, tests/test_gpu_spec_half*.py), and the exact zeros"""
    from ss_amd import ops
    w = world(out_len)
    spec, lens, p = w.r._spec, w.r.rirs.lengths, w.plans["dis"]
    bk, pb, nb = w.rb.rirs, w.bk_plans["dis"], len(w.rb.rirs.banks)
    ms, mw = w.mel
    one = out_len <= KB
    half_bk = ops.audio_obs_spec_buckets_into if one else ops.audio_obs_rows_spec16_buckets_into
    mel_one = ops.audio_obs_logmel_spec_into if one else ops.audio_obs_logmel_rows_spec_into
    half_mel_bk = ops.audio_obs_logmel_spec_buckets_into if one else ops.audio_obs_logmel_rows_spec16_buckets_into
    # name -> (the half entry, the fp32 entry on the dequantised spectra, log-mel?)
    pairs = {
        "half spectra": (
            lambda ag, sg, lm, nv, pad: ops.audio_obs_spec_into(spec, w.spectra16, lens, p.desc, ag, sg, nv, out_len, pad, flags=p.flags, hscale=w.hscale),
            lambda ag, sg, lm, nv, pad: ops.audio_obs_spec_into(spec, w.spectra_deq, lens, p.desc, ag, sg, nv, out_len, pad, flags=p.flags), False),
        "half spectra log-mel": (
            lambda ag, sg, lm, nv, pad: mel_one(spec, w.spectra16, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags, hscale=w.hscale),
            lambda ag, sg, lm, nv, pad: mel_one(spec, w.spectra_deq, lens, p.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad, flags=p.flags), True),
        "half spectral buckets": (
            lambda ag, sg, lm, nv, pad: half_bk(w.rb._spec, w.sbk16, nb, bk.lengths, pb.desc, ag, sg, nv, out_len, pad, flags=pb.flags),
            lambda ag, sg, lm, nv, pad: ops.audio_obs_spec_buckets_into(w.rb._spec, w.sbk_deq, nb, bk.lengths, pb.desc, ag, sg, nv, out_len, pad,
                                                                        flags=pb.flags), False),
        "half spectral buckets log-mel": (
            lambda ag, sg, lm, nv, pad: half_mel_bk(w.rb._spec, w.sbk16, nb, bk.lengths, pb.desc, ag, sg, lm, ms, mw, nv, out_len, EPS, pad,
                                                    flags=pb.flags),
            lambda ag, sg, lm, nv, pad: ops.audio_obs_logmel_spec_buckets_into(w.rb._spec, w.sbk_deq, nb, bk.lengths, pb.desc, ag, sg, lm, ms, mw, nv,
                                                                               out_len, EPS, pad, flags=pb.flags), True)}
    worst_ab = {}
    for pad in PADS:
        for nv in grid(out_len):
            for want_ag, name in ((a, n) for a in (True, False) for n in pairs):
                what = f"{name} n_valid={nv} {pad} waveform={want_ag}"
                mel = pairs[name][2]
                half = gpu_launch(out_len, lambda ag, sg, lm: pairs[name][0](ag, sg, lm, nv, pad), want_ag, True, mel)
                full = gpu_launch(out_len, lambda ag, sg, lm: pairs[name][1](ag, sg, lm, nv, pad), want_ag, True, mel)
                assert half is not None and full is not None, what
                live = P.live_pooled_blocks(nv, out_len)
                for got, ref in zip(half, full):
                    if got is None:
                        continue
                    assert np.isfinite(got).all() and np.isfinite(ref).all(), what
                    den = float(np.abs(ref).max())
                    e = float(np.abs(got.astype(np.float64) - ref).max()) / den if den > 0 else float(np.abs(got).max())
                    worst_ab[name] = max(worst_ab.get(name, 0.0), e)
                    assert e <= AB, f"{what}: half vs fp32(dequantised) {e:.2e}"
                assert is_pos_zero(half[1][:, :, live:]) and (half[0] is None or is_pos_zero(half[0][:, :, nv:])), what
                assert is_pos_zero(half[1][1]) and (half[0] is None or is_pos_zero(half[0][1])), what
                if mel:
                    assert is_log_eps(half[2][:, :, 4 * live:]) and is_log_eps(half[2][1]), what
    for name, e in worst_ab.items():
        print(f"[gpu {name}] out_len={out_len}: max |half - fp32(dequantised)| / peak worst {e:.1e}")


CTX_SUBSET = (0, 1, KB - 1, KB, KB + 1, seam(26) - 200, seam(26) + 200)


@pytest.mark.gpu
@pytest.mark.parametrize("out_len", OUT_LENS)
def test_gpu_context_seam_subset(out_len):
    """one context per (out_len, n_valid, pad) - time-domain rows under reflect padding, rows and block spectra under constant -:
    ss_ctx_observe with and without a waveform buffer, plain and cross-faded, and ss_ctx_observe_features with every log-mel
    policy opened"""
    import torch
    from ss_amd.context import AudioContext
    w = world(out_len)
    sc = scene(out_len)
    sound, t0, rir = np.array([0, 0, 1]), np.array([T0[0], 0, T0[2]]), np.array([0, -1, 2])
    cols = {"dis": dict(dis_sound=np.array([1, -1, -1]), dis_rir=np.array([1, -1, -1])), "xf": dict(last_rir=np.array([1, -1, -1]))}
    ms, mw = w.mel
    worst = {}
    for pad, both_forms in ((PADS[0], False), (PADS[1], True)):              # constant: block spectra bound next to the rows
        for nv in sorted({v for v in CTX_SUBSET + (out_len - 512, out_len - 511) if 0 <= v <= out_len}):
            ctx = AudioContext(out_len, pad_mode=pad, n_valid=nv)
            try:
                for i, s in enumerate(sc["srcs"]):
                    ctx.add_source(f"s{i}", s)
                ctx.set_rir_bank(w.r.rirs.data, w.r.rirs.lengths)
                if both_forms:
                    ctx.set_rir_spectra(w.spectra)
                for policy in (ctx.set_logmel_policy, ctx.set_logmel_rows_policy, ctx.set_logmel_ss2_policy):
                    policy(1, 1 << 20)
                for form in ("dis", "xf"):
                    for want_ag in (True, False):
                        what = f"ss_ctx_observe {form} n_valid={nv} {pad} waveform={want_ag}"
                        out = gpu_launch(out_len, lambda ag, sg, lm: ctx.observe(sound, t0, rir, sg, ag, **cols[form]), want_ag)
                        assert out is not None, what
                        check_launch(what, out_len, form, nv, pad, out[0], out[1], worst=worst.setdefault("ss_ctx_observe", {}))
                    what = f"ss_ctx_observe_features {form} n_valid={nv} {pad}"
                    out = gpu_launch(out_len, lambda ag, sg, lm: ctx.observe(sound, t0, rir, sg, None, logmel_out=lm, mel_start=ms, mel_w=mw,
                                                                            mel_eps=EPS, **cols[form]), False, True, True)
                    assert out is not None, what
                    check_launch(what, out_len, form, nv, pad, None, out[1], out[2], mel_sr=out_len,
                                 worst=worst.setdefault("ss_ctx_observe_features", {}))
                ctx.join()
                torch.cuda.synchronize()
            finally:
                ctx.close()
    for tag, wv in worst.items():
        report(f"gpu {tag}", out_len, "both pads", wv)


@pytest.mark.gpu
@pytest.mark.parametrize("out_len", OUT_LENS)
def test_gpu_renderer_step_times_on_the_seams(out_len):
    """BatchedAudioRenderer(step_time=...) with int(sr * step_time) on every value of G(out_len)"""
    import torch
    from ss_amd.renderer import BatchedAudioRenderer, RirBank
    w = world(out_len)
    sc = scene(out_len)
    worst = {}
    for k, nv in enumerate(grid(out_len)):
        pad = PADS[k % 2] if nv not in (KB, KB + 1, out_len - 512, out_len - 511) else None
        for pm in PADS if pad is None else (pad,):
            step_time = (nv + 0.5) / out_len
            r = BatchedAudioRenderer(out_len, device=DEV, pad_mode=pm, step_time=step_time)
            assert r.n_valid == nv
            for i, s in enumerate(sc["srcs"]):
                r.add_source(f"s{i}", s)
            r.set_rir_bank(RirBank(w.r.rirs.data, w.r.rirs.lengths))
            for form in ("dis", "xf"):
                plan = r.plan(_requests(form))
                for want_ag in (True, False):
                    ag, sg = r.render(plan, want_audiogoal=want_ag)
                    torch.cuda.synchronize()
                    check_launch(f"renderer step_time={step_time:.6f} (n_valid={nv}) {form} {pm} waveform={want_ag}", out_len, form, nv, pm,
                                 ag.cpu().numpy() if want_ag else None, sg.cpu().numpy(), worst=worst)
    report("gpu BatchedAudioRenderer", out_len, "both pads", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("n_valid", [KB + 1, 2 * KB + 1])
def test_gpu_obs_rows_persistent_loop_72_units(n_valid):
    """72 units (144 rows x 2-3 blocks: more than the chip's CUs, asserted) of a 44.1 kHz short step: k_obs_rows' persistent loop"""
    import torch
    from ss_amd import ops
    out_len = 44100
    w = world(out_len)
    assert 2 * 72 * P.ceil_div(n_valid, KB) > torch.cuda.get_device_properties(0).multi_processor_count
    p = w.plans["dis"]
    desc = p.desc.repeat(24, 1).contiguous()
    for pad in PADS:
        for want_ag in (True, False):
            out = gpu_launch(out_len, lambda ag, sg, lm: ops.audio_obs_into(w.r._spec, w.r.rirs.data, w.r.rirs.lengths, desc, ag, sg,
                                                                            n_valid, out_len, pad, flags=p.flags), want_ag, n=72)
            assert out is not None
            worst = {}
            for k in range(24):
                check_launch(f"72 units n_valid={n_valid} {pad} waveform={want_ag} units {3 * k}..", out_len, "dis", n_valid, pad,
                             None if out[0] is None else out[0][3 * k:3 * k + 3], out[1][3 * k:3 * k + 3], worst=worst)
            report(f"gpu k_obs_rows 72 units waveform={want_ag}", out_len, pad, worst)


@pytest.mark.gpu
def test_gpu_n_valid_0_writes_zeros_on_every_route():
    """the two spellings of nb_y at n_valid = 0 (0 blocks in the persistent rows launch, 1 in the observation body): every entry
    of every bank form writes all-zero outputs - +0 bit for bit, log(eps) in the log-mel - or refuses"""
    for out_len in OUT_LENS:
        w = world(out_len)
        for form_name in ("rows", "spectra", "half rows", "buckets", "spectral buckets", "32-core"):
            for tag, form, make, want_ag, mel, serves, variant in gpu_entries(w, form_name):
                for pad in PADS:
                    out = gpu_launch(out_len, make(0, pad), want_ag, True, mel)
                    assert (out is None) == (not serves(0)), (tag, out_len, pad)
                    if out is not None:
                        assert (out[0] is None or is_pos_zero(out[0])) and is_pos_zero(out[1]), (tag, out_len, pad)
                        assert out[2] is None or is_log_eps(out[2]), (tag, out_len, pad)
