"""The waveform-side kernels (k_spectrogram, k_logmel, k_gccphat, the fused k_features, k_intensity) where the rest of the suite
does not look: rows shorter than one STFT frame's reach (the centre padding then reflects more than once, as np.pad does),
levels from 1e-6 to 1e2 against regularisers from 1e-10 to 10, impulses / DC / on-bin tones / tilted noise, and the edges of
max_lag, n_mels and the rate of the filter bank.

The reference is always the oracle evaluated in float64 (the float32 rows are widened before they go in).  Every case runs
twice: on the kernels compiled for the host (tests/hostsim) and, marked gpu, through ss_amd.ops / torch.ops.ss_hip; each checks
the stand-alone kernel AND the same output of k_features, for every `want` subset where that is cheap.

Tolerances.  TOL = 1e-4 of the output's own peak is the project's.  GCC-PHAT is compared against THAT UNIT's oracle peak, never
against the full scale 1.0 (a regularised row peaks at 1e-4 or less).  Log-mel over the level x eps grid is compared in the log
domain with an absolute bound (LOGMEL_ABS).  A row of the pooled spectrogram is compared against that row's own peak where it is
at least 1e-2 of the global peak (below that float32 rounding of the loud bins sets the floor)."""
import itertools

import numpy as np
import pytest

from oracle import ss_oracle as O
from ss_amd import planning as P

TOL = 1e-4
NAMES = ("spectrogram", "logmel", "gccphat")
SUBSETS = [w for k in (1, 2, 3) for w in itertools.combinations(NAMES, k)]
PADS = ("reflect", "constant")

# worst |got - oracle| of the clean host kernels (k_logmel and k_features alike) over LEVELS x MEL_EPS below: 4.9e-6,
# rounded up to the next power of ten
LOGMEL_ABS = 1e-5

# Short rows under reflect padding are periodic (period 2(len-1)), so most STFT bins of a frame are nearly empty.  PHAT gives such
# a bin the phase of its float32 rounding noise unless eps outweighs that noise, and log(mel + eps) shows the same noise once it
# nears eps; both scale with the square of the level.  The short rows are therefore drawn at level SHORT_LEVEL (log-mel at its
# default eps = 1e-6 then sits 100x above the noise), and GCC-PHAT's eps was raised by decades from its default until the clean
# host kernels held 1e-4 of the unit's oracle peak with a 10x margin over SHORT_LENS x both pad modes:
#   eps 1e-8: 9.3e-5   1e-7: 2.0e-5   1e-6: 9.2e-6 (taken)   1e-5: 4.2e-6      (log-mel 5.6e-7, spectrogram 3.1e-6 of the peak)
SHORT_LEVEL = 1e-2
SHORT_GCC_EPS = 1e-6
# Tonal frames (DC, on-bin sines of amplitude 0.1): the same effect.  Clean host kernels, worst error / oracle peak over
# structured_inputs():  eps 1e-3: 1.5e-5 (holds 1e-4, but with a 6.5x margin)   1e-2: 4.9e-6 (taken: 20x)   1e-1: 1.2e-6
TONAL_GCC_EPS = 1e-2

SHORT_LENS = sorted({1, 2, 3, 37, 100, 159, 160, 161, 170, 178, 179, 192, 199, 200, 255, 256, 257} |
                    {160 * k + d for k in (3, 4, 15, 16) for d in (-1, 0, 1)})
LEVELS = (1e-6, 1e-4, 1e-2, 1.0, 1e2)
GCC_EPS = (1e-8, 1e-5, 1e-2, 10.0)
MEL_EPS = (1e-10, 1e-6, 1e-2)


# ---- the two back ends: the same calls on the host build and on the GPU ---------------------------------------------------
class Host:
    refused = (AssertionError, r"^-2")                       # hs.* asserts the launcher's return code (-2: argument check)

    def __init__(self, gpw=1):
        from hostsim import hs
        self.hs, self.gpw = hs, gpw

    def spectrogram(self, x, pad="reflect"):
        return self.hs.spectrogram(x, PADS.index(pad), self.gpw)

    def logmel(self, x, sr, n_mels=64, eps=1e-6, pad="reflect"):
        return self.hs.logmel(x, sr, n_mels, eps, PADS.index(pad), self.gpw)

    def gccphat(self, x, max_lag=32, eps=1e-8, pad="reflect"):
        return self.hs.gccphat(x, max_lag, eps, PADS.index(pad), self.gpw)

    def features(self, x, sr, want=NAMES, n_mels=64, mel_eps=1e-6, max_lag=32, gcc_eps=1e-8, pad="reflect"):
        return self.hs.features(x, sr, want, n_mels, mel_eps, max_lag, gcc_eps, PADS.index(pad), self.gpw)

    def intensity(self, x, num_frame=150):
        return self.hs.intensity(x, num_frame)

    def logmel_bank(self, x, start, w, eps):
        import ctypes
        hs = self.hs
        x = np.ascontiguousarray(x, np.float32)
        out = np.full((x.shape[0], w.shape[0], 1 + x.shape[2] // 160, 2), np.nan, np.float32)
        rc = hs.lib().hs_logmel(hs._p(x, ctypes.c_float), hs._p(out, ctypes.c_float), x.shape[0], x.shape[2], 0,
                                hs._p(start, ctypes.c_int), hs._p(w, ctypes.c_float), w.shape[0], w.shape[1], ctypes.c_float(eps), 1)
        assert rc == 0, rc
        full = np.full_like(out, np.nan)
        rc = hs.lib().hs_features(hs._p(x, ctypes.c_float), x.shape[0], x.shape[2], 0, None, hs._p(full, ctypes.c_float),
                                  hs._p(start, ctypes.c_int), hs._p(w, ctypes.c_float), w.shape[0], w.shape[1], ctypes.c_float(eps),
                                  None, 32, ctypes.c_float(1e-8), 1)
        assert rc == 0, rc
        return out, full


class Gpu:
    refused = (RuntimeError, "failed: invalid argument")     # SS_EINVAL as SsHipError (a RuntimeError) from ops.*
    dev = "cuda:0"

    def __init__(self):
        import torch
        from ss_amd import ops
        self.torch, self.ops, self._banks = torch, ops, {}

    def _x(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.dev)

    def _bank(self, sr, n_mels):
        if (sr, n_mels) not in self._banks:
            s, w, _ = P.mel_filterbank_sparse(sr, n_mels)
            self._banks[(sr, n_mels)] = (self.torch.from_numpy(s).to(self.dev), self.torch.from_numpy(w).to(self.dev))
        return self._banks[(sr, n_mels)]

    def spectrogram(self, x, pad="reflect"):
        xd = self._x(x)
        got = self.ops.spectrogram(xd, pad).cpu().numpy()
        np.testing.assert_array_equal(got, self.torch.ops.ss_hip.spectrogram(xd, PADS.index(pad)).cpu().numpy())
        return got

    def logmel(self, x, sr, n_mels=64, eps=1e-6, pad="reflect"):
        xd, (ms, mw) = self._x(x), self._bank(sr, n_mels)
        got = self.ops.logmel(xd, ms, mw, eps, pad).cpu().numpy()
        np.testing.assert_array_equal(got, self.torch.ops.ss_hip.logmel(xd, ms, mw, eps, PADS.index(pad)).cpu().numpy())
        return got

    def gccphat(self, x, max_lag=32, eps=1e-8, pad="reflect"):
        xd = self._x(x)
        got = self.ops.gccphat(xd, max_lag, eps, pad).cpu().numpy()
        np.testing.assert_array_equal(got, self.torch.ops.ss_hip.gccphat(xd, max_lag, eps, PADS.index(pad)).cpu().numpy())
        return got

    def features(self, x, sr, want=NAMES, n_mels=64, mel_eps=1e-6, max_lag=32, gcc_eps=1e-8, pad="reflect"):
        xd = self._x(x)
        ms, mw = self._bank(sr, n_mels) if "logmel" in want else (None, None)
        out = {k: v.cpu().numpy() for k, v in self.ops.audio_features(xd, want, ms, mw, mel_eps, max_lag, gcc_eps, pad).items()}
        if tuple(want) == ("logmel", "gccphat"):             # the torch op is this subset
            lm, gc = self.torch.ops.ss_hip.audio_features(xd, ms, mw, mel_eps, max_lag, gcc_eps, PADS.index(pad))
            np.testing.assert_array_equal(out["logmel"], lm.cpu().numpy())
            np.testing.assert_array_equal(out["gccphat"], gc.cpu().numpy())
        return out

    def intensity(self, x, num_frame=150):
        xd = self._x(x)
        got = self.ops.intensity(xd, num_frame).cpu().numpy()
        np.testing.assert_array_equal(got, self.torch.ops.ss_hip.intensity(xd, num_frame).cpu().numpy())
        return got

    def logmel_bank(self, x, start, w, eps):
        xd, ms, mw = self._x(x), self.torch.from_numpy(start).to(self.dev), self.torch.from_numpy(w).to(self.dev)
        return (self.ops.logmel(xd, ms, mw, eps).cpu().numpy(),
                self.ops.audio_features(xd, ("logmel",), ms, mw, eps)["logmel"].cpu().numpy())


# ---- inputs and comparisons -----------------------------------------------------------------------------------------------
def correlated_ears(rng, n_units, n, delay=7):
    """ear 1 = ear 0 delayed by `delay` samples and scaled by 0.7, plus 10 % noise: GCC-PHAT has a peak to find"""
    base = rng.standard_normal((n_units, n + delay))
    x = np.stack([base[:, delay:], 0.7 * base[:, :n] + 0.1 * rng.standard_normal((n_units, n))], axis=1)
    return x.astype(np.float32)


def err_peak(got, ref):
    """max |got - ref| relative to ref's own peak; shapes equal, no NaN (the host buffers start as NaN: every cell was written)"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    peak = np.abs(ref).max()
    e = np.abs(got - ref).max()
    return float(e / peak) if peak > 0 else float(e)


def oracle(x, sr, n_mels=64, mel_eps=1e-6, max_lag=32, gcc_eps=1e-8, pad="reflect", want=NAMES):
    x = np.asarray(x, np.float64)
    ref = {}
    if "spectrogram" in want:
        ref["spectrogram"] = O.compute_spectrogram(x, pad_mode=pad)
    if "logmel" in want:
        ref["logmel"] = O.compute_logmel(x, sr, n_mels, mel_eps, pad)
    if "gccphat" in want:
        ref["gccphat"] = O.compute_gcc_phat(x, max_lag, gcc_eps, pad)
    return ref


# ---- 1. short rows, both pad modes ----------------------------------------------------------------------------------------
def case_short_rows(be, n):
    rng = np.random.default_rng(1000 + n)
    n_units, sr = 3, 16000
    x = correlated_ears(rng, n_units, n)                    # every unit its own draw: a unit-stride error lands on other data
    x *= np.float32(SHORT_LEVEL)
    x[0] *= 0.25
    x[-1] *= 2.0
    worst = {}
    for pad in PADS:
        kw = dict(mel_eps=1e-6, gcc_eps=SHORT_GCC_EPS, pad=pad)
        refs = [oracle(x[u], sr, **kw) for u in range(n_units)]
        alone = {"spectrogram": be.spectrogram(x, pad), "logmel": be.logmel(x, sr, 64, 1e-6, pad),
                 "gccphat": be.gccphat(x, 32, SHORT_GCC_EPS, pad)}
        outs = [("alone", alone)] + [("features" + "+".join(w[0] for w in want), be.features(x, sr, want, **kw)) for want in SUBSETS]
        for tag, out in outs:
            for name, got in out.items():
                e = max(err_peak(got[u], refs[u][name]) for u in range(n_units))
                worst[(pad, tag, name)] = e
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    print(f"short rows len={n}: worst {max(worst.values()):.2e}")
    assert not bad, f"len={n}: " + ", ".join(f"{k}: {v:.2e}" for k, v in sorted(bad.items()))


@pytest.mark.parametrize("n", SHORT_LENS)
def test_hostsim_short_rows(n):
    assert any(m % 2 for m in SHORT_LENS) and any(m % 4 == 2 for m in SHORT_LENS) and any(m % 4 == 0 for m in SHORT_LENS)
    case_short_rows(Host(gpw=1 if n % 2 else 3), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHORT_LENS)
def test_gpu_short_rows(n):
    case_short_rows(Gpu(), n)


def test_np_pad_reflect_is_the_definition():
    """what the kernels follow: np.pad keeps reflecting with period 2(len-1); one sample is repeated"""
    np.testing.assert_array_equal(np.pad([3.0], 4, mode="reflect"), np.full(9, 3.0))
    np.testing.assert_array_equal(np.pad([1.0, 2.0, 3.0], 5, mode="reflect"), [2, 1, 2, 3, 2, 1, 2, 3, 2, 1, 2, 3, 2])
    x = np.arange(5.0)
    y = np.pad(x, 256, mode="reflect")
    i = np.arange(-256, 5 + 256) % 8
    np.testing.assert_array_equal(y, x[np.where(i < 5, i, 8 - i)])


def case_len_zero_refused(be):
    x = np.zeros((2, 2, 0), np.float32)
    for call in (lambda: be.spectrogram(x), lambda: be.logmel(x, 16000), lambda: be.gccphat(x),
                 lambda: be.features(x, 16000), lambda: be.features(x, 16000, ("gccphat",))):
        with pytest.raises(be.refused[0], match=be.refused[1]):
            call()


def test_hostsim_len_zero_refused():
    case_len_zero_refused(Host())


@pytest.mark.gpu
def test_gpu_len_zero_refused():
    case_len_zero_refused(Gpu())


# ---- 1b. the fused observation routes (waveform rendered and transformed in one launch) on short rows ----------------------
# ss_audio_obs_f32 and its siblings take rows of at least 257 samples (include/ss_hip.h: their centre padding reflects once);
# the right-edge pads of k_conv FUSE / WIDE, k_obs_rows and k_obs_blocks are exercised from that length up, at the lengths
# where the last frame group / the last partition block holds 1, 2, 3 ... samples.  (The GPU test found one: in k_obs_blocks
# a last block of fewer than 257 samples mirrored its right padding out of the previous block's samples while they were still
# being loaded - 5e-3 of the spectrogram's peak at out_len = 16385.)
OBS_LENS_ONE_BLOCK = [n for n in SHORT_LENS if n >= 257]
OBS_LENS_ROWS = [16385, 16386, 16387, 16384 + 159, 16384 + 160, 16384 + 161, 2 * 16384 + 1, 2 * 16384 + 255, 44100]


def _obs_scene(rng, out_len, rir_len):
    src = [rng.standard_normal(out_len + 500).astype(np.float32) for _ in range(2)]
    rirs = []
    for k in range(3):
        h = rng.standard_normal((2, rir_len)) * np.exp(-np.arange(rir_len) / (0.3 * rir_len))[None, :]
        rirs.append(h.astype(np.float32))
    return src, rirs


def _conv_ref(src, rir, t0, out_len, n_valid=None):
    """out[c, t] = sum_k rir[c, k] src[t0 + t - k] in float64 (zero outside the clip), zero from n_valid on"""
    from scipy.signal import fftconvolve
    full = fftconvolve(src.astype(np.float64)[None, :], rir.astype(np.float64), axes=1)[:, t0:t0 + out_len]
    out = np.zeros((2, out_len))
    out[:, :full.shape[1]] = full
    if n_valid is not None:
        out[:, n_valid:] = 0.0
    return out


def _obs_check(tag, ag, sg, src, rirs, units, out_len, pad, n_valid=None):
    worst = 0.0
    for n, (s, t0, r) in enumerate(units):
        ref_a = _conv_ref(src[s], rirs[r], t0, out_len, n_valid)
        if ag is not None:
            worst = max(worst, err_peak(ag[n], ref_a))
        worst = max(worst, err_peak(sg[n], O.compute_spectrogram(ref_a, pad_mode=pad)))
    print(f"{tag} out_len={out_len} pad={pad}: worst {worst:.2e}")
    assert worst <= TOL, (tag, out_len, pad, worst)


@pytest.mark.parametrize("out_len", OBS_LENS_ONE_BLOCK)
def test_hostsim_fused_conv_short_rows(out_len):
    """k_conv with the spectrogram fused, simple and loop form, at the lengths the entry points accept (the host build runs a
    workgroup's lanes one after the other, so it has nothing to say about the in-place pad of shorter rows)"""
    from hostsim import hs
    rng = np.random.default_rng(out_len)
    rir_len = min(out_len, 300)
    src, rirs = _obs_scene(rng, out_len, rir_len)
    bank = np.zeros((3, 2, rir_len), np.float32)
    for k, h in enumerate(rirs):
        bank[k] = h
    units = [(0, 0, 0), (1, 5, 2), (0, 200, 1)]
    ud = [dict(sound=s, t0=t0, rir=r) for s, t0, r in units]
    for pad in PADS:
        for simple in (True, False):
            ag, sg = hs.run(src, bank, [rir_len] * 3, ud, out_len, out_len, fuse=True, want_spectrogram=True,
                            pad_mode=PADS.index(pad), simple=simple)
            _obs_check(f"k_conv fuse simple={simple}", ag, sg, src, rirs, units, out_len, pad)


@pytest.mark.gpu
@pytest.mark.parametrize("out_len", OBS_LENS_ONE_BLOCK + OBS_LENS_ROWS)
def test_gpu_fused_observation_routes_short_rows(out_len):
    """the renderer at "rate" out_len: k_conv FUSE (one block), k_obs_blocks (2-3 blocks; three units fit the chip at one
    workgroup per block, so the launcher picks it over k_obs_rows - that kernel: test_gpu_obs_rows_short_last_block), with and
    without the waveform output; and k_conv WIDE (a short step of a longer row)"""
    import torch
    from ss_amd.renderer import BatchedAudioRenderer, RirBank, UnitRequest
    rng = np.random.default_rng(out_len)
    rir_len = min(out_len, 300) if out_len <= 16384 else 9000
    src, rirs = _obs_scene(rng, out_len, rir_len)
    units = [(0, 0, 0), (1, 5, 2), (0, 200, 1)]
    for pad in PADS:
        steps = (None,) if out_len <= 16384 else (None, 0.25)           # 0.25: n_valid <= one block of a longer row -> WIDE
        for step_time in steps:
            r = BatchedAudioRenderer(out_len, device="cuda:0", pad_mode=pad, step_time=step_time)
            for i, s in enumerate(src):
                r.add_source(f"s{i}", s)
            r.set_rir_bank(RirBank.from_arrays(rirs, "cuda:0"))
            plan = r.plan([UnitRequest(s, t0, k) for s, t0, k in units])
            for want_ag in (True, False):
                ag, sg = r.render(plan, want_audiogoal=want_ag)
                torch.cuda.synchronize()
                _obs_check(f"renderer step={step_time} audiogoal={want_ag}", ag.cpu().numpy() if want_ag else None,
                           sg.cpu().numpy(), src, rirs, units, out_len, pad, r.n_valid)


@pytest.mark.gpu
@pytest.mark.parametrize("out_len,n_units", [(16385, 72), (16384 + 200, 72), (2 * 16384 + 1, 56), (2 * 16384 + 255, 56)])
def test_gpu_obs_rows_short_last_block(out_len, n_units):
    """k_obs_rows itself: the launcher hands a step to k_obs_blocks while rows x blocks fit the chip (one workgroup per CU), so
    the small batches above never reach the row kernel.  Here rows x blocks exceeds the CU count (asserted), the step is not
    cross-faded and every sample is rendered, so k_obs_blocks is declined and the launch is k_obs_rows', with and without the
    waveform output; the last block of every row holds fewer than 257 samples, so its right padding mirrors into the previous
    block's samples."""
    import torch
    from ss_amd.renderer import BatchedAudioRenderer, RirBank, UnitRequest
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = P.ceil_div(out_len, P.KB)
    assert 2 * n_units * nb > n_cus and 0 < out_len - (nb - 1) * P.KB <= 256
    rng = np.random.default_rng(out_len)
    src, rirs = _obs_scene(rng, out_len, 9000)
    units = [(int(rng.integers(0, 2)), int(rng.integers(0, 400)), int(rng.integers(0, 3))) for _ in range(n_units)]
    for pad in PADS:
        r = BatchedAudioRenderer(out_len, device="cuda:0", pad_mode=pad)
        for i, s in enumerate(src):
            r.add_source(f"s{i}", s)
        r.set_rir_bank(RirBank.from_arrays(rirs, "cuda:0"))
        plan = r.plan([UnitRequest(s, t0, k) for s, t0, k in units])
        for want_ag in (True, False):
            ag, sg = r.render(plan, want_audiogoal=want_ag)
            torch.cuda.synchronize()
            _obs_check(f"k_obs_rows audiogoal={want_ag}", ag.cpu().numpy() if want_ag else None, sg.cpu().numpy(), src, rirs,
                       units, out_len, pad, r.n_valid)


@pytest.mark.gpu
def test_gpu_fused_observation_entry_points_refuse_rows_under_257_samples():
    import torch
    from ss_amd import ops
    from ss_amd.renderer import BatchedAudioRenderer, RirBank, UnitRequest
    rng = np.random.default_rng(3)
    src, rirs = _obs_scene(rng, 257, 100)
    r = BatchedAudioRenderer(257, device="cuda:0")
    r.add_source("s", src[0])
    r.set_rir_bank(RirBank.from_arrays(rirs, "cuda:0"))
    plan = r.plan([UnitRequest(0, 0, 0)])
    for out_len in (256, 100, 1):
        ag, sg = torch.empty((1, 2, out_len), device="cuda:0"), torch.empty((1,) + P.spectrogram_shape(out_len), device="cuda:0")
        with pytest.raises(RuntimeError, match="failed: invalid argument"):
            ops.audio_obs_into(r._spec, r.rirs.data, r.rirs.lengths, plan.desc, ag, sg, out_len, out_len, "reflect", flags=plan.flags)


def test_every_fused_observation_entry_point_refuses_rows_under_257_samples():
    """ss_audio_obs_f32 and its *_spec_, *_buckets_ and 32 forms check out_len before they touch a device: SS_EINVAL (-1) below
    257 samples whatever else is passed (dummy pointers: only calls that return from the argument checks are made)"""
    import ctypes
    from ss_amd import _lib
    lib = _lib.load()
    one, null = ctypes.c_void_p(16), None
    bucket = (_lib.SsRirBucket * 1)()
    for out_len in (256, 1, 0):
        assert lib.ss_audio_obs_f32(one, one, one, one, one, one, 1, 512, 256, 1, 256, out_len, out_len, 0, 0, null) == -1
        assert lib.ss_audio_obs32_f32(one, one, one, one, one, one, 1, 512, 256, 1, 256, out_len, out_len, 0, null) == -1
        assert lib.ss_audio_obs_spec_f32(one, one, one, one, one, one, 1, 1, out_len, out_len, 0, 0, null) == -1
        assert lib.ss_audio_obs_buckets_f32(one, bucket, 1, one, one, one, one, 1, out_len, out_len, 0, 0, null) == -1


# ---- 2. level x eps grid --------------------------------------------------------------------------------------------------
def grid_rows():
    rng = np.random.default_rng(77)
    x = correlated_ears(rng, 1, 8000)[0].astype(np.float64)
    return np.stack([(a * x).astype(np.float32) for a in LEVELS])          # all levels = the units of ONE launch


def test_grid_has_a_dominating_eps_and_a_level_where_G_is_about_eps():
    x = grid_rows().astype(np.float64)
    ratios = {}
    for a, xu in zip(LEVELS, x):
        G = np.abs(O.stft(xu[0]) * np.conj(O.stft(xu[1])))
        for eps in GCC_EPS:
            ratios[(a, eps)] = float(np.median(G)) / eps
    assert any(0.1 <= r <= 10 for r in ratios.values()), ratios          # |G| ~ eps: the regulariser's exact size matters
    assert any(r <= 1e-3 for r in ratios.values()), ratios               # eps dominates: the output is G / eps
    assert any(r >= 1e6 for r in ratios.values()), ratios                # ... and the regime the rest of the suite lives in


def case_gcc_grid(be, eps):
    x = grid_rows()
    alone = be.gccphat(x, 32, eps)
    fused = [be.features(x, 16000, want, gcc_eps=eps)["gccphat"] for want in SUBSETS if "gccphat" in want]
    worst = 0.0
    for u, a in enumerate(LEVELS):
        ref = O.compute_gcc_phat(x[u].astype(np.float64), 32, eps)
        for tag, got in [("k_gccphat", alone)] + [("k_features", f) for f in fused]:
            e = err_peak(got[u], ref)                        # relative to THIS unit's own oracle peak
            worst = max(worst, e)
            assert e <= TOL, f"{tag} a={a:g} eps={eps:g}: {e:.2e} of the unit's peak {np.abs(ref).max():.2e}"
    print(f"gcc grid eps={eps:g}: worst {worst:.2e} of the unit's own peak")


def case_logmel_grid(be, eps):
    x = grid_rows()
    alone = be.logmel(x, 16000, 64, eps)
    fused = [be.features(x, 16000, want, mel_eps=eps)["logmel"] for want in SUBSETS if "logmel" in want]
    worst = 0.0
    for u, a in enumerate(LEVELS):
        ref = O.compute_logmel(x[u].astype(np.float64), 16000, 64, eps)
        for tag, got in [("k_logmel", alone)] + [("k_features", f) for f in fused]:
            assert got[u].shape == ref.shape and np.isfinite(got[u]).all()
            e = float(np.abs(got[u] - ref).max())             # log domain, absolute
            worst = max(worst, e)
            assert e <= LOGMEL_ABS, f"{tag} a={a:g} eps={eps:g}: {e:.2e}"
    print(f"logmel grid eps={eps:g}: worst absolute {worst:.2e}")


@pytest.mark.parametrize("eps", GCC_EPS)
def test_hostsim_gccphat_level_eps_grid(eps):
    case_gcc_grid(Host(gpw=2), eps)


@pytest.mark.parametrize("eps", MEL_EPS)
def test_hostsim_logmel_level_eps_grid(eps):
    case_logmel_grid(Host(gpw=2), eps)


@pytest.mark.gpu
@pytest.mark.parametrize("eps", GCC_EPS)
def test_gpu_gccphat_level_eps_grid(eps):
    case_gcc_grid(Gpu(), eps)


@pytest.mark.gpu
@pytest.mark.parametrize("eps", MEL_EPS)
def test_gpu_logmel_level_eps_grid(eps):
    case_logmel_grid(Gpu(), eps)


# ---- 3. structured inputs -------------------------------------------------------------------------------------------------
STRUCT_N = 4000


def _both_ears(left, shift=3, gain=0.5):
    """ear 1 = ear 0 moved `shift` samples later (circularly: an impulse at the last sample stays inside the row), scaled"""
    return np.stack([left, gain * np.roll(left, shift)])


def structured_inputs():
    n, t = STRUCT_N, np.arange(STRUCT_N)
    rng = np.random.default_rng(9)
    out = {}
    for tag, pos in (("first", 0), ("interior", 1234), ("last", n - 1)):
        y = np.zeros(n)
        y[pos] = 1.0
        out["impulse_" + tag] = _both_ears(y, shift=-3 if pos == n - 1 else 3)
    out["dc"] = np.stack([np.full(n, 0.5), np.full(n, 0.25)])
    for k in (0, 1, 128, 255, 256, 100.5):
        out[f"sine_bin{k:g}"] = _both_ears(0.1 * np.cos(2 * np.pi * k * t / 512 + 0.3))
    white = rng.standard_normal(n)
    f = np.fft.rfftfreq(n)
    out["tilt40dB"] = _both_ears(np.fft.irfft(np.fft.rfft(white) * 10.0 ** (-2.0 * f / f[-1]), n))
    return {k: v.astype(np.float32) for k, v in out.items()}


PER_ROW = ("impulse_first", "impulse_interior", "impulse_last", "tilt40dB")


def per_row_error(got, ref):
    """pooled spectrogram [65, T4, 2]: worst |got - ref| / (that frequency row's own peak), and the smallest row peak / global peak"""
    row_peak = np.abs(ref).max(axis=(1, 2))
    ratio = row_peak / row_peak.max()
    assert (ratio >= 1e-2).all(), f"rows {np.nonzero(ratio < 1e-2)[0]} do not qualify (smallest ratio {ratio.min():.2e})"
    return float((np.abs(got - ref).max(axis=(1, 2)) / row_peak).max()), float(ratio.min())


def case_structured(be):
    inputs = structured_inputs()
    names = list(inputs)
    x = np.stack([inputs[k] for k in names])
    sr = 16000
    kw = dict(mel_eps=1e-6, gcc_eps=TONAL_GCC_EPS)
    alone = {"spectrogram": be.spectrogram(x), "logmel": be.logmel(x, sr, 64, 1e-6), "gccphat": be.gccphat(x, 32, TONAL_GCC_EPS)}
    outs = [("alone", alone)] + [("features" + "+".join(w[0] for w in want), be.features(x, sr, want, **kw)) for want in SUBSETS]
    bad = []
    for u, name in enumerate(names):
        ref = oracle(x[u], sr, **kw)
        for tag, out in outs:
            for feat, got in out.items():
                e = err_peak(got[u], ref[feat])
                if not e <= TOL:
                    bad.append((name, tag, feat, e))
            if "spectrogram" in out and name in PER_ROW:
                e, ratio = per_row_error(out["spectrogram"][u], ref["spectrogram"])
                print(f"{name} {tag}: worst per-row error {e:.2e}, smallest row peak / global peak {ratio:.2e}")
                if not e <= TOL:
                    bad.append((name, tag, "spectrogram per row", e))
    assert not bad, bad


def test_hostsim_structured_inputs():
    case_structured(Host(gpw=1))


@pytest.mark.gpu
def test_gpu_structured_inputs():
    case_structured(Gpu())


# ---- 4. parameter edges ---------------------------------------------------------------------------------------------------
def case_max_lag(be):
    rng = np.random.default_rng(11)
    x = correlated_ears(rng, 2, 3000)
    for max_lag in (1, 31, 32):
        got = be.gccphat(x, max_lag, 1e-5)
        fused = be.features(x, 16000, ("gccphat",), max_lag=max_lag, gcc_eps=1e-5)["gccphat"]
        for u in range(2):
            ref = O.compute_gcc_phat(x[u].astype(np.float64), max_lag, 1e-5)
            assert ref.shape == (2 * max_lag + 1, 19)
            assert err_peak(got[u], ref) <= TOL and err_peak(fused[u], ref) <= TOL, max_lag
            assert max_lag < 7 or np.argmax(ref[:, 3]) == max_lag - 7                   # ear 1 lags by 7: peak at lag -7
    for max_lag in (0, 33):                              # include/ss_hip.h: 1 <= max_lag <= 32, SS_EINVAL outside
        with pytest.raises(be.refused[0], match=be.refused[1]):
            be.gccphat(x, max_lag, 1e-5)
        with pytest.raises(be.refused[0], match=be.refused[1]):
            be.features(x, 16000, ("gccphat",), max_lag=max_lag)


def case_n_mels(be):
    rng = np.random.default_rng(12)
    x = correlated_ears(rng, 2, 3000) * np.float32(0.3)
    for sr, n_mels in ((16000, 32), (16000, 64), (16000, 128), (8000, 64), (48000, 32), (8000, 32), (48000, 64)):
        got = be.logmel(x, sr, n_mels, 1e-6)
        outs = [got]
        if n_mels <= 64:                                     # the fused kernel's stated limit (n_mels <= 64)
            outs.append(be.features(x, sr, ("logmel",), n_mels=n_mels)["logmel"])
        else:
            with pytest.raises(be.refused[0], match=be.refused[1]):
                be.features(x, sr, ("logmel",), n_mels=n_mels)
        for u in range(2):
            ref = O.compute_logmel(x[u].astype(np.float64), sr, n_mels, 1e-6)
            for g in outs:
                assert err_peak(g[u], ref) <= TOL, (sr, n_mels, err_peak(g[u], ref))
    with pytest.raises(be.refused[0], match=be.refused[1]):                          # 65 bands: one above the fused kernel's limit
        be.features(x, 16000, ("logmel",), n_mels=65)
    assert be.logmel(x, 16000, 65).shape == (2, 65, 19, 2)   # ... which the stand-alone kernel serves
    # n_mels = 1 (include/ss_hip.h: 1 <= n_mels): one band of the ABI's widest form, 64 bins from bin 100, hand-built
    # (the Slaney bank of ONE band spans all 257 bins, wider than the ABI's max_len: refused)
    start = np.array([100], np.int32)
    w = (np.bartlett(66)[1:65][None, :] / 32.0).astype(np.float32)
    alone, fused = be.logmel_bank(x, start, w, 1e-6)
    for u in range(2):
        p = np.stack([np.abs(O.stft(x[u, c].astype(np.float64))) ** 2 for c in range(2)], axis=-1)     # [257, T, 2]
        ref = np.log(np.einsum("i,itc->tc", w[0].astype(np.float64), p[100:164]) + 1e-6)[None]
        assert err_peak(alone[u], ref) <= TOL and err_peak(fused[u], ref) <= TOL
    assert P.mel_filterbank_sparse(16000, 1)[2] > 64
    with pytest.raises(be.refused[0], match=be.refused[1]):
        be.logmel(x, 16000, 1)


def case_intensity(be):
    rng = np.random.default_rng(13)
    levels = (1e-6, 1e-4, 1e-2, 1.0, 1e2)
    for n in (150, 151, 16000):
        x = rng.standard_normal((len(levels), 2, n))
        x[:, :, : n // 3] *= 0.01                            # a quiet head: the onset is not sample 0
        if n == 16000:
            x[1, :, 15900:] *= 30.0                          # onset 100 samples before the end: fewer than num_frame remain
        x = (x * np.array(levels)[:, None, None]).astype(np.float32)
        got = be.intensity(x)
        for u, a in enumerate(levels):
            ref = float(O.intensity(x[u].astype(np.float64))[0])
            assert ref > 0 and abs(float(got[u]) - ref) <= TOL * ref, (n, a, float(got[u]), ref)


def test_hostsim_max_lag_edges():
    case_max_lag(Host())


def test_hostsim_n_mels_and_rate_edges():
    case_n_mels(Host())


def test_hostsim_intensity_short_rows_and_levels():
    case_intensity(Host())


@pytest.mark.gpu
def test_gpu_max_lag_edges():
    case_max_lag(Gpu())


@pytest.mark.gpu
def test_gpu_n_mels_and_rate_edges():
    case_n_mels(Gpu())


@pytest.mark.gpu
def test_gpu_intensity_short_rows_and_levels():
    case_intensity(Gpu())
