#!/usr/bin/env python
"""Log-mel observation of rows of 2 or 3 partition blocks (44.1 / 48 kHz): the one-launch log-mel form of the fused row kernels
(ss_audio_obs_logmel_rows_f32 / _spec_f32: k_obs_blocks<.., MEL> for small steps, k_obs_rows<.., MEL> beyond) against the route a
context takes without it for the same outputs, into a waveform buffer:
  log-mel alone:                the convolution without its STFT phase (ss_fftconv_binaural_f32 / _spec_f32), then k_features;
  log-mel + pooled spectrogram: k_obs_rows / k_obs_blocks writing the waveform and the spectrogram (ss_audio_obs_f32 / _spec_f32),
                                then k_features (log-mel).
Both bank forms.

Stateless entries through bound ctypes calls (~3 us of host time per launch), HIP events on the launch stream, the arms
ALTERNATING in one process: every round times `--launches` launches of each arm back to back; the table gives the median
and the minimum over the rounds, in us per launch (per pair of launches for the two-launch arms).
usage: python scripts/kbench_obs_logmel_rows.py [--points "44100:1,5,10,42,43,128,512;48000:5,128"] [--rounds 7] [--launches 40]
                                                [--out FILE]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]
import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import _lib, planning as P
from ss_amd.renderer import BatchedAudioRenderer, RirBank

ap = argparse.ArgumentParser()
ap.add_argument("--points", default="44100:1,5,10,42,43,128,512;48000:5,128", help="rate:unit counts;...")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=40, help="launches per arm and round (rounds x launches >= 200 per point)")
ap.add_argument("--bank-mib", type=int, default=512)
ap.add_argument("--sounds", type=int, default=102)
ap.add_argument("--distinct", type=int, default=8, help="pre-planned batches cycled")
ap.add_argument("--n-mels", type=int, default=64)
ap.add_argument("--out", default="")
a = ap.parse_args()

F = ctypes.c_float
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream
EPS = 1e-6
sr = 0


def setup(rate):
    """renderer (sources, window spectra), bank in both forms and mel tables of one rate"""
    global sr, r, R, msd, mwd, max_len, T
    sr = rate
    r = BatchedAudioRenderer(sr, device=dev)
    for i, c in enumerate(O.synth_sources(rng, sr, k=a.sounds)):
        r.add_source(str(i), c)
    R = max(8, (a.bank_mib << 20) // (2 * sr * 4))
    r.set_rir_bank(RirBank(synth_rir_bank_device(torch, R, sr, sr, dev, 3), torch.full((R,), sr, dtype=torch.int32, device=dev)))
    r.rirs.build_spectra()
    ms, mw, max_len = P.mel_filterbank_sparse(sr, a.n_mels)
    msd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(dev)
    mwd = torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(dev)
    T = 1 + sr // 160


def arms(plan, spectral, want_sg, ag, sg, lm):
    """-> (fused, two_launch): callables that issue the launch(es) of one step"""
    n, cap = len(plan), r.rirs.cap
    sgp = sg.data_ptr() if want_sg else None
    mel = (lm.data_ptr(), msd.data_ptr(), mwd.data_ptr(), a.n_mels, int(max_len), F(EPS))
    if spectral:
        head = (r._spec.data_ptr(), r.rirs.spectra.data_ptr(), r.rirs.lengths.data_ptr(), plan.desc.data_ptr())
        tail = (n, r.rirs.spectra.shape[2], r.n_valid, r.out_len)
        f_fn = LIB.ss_audio_obs_logmel_rows_spec_f32
        c_fn = LIB.ss_audio_obs_spec_f32 if want_sg else LIB.ss_fftconv_binaural_spec_f32
    else:
        head = (r._spec.data_ptr(), r.rirs.data.data_ptr(), r.rirs.lengths.data_ptr(), plan.desc.data_ptr())
        tail = (n, 2 * cap, cap, 1, cap, r.n_valid, r.out_len)
        f_fn = LIB.ss_audio_obs_logmel_rows_f32
        c_fn = LIB.ss_audio_obs_f32 if want_sg else LIB.ss_fftconv_binaural_f32
    fa = head + (None, sgp) + mel + tail + (0, plan.flags, STREAM)
    if want_sg:                                          # waveform + spectrogram from the fused row kernels (pad_mode 0)
        ca = head + (ag.data_ptr(), sgp) + tail + (0, plan.flags, STREAM)
    else:                                                # the convolution alone
        ca = head + (ag.data_ptr(),) + tail + (plan.flags, STREAM)
    ka = (ag.data_ptr(), n, sr, 0, None) + mel + (None, 1, F(1.0), STREAM)       # k_features: log-mel of the waveform

    def fused():
        assert f_fn(*fa) == 0

    def two():
        assert c_fn(*ca) == 0
        assert LIB.ss_audio_features_f32(*ka) == 0
    return fused, two


def spin_up(fn, ms=60.0):
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < ms * 1e-3:
        for _ in range(16):
            fn(k); k += 1
        torch.cuda.synchronize()


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


lines = [f"# kbench_obs_logmel_rows: {a.n_mels} bands, bank {a.bank_mib} MiB per rate, {a.sounds} sounds, "
         f"{a.rounds} rounds x {a.launches} launches per arm, arms alternating; us per step: median (min)",
         f"{'rate':>6s} {'units':>5s} {'bank':>8s} {'outputs':>10s} {'fused':>16s} {'two launches':>16s} {'fused/two':>9s}"]
print("\n".join(lines), flush=True)
first = True
points = []
for part in a.points.split(";"):
    rate, sizes = part.split(":")
    points += [(int(rate), int(x)) for x in sizes.split(",")]
for rate, N in points:
    if rate != sr:
        setup(rate)
    plans = [r.plan_arrays(rng.integers(0, a.sounds, N), np.zeros(N, np.int64), rng.integers(0, R, N)) for _ in range(a.distinct)]
    ag = torch.empty((N, 2, sr), device=dev)
    sg = torch.empty((N,) + r.spectrogram_shape, device=dev)
    lm = torch.empty((N, a.n_mels, T, 2), device=dev)
    for spectral in (False, True):
        for want_sg in (False, True):
            pairs = [arms(p, spectral, want_sg, ag, sg, lm) for p in plans]
            fa = lambda k: pairs[k % a.distinct][0]()
            fb = lambda k: pairs[k % a.distinct][1]()
            if first:
                spin_up(fb)
                first = False
            for k in range(4):
                fa(k); fb(k)
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(a.rounds):
                ta.append(timed(fa, a.launches))
                tb.append(timed(fb, a.launches))
            ma, mb = float(np.median(ta)), float(np.median(tb))
            line = (f"{sr:6d} {N:5d} {'spectral' if spectral else 'time':>8s} {'mel+sgram' if want_sg else 'mel':>10s} "
                    f"{ma:8.1f} ({min(ta):5.1f}) {mb:8.1f} ({min(tb):5.1f}) {ma / mb:9.3f}")
            lines.append(line)
            print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
