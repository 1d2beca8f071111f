#!/usr/bin/env python
"""Half-precision time-domain RIR rows: kernel time per launch of three bank forms on identical inputs, in one process per rate -
fp32 time-domain rows (ss_audio_obs_f32 / ss_fftconv_binaural_f32: the comparison point), half rows (ss_audio_obs_rir16_f32 /
ss_fftconv_binaural_rir16_f32, k_conv<.., HALF>) and half spectra (ss_audio_obs_spec16_f32 / ss_fftconv_binaural_spec16_f32).

  16 kHz    the fused observation (spectrogram, no waveform buffer) and the convolution alone, at 5 / 32 / 128 / 2 048 units
  44.1 kHz  the unfused convolution (three output blocks), at 5 / 128 units

The three banks hold the same RIRs (both half forms are quantised from the rows the fp32 arm reads).  Every launch of an arm
reads entries no earlier launch of the timed window has read since the whole bank went by (launch k takes the N entries behind
those of launch k - 1, modulo the bank, in every arm alike), so a row's read comes from HBM at every size; the window spectra
of the sounds are cache hits in every arm, as in the product.  Stateless entries through bound ctypes calls, HIP events on the
launch stream, the arms ALTERNATING after a warm-up of the shape; the table gives the median and the minimum over the rounds in
us per launch and the ratio to the fp32 rows.  The half-rows output is compared with the fp32 arm's once per point (max
|difference| over the fp32 arm's peak: the format's error, not a rounding difference).

Without --rate the script is a driver: one child process per rate, each under its own time limit, and it stops at the first one
that fails.  usage: python scripts/kbench_rir16.py [--out FILE] [--rounds 7] [--launches 30] [--step-timeout 240]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--rate", type=int, default=0, help="16000 or 44100: run that step in this process (default: drive both)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=30, help="launches per arm and round (rounds x launches >= 200 per point)")
ap.add_argument("--bank-mib", type=int, default=1024, help="size of the fp32 time-domain bank")
ap.add_argument("--sounds", type=int, default=102)
ap.add_argument("--warm", type=int, default=8, help="warm-up launches per arm and point")
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a rate's child process may take")
ap.add_argument("--out", default="")
a = ap.parse_args()

if not a.rate:                                                           # the driver: a fresh child per rate, each with its own limit
    text = []
    for rate in (16000, 44100):
        cmd = [sys.executable, os.path.abspath(__file__), "--rate", str(rate), "--rounds", str(a.rounds), "--launches", str(a.launches),
               "--bank-mib", str(a.bank_mib), "--sounds", str(a.sounds), "--warm", str(a.warm)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"kbench_rir16: the {rate} Hz step ran past {a.step_timeout} s: stopping", file=sys.stderr)
            sys.exit(124)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:                                            # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stderr[-4000:])
            print(f"kbench_rir16: the {rate} Hz step failed with status {p.returncode}: stopping", file=sys.stderr)
            sys.exit(p.returncode if p.returncode > 0 else 1)
        text.append(p.stdout)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(text))
    sys.exit(0)

import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import _lib, ops
from ss_amd.renderer import BatchedAudioRenderer, RirBank

assert torch.cuda.is_available(), "kbench_rir16 needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
sr = a.rate
fused_rate = sr <= ops.KB
rng = np.random.default_rng(0)
r = BatchedAudioRenderer(sr, device=dev)
for i, c in enumerate(O.synth_sources(rng, sr, k=a.sounds)):
    r.add_source(str(i), c)
cap = sr + (sr & 1)
R = max(8, (a.bank_mib << 20) // (2 * cap * 4))
rows = synth_rir_bank_device(torch, R, sr, cap, dev, 3)
lengths = torch.full((R,), sr, dtype=torch.int32, device=dev)
r.set_rir_bank(RirBank(rows, lengths))
q16, qsc = ops.rir_rows16(rows)
h16, hsc = ops.rir_spectra16(rows)
hb = int(h16.shape[2])
torch.cuda.synchronize()
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream


def arms(plan, out, fused):
    """-> the three bound launches of one plan: fp32 rows, half rows, half spectra"""
    n = len(plan)
    sp, ln, ds, o = r._spec.data_ptr(), lengths.data_ptr(), plan.desc.data_ptr(), out.data_ptr()
    if fused:
        c32 = (LIB.ss_audio_obs_f32, (sp, rows.data_ptr(), ln, ds, None, o, n, 2 * cap, cap, 1, cap, r.n_valid, r.out_len, 0, plan.flags, STREAM))
        c16 = (LIB.ss_audio_obs_rir16_f32, (sp, q16.data_ptr(), qsc.data_ptr(), ln, ds, None, o, n, cap, r.n_valid, r.out_len, 0, plan.flags, STREAM))
        s16 = (LIB.ss_audio_obs_spec16_f32, (sp, h16.data_ptr(), hsc.data_ptr(), ln, ds, None, o, n, hb, r.n_valid, r.out_len, 0, plan.flags, STREAM))
    else:
        c32 = (LIB.ss_fftconv_binaural_f32, (sp, rows.data_ptr(), ln, ds, o, n, 2 * cap, cap, 1, cap, r.n_valid, r.out_len, plan.flags, STREAM))
        c16 = (LIB.ss_fftconv_binaural_rir16_f32, (sp, q16.data_ptr(), qsc.data_ptr(), ln, ds, o, n, cap, r.n_valid, r.out_len, plan.flags, STREAM))
        s16 = (LIB.ss_fftconv_binaural_spec16_f32, (sp, h16.data_ptr(), hsc.data_ptr(), ln, ds, o, n, hb, r.n_valid, r.out_len, plan.flags, STREAM))

    def bind(f, args):
        def call():
            assert f(*args) == 0
        return call
    return bind(*c32), bind(*c16), bind(*s16)


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


print(f"# kbench_rir16 {sr} Hz, {torch.cuda.get_device_name(0)}; {R} entries of {cap} samples: fp32 rows {rows.numel() * 4 >> 20} MiB, "
      f"half rows {q16.numel() * 2 >> 20} MiB + {qsc.numel() * 4 >> 10} KiB of scales, half spectra {h16.numel() * 2 >> 20} MiB; "
      f"{a.sounds} sounds, {a.rounds} rounds x {a.launches} launches per arm, arms alternating, every launch reads bank entries not read "
      f"since the whole bank went by; us per launch: median (min)", flush=True)
print(f"{'kernel':>6s} {'units':>5s} {'fp32 rows':>16s} {'half rows':>16s} {'half spectra':>16s} {'rows16/fp32':>11s} {'spec16/fp32':>11s} "
      f"{'rows16 diff/peak':>16s}", flush=True)
points = [(True, n) for n in (5, 32, 128, 2048)] + [(False, n) for n in (5, 32, 128, 2048)] if fused_rate else [(False, 5), (False, 128)]
walk = 0
spun = False
for fused, N in points:
    n_plans = a.warm + 1 + a.rounds * a.launches                         # one plan per launch of an arm: no entry is read twice
    plans = []
    for _ in range(n_plans):
        plans.append(r.plan_arrays(rng.integers(0, a.sounds, N), np.zeros(N, np.int64), (walk + np.arange(N)) % R))
        walk = (walk + N) % R
    out = torch.empty(((N,) + r.spectrogram_shape) if fused else (N, 2, r.out_len), device=dev)
    trip = [arms(p, out, fused) for p in plans]
    if not spun:                                                         # clocks up before the first timed window
        t0, k = time.perf_counter(), 0
        while time.perf_counter() - t0 < 0.06:
            trip[k % a.warm][0](); k += 1
        torch.cuda.synchronize()
        spun = True
    for k in range(a.warm):                                              # the shape of the timed window, every arm
        for arm in range(3):
            trip[k][arm]()
    torch.cuda.synchronize()
    trip[a.warm][0](); ref = out.clone()
    trip[a.warm][1](); got = out.clone()
    torch.cuda.synchronize()
    diff = float((got - ref).abs().max() / ref.abs().max())
    t = [[], [], []]
    for rd in range(a.rounds):
        k0 = a.warm + 1 + rd * a.launches
        for arm in range(3):
            t[arm].append(timed(lambda k: trip[k0 + k][arm](), a.launches))
    m = [float(np.median(x)) for x in t]
    print(f"{'fused' if fused else 'conv':>6s} {N:5d} " + " ".join(f"{m[i]:8.1f} ({min(t[i]):5.1f})" for i in range(3)) +
          f" {m[1] / m[0]:11.3f} {m[2] / m[0]:11.3f} {diff:16.2e}", flush=True)
