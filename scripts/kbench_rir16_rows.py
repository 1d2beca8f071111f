#!/usr/bin/env python
"""Half-precision time-domain RIR rows under the fused 44.1 kHz row kernels: kernel time per step of four arms on identical
inputs, in one process - three-block rows (44 100 samples, RIRs of 44 100 taps), with and without a waveform buffer:

  (a) half rows, fused     ss_audio_obs_rows_rir16_f32: k_obs_blocks / k_obs_rows <.., ROWS16>, one launch (what a context bound by
                           ss_ctx_set_rir_bank16_rows runs)
  (b) half rows, 2 launch  ss_fftconv_binaural_rir16_f32 into a waveform buffer + ss_spectrogram_f32 over it (what a context bound
                           by ss_ctx_set_rir_bank16 runs: the caller's buffer or, without one, its hand-over buffer)
  (c) fp32 rows            ss_audio_obs_f32: k_obs_blocks / k_obs_rows on the time-domain bank
  (d) half spectra         ss_audio_obs_rows_spec16_f32: the half forms of the row kernels on fp16 block spectra

at 5, 10, 42, 43 (either side of k_obs_blocks' budget of one workgroup per CU), 128 and 512 units.  The three banks hold the same
RIRs (both half forms are quantised from the rows the fp32 arm reads) and are larger than the caches; launch k of an arm takes
the N entries behind those of launch k - 1, modulo the bank, in every arm alike, so a row's read comes from HBM at every size;
the window spectra of the sounds are cache hits in every arm, as in the product.  Stateless entries through bound ctypes calls,
HIP events on the launch stream, the arms ALTERNATING after a warm-up of the shape; the table gives the median and the minimum
over the rounds in us per step and the ratios (a)/(b), (a)/(c), (a)/(d).  (a)'s spectrogram is compared with (b)'s once per point.

usage: python scripts/kbench_rir16_rows.py [--out FILE] [--rounds 7] [--launches 30]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=30, help="steps per arm and round (rounds x launches >= 200 per point)")
ap.add_argument("--bank-mib", type=int, default=1024, help="size of the fp32 time-domain bank")
ap.add_argument("--sounds", type=int, default=102)
ap.add_argument("--warm", type=int, default=8, help="warm-up steps per arm and point")
ap.add_argument("--units", default="5,10,42,43,128,512")
ap.add_argument("--out", default="")
a = ap.parse_args()

import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import _lib, ops
from ss_amd.renderer import BatchedAudioRenderer, RirBank

assert torch.cuda.is_available(), "kbench_rir16_rows needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
sr = 44100
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
NAMES = ("(a) half fused", "(b) half 2-launch", "(c) fp32 rows", "(d) half spectra")


def arms(plan, wave, hand, sg, want_wave):
    """-> the four bound steps of one plan.  wave: the caller's waveform buffer (want_wave), hand: arm (b)'s hand-over buffer"""
    n = len(plan)
    sp, ln, ds, o = r._spec.data_ptr(), lengths.data_ptr(), plan.desc.data_ptr(), sg.data_ptr()
    ag = wave.data_ptr() if want_wave else None
    mid = wave.data_ptr() if want_wave else hand.data_ptr()
    nv, ol, fl = r.n_valid, r.out_len, plan.flags

    def fused16():
        assert LIB.ss_audio_obs_rows_rir16_f32(sp, q16.data_ptr(), qsc.data_ptr(), ln, ds, ag, o, n, cap, nv, ol, 0, fl, STREAM) == 0

    def two16():
        assert LIB.ss_fftconv_binaural_rir16_f32(sp, q16.data_ptr(), qsc.data_ptr(), ln, ds, mid, n, cap, nv, ol, fl, STREAM) == 0
        assert LIB.ss_spectrogram_f32(mid, o, n, ol, 0, STREAM) == 0

    def rows32():
        assert LIB.ss_audio_obs_f32(sp, rows.data_ptr(), ln, ds, ag, o, n, 2 * cap, cap, 1, cap, nv, ol, 0, fl, STREAM) == 0

    def spec16():
        assert LIB.ss_audio_obs_rows_spec16_f32(sp, h16.data_ptr(), hsc.data_ptr(), ln, ds, ag, o, n, hb, nv, ol, 0, fl, STREAM) == 0
    return fused16, two16, rows32, spec16


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


emit(f"# kbench_rir16_rows {sr} Hz, {torch.cuda.get_device_name(0)}; {R} entries of {cap} samples (3 partition blocks): fp32 rows "
     f"{rows.numel() * 4 >> 20} MiB, half rows {q16.numel() * 2 >> 20} MiB + {qsc.numel() * 4 >> 10} KiB of scales, half spectra "
     f"{h16.numel() * 2 >> 20} MiB; {a.sounds} sounds, {a.rounds} rounds x {a.launches} steps per arm, arms alternating, every step "
     f"reads bank entries not read since the whole bank went by; us per step: median (min)")
emit(f"{'waveform':>8s} {'units':>5s} " + " ".join(f"{nm:>17s}" for nm in NAMES) + f" {'a/b':>6s} {'a/c':>6s} {'a/d':>6s} {'a vs b diff/peak':>16s}")
walk = 0
spun = False
for want_wave in (False, True):
    for N in [int(x) for x in a.units.split(",")]:
        n_plans = a.warm + 1 + a.rounds * a.launches                     # one plan per step of an arm: no entry is read twice
        plans = []
        for _ in range(n_plans):
            plans.append(r.plan_arrays(rng.integers(0, a.sounds, N), np.zeros(N, np.int64), (walk + np.arange(N)) % R))
            walk = (walk + N) % R
        sg = torch.empty((N,) + r.spectrogram_shape, device=dev)
        wave = torch.empty((N, 2, r.out_len), device=dev)
        hand = torch.empty((N, 2, r.out_len), device=dev)
        quad = [arms(p, wave, hand, sg, want_wave) for p in plans]
        if not spun:                                                     # clocks up before the first timed window
            t0, k = time.perf_counter(), 0
            while time.perf_counter() - t0 < 0.06:
                quad[k % a.warm][2](); k += 1
            torch.cuda.synchronize()
            spun = True
        for k in range(a.warm):                                          # the shape of the timed window, every arm
            for arm in range(4):
                quad[k][arm]()
        torch.cuda.synchronize()
        quad[a.warm][1](); ref = sg.clone()
        quad[a.warm][0](); got = sg.clone()
        torch.cuda.synchronize()
        diff = float((got - ref).abs().max() / ref.abs().max())
        t = [[], [], [], []]
        for rd in range(a.rounds):
            k0 = a.warm + 1 + rd * a.launches
            for arm in range(4):
                t[arm].append(timed(lambda k: quad[k0 + k][arm](), a.launches))
        m = [float(np.median(x)) for x in t]
        emit(f"{'yes' if want_wave else 'no':>8s} {N:5d} " + " ".join(f"{m[i]:9.1f} ({min(t[i]):5.1f})" for i in range(4)) +
             f" {m[0] / m[1]:6.3f} {m[0] / m[2]:6.3f} {m[0] / m[3]:6.3f} {diff:16.2e}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
