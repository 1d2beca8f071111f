#!/usr/bin/env python
"""Spectral length buckets: ONE mixed-bucket fused 16 kHz observation launch (spectrogram, no waveform buffer) from the three
forms of the same length-bucketed bank, at 16 and 128 units:

  half   fp16 block spectra + scales   ss_audio_obs_spec_buckets_f32, k_conv_spec<.., HALF, HBK>
  only   fp32 block spectra, no rows   ss_audio_obs_spec_buckets_f32, k_conv_spec (the kernel of the both-forms bank)
  both   rows + fp32 block spectra     ss_audio_obs_buckets_f32

Four buckets of 1 / 2 / 3 / 5 partition blocks (caps 16384 / 32768 / 49152 / 81920 samples) with --entries 1024,256,128,64
entries (x --scale); every entry is as long as its cap and the clips are 6 s long and heard at t0 = 5 s, so every block of a
row is multiplied.  A launch of N units takes N/2, N/4, N/8, N/8 units from the four buckets; launch k reads the entries
behind those of launch k - 1 in every bucket (modulo the bucket), in all three arms alike, so a row's read comes from HBM
once the bank is larger than the caches (the default half bank is 560 MiB, the fp32 ones 1120 MiB).  Stateless entries through
bound ctypes calls, HIP events on the launch stream, the arms ALTERNATING in one process after a warm-up of the shape: every
round times `--launches` launches of each arm back to back; the table gives the median and the minimum over the rounds in us per
launch and the ratios to the both-forms bank.  The outputs are compared once per size (only against both: bit for bit; half
against both: the format's error).
usage: python scripts/kbench_spec_buckets.py [--sizes 16,128] [--rounds 9] [--launches 30] [--scale 2] [--out FILE]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]
import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import _lib, ops, planning as P
from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="16,128")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--launches", type=int, default=30, help="launches per arm and round")
ap.add_argument("--entries", default="1024,256,128,64", help="entries per bucket, before --scale")
ap.add_argument("--scale", type=int, default=2)
ap.add_argument("--sounds", type=int, default=16)
ap.add_argument("--warm", type=int, default=8, help="warm-up launches per arm and size")
ap.add_argument("--out", default="")
a = ap.parse_args()

assert torch.cuda.is_available(), "kbench_spec_buckets needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
sr = 16000
CAPS = [P.KB, 2 * P.KB, 3 * P.KB, 5 * P.KB]
COUNTS = [int(x) * a.scale for x in a.entries.split(",")]
FIRST = [int(v) for v in np.cumsum([0] + COUNTS[:-1])]
SHARE = [2, 4, 8, 8]                                                     # a launch takes N / SHARE[b] units from bucket b
rng = np.random.default_rng(0)
r = BatchedAudioRenderer(sr, device=dev)
for i, c in enumerate(O.synth_sources(rng, sr, k=a.sounds, seconds=6)):
    r.add_source(str(i), c)
lengths = torch.cat([torch.full((n,), cap, dtype=torch.int32, device=dev) for n, cap in zip(COUNTS, CAPS)])
both, only, half = [], [], []
for b, (n, cap) in enumerate(zip(COUNTS, CAPS)):
    view = lengths[FIRST[b]:FIRST[b] + n]
    rows = synth_rir_bank_device(torch, n, sr, cap, dev, 3 + b)
    bank = RirBank(rows, view)
    bank.spectra = ops.rir_spectra(rows)
    both.append(bank)
    o = RirBank(torch.zeros((n, 2, 0), dtype=torch.float32, device=dev), view, cap=cap)
    o.spectra = bank.spectra
    only.append(o)
    h = RirBank(torch.zeros((n, 2, 0), dtype=torch.float32, device=dev), view, cap=cap)
    h.spectra, h.scales = ops.rir_spectra16(rows)
    half.append(h)
torch.cuda.synchronize()
both, only, half = (BucketedRirBank(x, lengths, FIRST) for x in (both, only, half))
r.set_rir_bank(both)
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream
ARR = dict(both=both.c_array(True), only=only.spec_c_array(), half=half.spec_c_array())
NAMES = ("half", "only", "both")


def arms(plan, sg):
    tail = (4, lengths.data_ptr(), plan.desc.data_ptr(), None, sg.data_ptr(), len(plan), r.n_valid, r.out_len, 0, plan.flags, STREAM)

    def arm(name):
        fn = LIB.ss_audio_obs_buckets_f32 if name == "both" else LIB.ss_audio_obs_spec_buckets_f32
        args = (r._spec.data_ptr(), ctypes.cast(ARR[name], ctypes.c_void_p)) + tail

        def run():
            assert fn(*args) == 0
        return run
    return {name: arm(name) for name in NAMES}


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


def mib(banks, scales=False):
    return sum(b.spectra.numel() * b.spectra.element_size() + (b.scales.numel() * 4 if scales else 0) for b in banks.banks) >> 20


lines = [f"# kbench_spec_buckets: fused 16 kHz observation (spectrogram, no waveform buffer) over 4 length buckets of 1/2/3/5 blocks, "
         f"{torch.cuda.get_device_name(0)}; entries {COUNTS}: half {mib(half, True)} MiB, only {mib(only)} MiB, both {mib(both)} MiB of "
         f"spectra + {sum(b.data.numel() * 4 for b in both.banks) >> 20} MiB of rows; {a.sounds} 6-s sounds at t0 = 5 s, {a.rounds} rounds x "
         f"{a.launches} launches per arm, arms alternating; us per launch: median (min)",
         f"{'units':>5s} {'half':>16s} {'only':>16s} {'both':>16s} {'half/both':>9s} {'only/both':>9s} {'half diff/peak':>15s} {'only == both':>12s}"]
print("\n".join(lines), flush=True)
walk = [0, 0, 0, 0]
for N in [int(x) for x in a.sizes.split(",")]:
    n_plans = a.warm + 1 + a.rounds * a.launches
    plans = []
    for _ in range(n_plans):
        rir = []
        for b in range(4):
            k = max(1, N // SHARE[b])
            rir.append(FIRST[b] + (walk[b] + np.arange(k)) % COUNTS[b])
            walk[b] = (walk[b] + k) % COUNTS[b]
        rir = rng.permutation(np.concatenate(rir))[:N]
        plans.append(r.plan_arrays(rng.integers(0, a.sounds, len(rir)), np.full(len(rir), 5 * sr, np.int64), rir))
    sg = torch.empty((len(plans[0]),) + r.spectrogram_shape, device=dev)
    runs = [arms(p, sg) for p in plans]
    for k in range(a.warm):
        for name in NAMES:
            runs[k][name]()
    torch.cuda.synchronize()
    got = {}
    for name in NAMES:
        runs[a.warm][name]()
        got[name] = sg.clone()
    torch.cuda.synchronize()
    diff = float((got["half"] - got["both"]).abs().max() / got["both"].abs().max())
    same = bool(torch.equal(got["only"], got["both"]))
    t = {name: [] for name in NAMES}
    for rd in range(a.rounds):
        k0 = a.warm + 1 + rd * a.launches
        for name in NAMES:
            t[name].append(timed(lambda k: runs[k0 + k][name](), a.launches))
    m = {name: float(np.median(t[name])) for name in NAMES}
    line = (f"{len(plans[0]):5d} " + " ".join(f"{m[name]:8.1f} ({min(t[name]):5.1f})" for name in NAMES) +
            f" {m['half'] / m['both']:9.3f} {m['only'] / m['both']:9.3f} {diff:15.2e} {str(same):>12s}")
    lines.append(line)
    print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
