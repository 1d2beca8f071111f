#!/usr/bin/env python
"""Half-precision time-domain RIR rows in length buckets: kernel time per 16 kHz step (the fused observation, spectrogram only) of
three arms on identical units, in one process:

  (a) fp32 length buckets      ss_audio_obs_buckets_f32 on ss_rir_bucket[] without spectra (k_conv, loop kernel; bucket-0 steps: the
                               loop-free kernel)
  (b) half rows, one capacity  ss_audio_obs_rir16_f32 on ONE allocation at the longest bucket's capacity (what rir_rows="half" could
                               do before: every entry pays 65 536 samples; k_conv<.., HALF>, loop kernel at this capacity)
  (c) half rows in buckets     ss_audio_obs_rir16_buckets_f32 (k_conv<.., HALF, RBK>; bucket-0 steps: the loop-free half kernel)

over the capacities of the engine's example buckets, 16 000 / 49 152 / 65 536 samples - with more entries per bucket than the
example (8192 / 1024 / 512), so that every bucket in every form is larger than the caches - for two kinds of step at 5, 32 and 128
units: MIXED (about 10 % of the units, at least one, outside bucket 0, alternating between the two long buckets) and BUCKET 0 (every
unit in bucket 0; arms (a) and (c) carry SS_FLAG_FIRST_BUCKET as a context's planner would set it).  The three banks hold the same
RIRs: (b) and (c) the same halves and scales, quantised per row from the rows (a) reads; every entry is as long as its bucket.
Launch k of an arm takes the entries behind those of launch k - 1 in every bucket, modulo the bucket, in every arm alike, so every
row is read from HBM; the window spectra of the sounds are cache hits in every arm, as in the product.  Stateless entries through
bound ctypes calls, HIP events on the launch stream, the arms ALTERNATING after a warm-up of the shape; the table gives the median
and the minimum over the rounds in us per step and the ratios (c)/(a), (c)/(b).  (c)'s spectrogram is compared with (b)'s once per
point (the same halves: 0 expected).

usage: python scripts/kbench_rir16_buckets.py [--out FILE] [--rounds 7] [--launches 30]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=30, help="steps per arm and round (rounds x launches >= 200 per point)")
ap.add_argument("--slots", default="8192,1024,512", help="entries per bucket")
ap.add_argument("--caps", default="16000,49152,65536", help="samples per row of each bucket")
ap.add_argument("--sounds", type=int, default=102)
ap.add_argument("--warm", type=int, default=8, help="warm-up steps per arm and point")
ap.add_argument("--units", default="5,32,128")
ap.add_argument("--out", default="")
a = ap.parse_args()

import ctypes

import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import _lib, ops
from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank

assert torch.cuda.is_available(), "kbench_rir16_buckets needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
sr = 16000
rng = np.random.default_rng(0)
slots = [int(x) for x in a.slots.split(",")]
caps = [int(x) for x in a.caps.split(",")]
assert len(slots) == len(caps) == 3 and caps == sorted(caps) and all(c % 2 == 0 for c in caps)
first = [0, slots[0], slots[0] + slots[1]]
total = sum(slots)
r = BatchedAudioRenderer(sr, device=dev)
for i, c in enumerate(O.synth_sources(rng, sr, k=a.sounds)):
    r.add_source(str(i), c)
lengths = torch.cat([torch.full((n,), c, dtype=torch.int32, device=dev) for n, c in zip(slots, caps)])
views = [lengths[f:f + n] for f, n in zip(first, slots)]
rows = [synth_rir_bank_device(torch, n, sr, c, dev, 3 + b) for b, (n, c) in enumerate(zip(slots, caps))]
halves = [ops.rir_rows16(x) for x in rows]
bank32 = BucketedRirBank([RirBank(x, v) for x, v in zip(rows, views)], lengths, first)
bank16 = BucketedRirBank([RirBank(q, v, scales=s) for (q, s), v in zip(halves, views)], lengths, first)
one_q = torch.zeros((total, 2, caps[-1]), dtype=torch.float16, device=dev)       # the same halves at ONE capacity, zero behind
one_s = torch.cat([s for _, s in halves]).contiguous()
for (q, _), f, n, c in zip(halves, first, slots, caps):
    one_q[f:f + n, :, :c] = q
r.set_rir_bank(bank16)                                                         # planning depth: the deepest bucket, every arm
arr32, arr16 = bank32.c_array(False), bank16.rir16_c_array()
torch.cuda.synchronize()
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream
NAMES = ("(a) fp32 buckets", "(b) half, one cap", "(c) half buckets")


def arms(plan, sg, bucket0):
    n = len(plan)
    sp, ln, ds, o = r._spec.data_ptr(), lengths.data_ptr(), plan.desc.data_ptr(), sg.data_ptr()
    nv, ol = r.n_valid, r.out_len
    fl = plan.flags | (ops.FLAG_FIRST_BUCKET if bucket0 else 0)
    p32, p16 = ctypes.cast(arr32, ctypes.c_void_p), ctypes.cast(arr16, ctypes.c_void_p)

    def fp32():
        assert LIB.ss_audio_obs_buckets_f32(sp, p32, 3, ln, ds, None, o, n, nv, ol, 0, fl, STREAM) == 0

    def one():
        assert LIB.ss_audio_obs_rir16_f32(sp, one_q.data_ptr(), one_s.data_ptr(), ln, ds, None, o, n, caps[-1], nv, ol, 0, plan.flags, STREAM) == 0

    def bk16():
        assert LIB.ss_audio_obs_rir16_buckets_f32(sp, p16, 3, ln, ds, None, o, n, nv, ol, 0, fl, STREAM) == 0
    return fp32, one, bk16


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


def bank_bytes(form):
    if form == 0:
        return sum(n * 8 * c for n, c in zip(slots, caps))
    if form == 1:
        return total * (4 * caps[-1] + 8)
    return sum(n * (4 * c + 8) for n, c in zip(slots, caps))


emit(f"# kbench_rir16_buckets {sr} Hz, {torch.cuda.get_device_name(0)}; buckets of {slots} entries x {caps} samples: fp32 buckets "
     f"{bank_bytes(0) >> 20} MiB, half rows at one capacity {bank_bytes(1) >> 20} MiB, half buckets {bank_bytes(2) >> 20} MiB; "
     f"{a.sounds} sounds, {a.rounds} rounds x {a.launches} steps per arm, arms alternating, every step reads entries not read since "
     f"their whole bucket went by; spectrogram only; us per step: median (min)")
emit(f"{'step':>8s} {'units':>5s} {'outside':>7s} " + " ".join(f"{nm:>17s}" for nm in NAMES) + f" {'c/a':>6s} {'c/b':>6s} {'c vs b diff/peak':>16s}")
walk = [0, 0, 0]
spun = False
for kind in ("mixed", "bucket0"):
    for N in [int(x) for x in a.units.split(",")]:
        n_out = 0 if kind == "bucket0" else max(1, int(round(N / 10)))
        n_plans = a.warm + 1 + a.rounds * a.launches                     # one plan per step of an arm
        plans = []
        for _ in range(n_plans):
            idx = np.empty(N, np.int64)
            for u in range(N):
                b = 0 if u >= n_out else 1 + (u & 1)
                idx[u] = first[b] + walk[b]
                walk[b] = (walk[b] + 1) % slots[b]
            plans.append(r.plan_arrays(rng.integers(0, a.sounds, N), np.zeros(N, np.int64), rng.permutation(idx)))
        sg = torch.empty((N,) + r.spectrogram_shape, device=dev)
        trio = [arms(p, sg, kind == "bucket0") for p in plans]
        if not spun:                                                     # clocks up before the first timed window
            t0, k = time.perf_counter(), 0
            while time.perf_counter() - t0 < 0.06:
                trio[k % a.warm][0](); k += 1
            torch.cuda.synchronize()
            spun = True
        for k in range(a.warm):                                          # the shape of the timed window, every arm
            for arm in range(3):
                trio[k][arm]()
        torch.cuda.synchronize()
        trio[a.warm][1](); ref = sg.clone()
        trio[a.warm][2](); got = sg.clone()
        torch.cuda.synchronize()
        diff = float((got - ref).abs().max() / ref.abs().max())
        t = [[], [], []]
        for rd in range(a.rounds):
            k0 = a.warm + 1 + rd * a.launches
            for arm in range(3):
                t[arm].append(timed(lambda k: trio[k0 + k][arm](), a.launches))
        m = [float(np.median(x)) for x in t]
        emit(f"{kind:>8s} {N:5d} {n_out:7d} " + " ".join(f"{m[i]:9.1f} ({min(t[i]):5.1f})" for i in range(3)) +
             f" {m[2] / m[0]:6.3f} {m[2] / m[1]:6.3f} {diff:16.2e}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
