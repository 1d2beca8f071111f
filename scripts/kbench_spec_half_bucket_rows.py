#!/usr/bin/env python
"""Half-precision spectral LENGTH BUCKETS at 44.1 kHz: the fused observation of rows of three partition blocks from fp16 block
spectra in buckets (ss_audio_obs_rows_spec16_buckets_f32 / ss_audio_obs_logmel_rows_spec16_buckets_f32: k_obs_blocks<true, MEL,
HALF, HBK> / k_obs_rows<true, false, BUCKETS, MEL, HALF>) against the same launch from fp32 spectral buckets
(ss_audio_obs_spec_buckets_f32 / ss_audio_obs_logmel_spec_buckets_f32), same units, same window spectra, at 5 / 32 / 128 units, for
the pooled spectrogram alone and for spectrogram + log-mel (no waveform buffer).

Three buckets of 1 / 3 / 5 partition blocks (caps 16 384 / 49 152 / 81 920), each a third of the bank's bytes, every entry as
long as its bucket; the units of a launch are dealt out over the three buckets in turn and hear second 1 of a 3-s clip, so every
RIR block of an entry has a window.  The protocol of scripts/kbench_spec_half_rows.py: the two banks hold the same RIRs;
--bank-mib is the size of the HALF bank (the fp32 bank is twice that); launch k of an arm takes, per bucket, the entries behind
those of launch k - 1 (modulo the bucket), in both arms alike, so a row's read comes from HBM at every size.  Stateless entries
through bound ctypes calls, HIP events on the launch stream, the arms ALTERNATING in one process after a warm-up of the shape:
every round times `--launches` launches of each arm back to back; the table gives the median and the minimum over the rounds in
us per launch, and fp16 / fp32.  The outputs of the two arms are compared once per size (max |difference| over the fp32 arm's
peak: the format's error, not a rounding difference).
usage: python scripts/kbench_spec_half_bucket_rows.py [--sizes 5,32,128] [--rounds 9] [--launches 24] [--out FILE]"""
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
from ss_amd import _lib, ops, planning as P
from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="5,32,128")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--launches", type=int, default=24, help="launches per arm and round (rounds x launches >= 200 per point)")
ap.add_argument("--bank-mib", type=int, default=768, help="size of the half bank (the fp32 bank is twice as large)")
ap.add_argument("--sounds", type=int, default=16)
ap.add_argument("--warm", type=int, default=8, help="warm-up launches per arm and size")
ap.add_argument("--out", default="")
a = ap.parse_args()

assert torch.cuda.is_available(), "kbench_spec_half_bucket_rows needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
sr = 44100
CAPS = [16384, 49152, 81920]
rng = np.random.default_rng(0)
r = BatchedAudioRenderer(sr, device=dev)
for i, c in enumerate(O.synth_sources(rng, sr, k=a.sounds, seconds=3)):
    r.add_source(str(i), c)
COUNTS = [max(8, ((a.bank_mib << 20) // 3) // (2 * P.ceil_div(cap, P.KB) * ops.SPEC_FLOATS * 2)) for cap in CAPS]
FIRST = [0, COUNTS[0], COUNTS[0] + COUNTS[1]]
lengths = torch.cat([torch.full((n,), cap, dtype=torch.int32, device=dev) for n, cap in zip(COUNTS, CAPS)])
h32, h16, hsc = [], [], []
for b, (n, cap) in enumerate(zip(COUNTS, CAPS)):
    rows = synth_rir_bank_device(torch, n, sr, cap, dev, 3 + b)
    h32.append(ops.rir_spectra(rows))
    q, s = ops.rir_spectra16(rows)
    h16.append(q); hsc.append(s)
    torch.cuda.synchronize()
    del rows


def bank_of(spectra, scales=None):
    banks = []
    for b, sp in enumerate(spectra):
        bank = RirBank(torch.zeros((COUNTS[b], 2, 0), dtype=torch.float32, device=dev), lengths[FIRST[b]:FIRST[b] + COUNTS[b]], cap=CAPS[b])
        bank.spectra = sp
        bank.scales = scales[b] if scales is not None else None
        banks.append(bank)
    return BucketedRirBank(banks, lengths, FIRST)


bank32, bank16 = bank_of(h32), bank_of(h16, hsc)
r.set_rir_bank(bank32)
ARR32, ARR16 = bank32.spec_c_array(), bank16.spec_c_array()
N_MELS = 64
ms, mw, MAX_LEN = P.mel_filterbank_sparse(sr, N_MELS)
msd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(dev)
mwd = torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(dev)
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream
F = ctypes.c_float


def arms(plan, sg, lm):
    n = len(plan)

    def head(arr):
        return (r._spec.data_ptr(), ctypes.cast(arr, ctypes.c_void_p), 3, lengths.data_ptr(), plan.desc.data_ptr(), None, sg.data_ptr())
    tail = (n, r.n_valid, r.out_len, 0, plan.flags, STREAM)
    if lm is None:
        def half():
            assert LIB.ss_audio_obs_rows_spec16_buckets_f32(*(head(ARR16) + tail)) == 0

        def full():
            assert LIB.ss_audio_obs_spec_buckets_f32(*(head(ARR32) + tail)) == 0
        return half, full
    mel = (lm.data_ptr(), msd.data_ptr(), mwd.data_ptr(), N_MELS, int(MAX_LEN), F(1e-6))

    def half_mel():
        assert LIB.ss_audio_obs_logmel_rows_spec16_buckets_f32(*(head(ARR16) + mel + tail)) == 0

    def full_mel():
        assert LIB.ss_audio_obs_logmel_spec_buckets_f32(*(head(ARR32) + mel + tail)) == 0
    return half_mel, full_mel


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


half_mib = sum(q.numel() * 2 for q in h16) >> 20
lines = [f"# kbench_spec_half_bucket_rows: fused 44.1 kHz observation (no waveform buffer), {torch.cuda.get_device_name(0)}; buckets of "
         f"{COUNTS} entries at caps {CAPS}: half bank {half_mib} MiB + {sum(s.numel() * 4 for s in hsc) >> 10} KiB of scales, fp32 bank "
         f"{sum(h.numel() * 4 for h in h32) >> 20} MiB; {a.sounds} 3-s sounds at t0 = 1 s, {a.rounds} rounds x {a.launches} launches per arm, "
         f"arms alternating, every launch reads bank entries not read since the whole bucket went by (HBM reads at every size); "
         f"us per launch: median (min)",
         f"{'output':>12s} {'units':>5s} {'fp16 buckets':>16s} {'fp32 buckets':>16s} {'fp16/fp32':>9s} {'max diff / peak':>16s}"]
print("\n".join(lines), flush=True)
first = True
walk = [0, 0, 0]                                                         # per bucket: the entry the next plan starts at
for N in [int(x) for x in a.sizes.split(",")]:
    n_plans = a.warm + 1 + a.rounds * a.launches                         # one plan per launch of an arm: no entry is read twice
    plans = []
    for _ in range(n_plans):
        idx = np.empty(N, np.int64)
        for b in range(3):
            m = len(idx[b::3])
            idx[b::3] = FIRST[b] + (walk[b] + np.arange(m)) % COUNTS[b]
            walk[b] = (walk[b] + m) % COUNTS[b]
        plans.append(r.plan_arrays(rng.integers(0, a.sounds, N), np.full(N, sr, np.int64), idx))
    sg = torch.empty((N,) + r.spectrogram_shape, device=dev)
    lm = torch.empty((N, N_MELS, 1 + sr // 160, 2), device=dev)
    for label, lm_out in (("sgram", None), ("sgram+logmel", lm)):
        pairs = [arms(p, sg, lm_out) for p in plans]
        fa = lambda k: pairs[k][0]()
        fb = lambda k: pairs[k][1]()
        if first:
            spin_up(lambda k: pairs[k % a.warm][1]())
            first = False
        for k in range(a.warm):                                          # the shape of the timed window, both arms
            fa(k); fb(k)
        torch.cuda.synchronize()
        out = sg if lm_out is None else lm
        pairs[a.warm][0](); got16 = out.clone()
        pairs[a.warm][1](); got32 = out.clone()
        torch.cuda.synchronize()
        diff = float((got16 - got32).abs().max() / got32.abs().max())
        ta, tb = [], []
        for rd in range(a.rounds):
            k0 = a.warm + 1 + rd * a.launches
            ta.append(timed(lambda k: fa(k0 + k), a.launches))
            tb.append(timed(lambda k: fb(k0 + k), a.launches))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        line = f"{label:>12s} {N:5d} {ma:8.1f} ({min(ta):5.1f}) {mb:8.1f} ({min(tb):5.1f}) {ma / mb:9.3f} {diff:16.2e}"
        lines.append(line)
        print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
