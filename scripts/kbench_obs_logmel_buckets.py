#!/usr/bin/env python
"""Log-mel observation from a LENGTH-BUCKETED bank: the one-launch fused kernels behind ss_ctx_set_logmel_buckets_policy
(ss_audio_obs_logmel_buckets_f32 / ss_audio_obs_logmel_spec_buckets_f32) against the route they replace ON THE SAME CONTEXT -
ss_ctx_observe_features under the default policy: the step rendered into the context's waveform scratch, then
ss_audio_features_f32 over it - for the same outputs (log-mel alone, and log-mel + pooled spectrogram).  The policy set to
"never" is the route of the library before the fused entries existed, and is the baseline.

The mixed-bucket step of scripts/kbench_spec_buckets.py: four buckets of 1 / 2 / 3 / 5 partition blocks with --entries entries,
every entry as long as its cap, 6-s clips heard at t0 = 5 s, so every block of a row is multiplied; a step of N units takes N/2,
N/4, N/8, N/8 units from the four buckets (at least one each while N allows) and walks through the entries of every bucket.
16 kHz: the three bank forms (rows + spectra, fp32 spectra alone, fp16 spectra + scales) at 1 / 5 / 16 / 128 units; 44.1 kHz: the
two fp32 forms the row kernels read (rows alone, fp32 spectra alone) at 5 / 42 / 43 / 128 units - 42 | 43 is where the grid of one
workgroup per output block stops fitting the chip.

Prepared unit columns (ss_ctx_observe_features through bound ctypes calls), HIP events on the launch stream, the arms ALTERNATING
in one process: every round sets the policy and times `--launches` steps of each arm back to back; the table gives the median and
the minimum over the rounds in us per step, the baseline arm's own spread over its rounds (max - min), and whether the fused
arm's median lies below the baseline's by more than that spread.
usage: python scripts/kbench_obs_logmel_buckets.py [--rounds 7] [--launches 40] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]
import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import ops, planning as P
from ss_amd.context import AudioContext
from ss_amd.renderer import BucketedRirBank, RirBank

ap = argparse.ArgumentParser()
ap.add_argument("--sizes16", default="1,5,16,128")
ap.add_argument("--sizes44", default="5,42,43,128")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=40, help="steps per arm and round")
ap.add_argument("--entries", default="512,128,64,32", help="entries per bucket")
ap.add_argument("--sounds", type=int, default=16)
ap.add_argument("--distinct", type=int, default=8, help="pre-planned steps cycled")
ap.add_argument("--n-mels", type=int, default=64)
ap.add_argument("--out", default="")
a = ap.parse_args()

assert torch.cuda.is_available(), "kbench_obs_logmel_buckets needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
STREAM = torch.cuda.current_stream().cuda_stream
EPS = 1e-6
ALWAYS, NEVER = (1, 2 ** 31 - 1), (1, 0)
CAPS = [P.KB, 2 * P.KB, 3 * P.KB, 5 * P.KB]
COUNTS = [int(x) for x in a.entries.split(",")]
FIRST = [int(v) for v in np.cumsum([0] + COUNTS[:-1])]
SHARE = [2, 4, 8, 8]                                                     # a step takes N / SHARE[b] units from bucket b


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


def banks_of(sr, form):
    """the bucketed bank in one form: 'both' (rows + fp32 spectra) | 'rows' | 'only' | 'half'"""
    lengths = torch.cat([torch.full((n,), cap, dtype=torch.int32, device=dev) for n, cap in zip(COUNTS, CAPS)])
    out = []
    for b, (n, cap) in enumerate(zip(COUNTS, CAPS)):
        view = lengths[FIRST[b]:FIRST[b] + n]
        rows = synth_rir_bank_device(torch, n, sr, cap, dev, 3 + b)
        if form in ("both", "rows"):
            bank = RirBank(rows, view)
            if form == "both":
                bank.spectra = ops.rir_spectra(rows)
        else:
            bank = RirBank(torch.zeros((n, 2, 0), dtype=torch.float32, device=dev), view, cap=cap)
            if form == "half":
                bank.spectra, bank.scales = ops.rir_spectra16(rows)
            else:
                bank.spectra = ops.rir_spectra(rows)
        out.append(bank)
    torch.cuda.synchronize()
    return BucketedRirBank(out, lengths, FIRST)


lines = [f"# kbench_obs_logmel_buckets: {torch.cuda.get_device_name(0)}; 4 length buckets of 1/2/3/5 blocks, entries {COUNTS}, "
         f"{a.sounds} 6-s sounds at t0 = 5 s, {a.n_mels} bands, {a.rounds} rounds x {a.launches} steps per arm, arms alternating on one "
         f"context (policy always | never); us per step: median (min); spread = max - min of the baseline arm's rounds",
         f"{'sr':>6s} {'bank':>5s} {'units':>5s} {'outputs':>10s} {'fused':>16s} {'scratch route':>16s} {'spread':>7s} {'fused/scr':>9s} "
         f"{'below by > spread':>17s}"]
print("\n".join(lines), flush=True)
first = True
walk = [0, 0, 0, 0]
for sr, forms, sizes in ((16000, ("both", "only", "half"), a.sizes16), (44100, ("rows", "only"), a.sizes44)):
    rng = np.random.default_rng(sr)
    ms, mw, _ = P.mel_filterbank_sparse(sr, a.n_mels)
    msd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(dev)
    mwd = torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(dev)
    T, sg_shape = 1 + sr // 160, P.spectrogram_shape(sr)
    clips = O.synth_sources(rng, sr, k=a.sounds, seconds=6)
    for form in forms:
        bank = banks_of(sr, form)
        ctx = AudioContext(sr, max_window_sets=1024)
        for i, c in enumerate(clips):
            ctx.add_source(str(i), c)
        if form in ("only", "half"):
            ctx.set_rir_spec_buckets(bank)
        else:
            ctx.set_rir_buckets(bank, spectral=form == "both")
        for N in [int(x) for x in sizes.split(",")]:
            preps = []
            for _ in range(a.distinct):
                rir = []
                for b in range(4):
                    k = max(1, N // SHARE[b])
                    rir.append(FIRST[b] + (walk[b] + np.arange(k)) % COUNTS[b])
                    walk[b] = (walk[b] + k) % COUNTS[b]
                short = N - sum(len(x) for x in rir)            # (N / 2 + N / 4 + 2 (N / 8) rounds down: the rest from bucket 0)
                if short > 0:
                    rir.append(FIRST[0] + (walk[0] + np.arange(short)) % COUNTS[0])
                    walk[0] = (walk[0] + short) % COUNTS[0]
                rir = rng.permutation(np.concatenate(rir))[:N]
                if N >= 4:                                       # (small steps: the longest buckets must not be cut off)
                    rir[:4] = [FIRST[b] + walk[b] % COUNTS[b] for b in range(4)]
                preps.append(ctx.prepare(sound=rng.integers(0, a.sounds, N), t0=np.full(N, 5 * sr, np.int64), rir=rir))
            sg = torch.empty((N,) + sg_shape, device=dev)
            lm = torch.empty((N, a.n_mels, T, 2), device=dev)
            feat = ctx.features(lm, msd, mwd, EPS)
            for want_sg in (False, True):
                sgp = sg.data_ptr() if want_sg else None
                step = lambda k: ctx.observe_prepared_features(preps[k % a.distinct], sgp, None, STREAM, feat)
                if first:
                    spin_up(step)
                    first = False
                for pol in (ALWAYS, NEVER):                      # both arms warm: window spectra cached, the scratch allocated
                    ctx.set_logmel_buckets_policy(*pol)
                    for k in range(a.distinct):
                        step(k)
                torch.cuda.synchronize()
                ta, tb = [], []
                for _ in range(a.rounds):
                    ctx.set_logmel_buckets_policy(*ALWAYS)
                    ta.append(timed(step, a.launches))
                    ctx.set_logmel_buckets_policy(*NEVER)
                    tb.append(timed(step, a.launches))
                ma, mb, spread = float(np.median(ta)), float(np.median(tb)), max(tb) - min(tb)
                line = (f"{sr:6d} {form:>5s} {N:5d} {'mel+sgram' if want_sg else 'mel':>10s} {ma:8.1f} ({min(ta):5.1f}) "
                        f"{mb:8.1f} ({min(tb):5.1f}) {spread:7.1f} {ma / mb:9.3f} {str(mb - ma > spread):>17s}")
                lines.append(line)
                print(line, flush=True)
        torch.cuda.synchronize()
        ctx.close()
        del bank
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
