#!/usr/bin/env python
"""Log-mel observation of SoundSpaces 2.0 steps (0.25 s of a 1-s row): the one-launch fused kernel behind
ss_ctx_set_logmel_ss2_policy (ss_audio_obs_logmel_ss2_f32) against the route it replaces ON THE SAME CONTEXT -
ss_ctx_observe_features under the default policy: the step rendered into the context's waveform scratch, then
ss_audio_features_f32 over it - for the same outputs (log-mel alone, and log-mel + pooled spectrogram).  16 kHz cross-faded,
44.1 kHz cross-faded and 44.1 kHz without a previous RIR (the first step of an episode); RIRs of 9000 taps and of 4 s.

Prepared unit columns (ss_ctx_observe_features through bound ctypes calls), HIP events on the launch stream, the arms
ALTERNATING in one process: every round sets the policy and times `--launches` steps of each arm back to back; the table gives
the median and the minimum over the rounds, in us per step.
usage: python scripts/kbench_obs_logmel_ss2.py [--sizes 1,5,10,32,128,256] [--rounds 7] [--launches 40] [--out FILE]"""
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
from ss_amd import planning as P
from ss_amd.context import AudioContext

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1,5,10,32,128,256")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=40, help="steps per arm and round (rounds x launches >= 200 per point)")
ap.add_argument("--entries", type=int, default=256, help="RIR bank entries")
ap.add_argument("--sounds", type=int, default=16)
ap.add_argument("--distinct", type=int, default=8, help="pre-planned steps cycled")
ap.add_argument("--n-mels", type=int, default=64)
ap.add_argument("--out", default="")
a = ap.parse_args()

dev = torch.device("cuda:0")
STREAM = torch.cuda.current_stream().cuda_stream
EPS = 1e-6
ALWAYS, NEVER = (1, 2 ** 31 - 1), (1, 0)


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


lines = [f"# kbench_obs_logmel_ss2: n_valid = sr / 4, {a.n_mels} bands, bank of {a.entries} entries, {a.sounds} sounds (1 s, tiled "
         f"x3), {a.rounds} rounds x {a.launches} steps per arm, arms alternating on one context; us per step: median (min)",
         f"{'sr':>6s} {'step':>9s} {'rir taps':>8s} {'units':>5s} {'outputs':>10s} {'fused':>16s} {'scratch route':>16s} {'fused/scr':>9s}"]
print("\n".join(lines), flush=True)
first = True
for sr, crossfade in ((16000, True), (44100, True), (44100, False)):
    rng = np.random.default_rng(sr + crossfade)
    ms, mw, _ = P.mel_filterbank_sparse(sr, a.n_mels)
    msd = torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(dev)
    mwd = torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(dev)
    T, sg_shape = 1 + sr // 160, P.spectrogram_shape(sr)
    clips = [O.tile_short_source(c, sr) for c in O.synth_sources(rng, sr, k=a.sounds)]
    starts = rng.integers(0, 3 * sr, 32)                   # sample indices the steps draw from (early, steady and wrapped branches)
    for taps in (9000, 4 * sr):
        ctx = AudioContext(sr, step_time=0.25, wrap=True, max_window_sets=1024)       # every (sound, index) of the run stays cached
        for i, c in enumerate(clips):
            ctx.add_source(str(i), c)
        bank = synth_rir_bank_device(torch, a.entries, sr, taps, dev, 3)
        lengths = torch.full((a.entries,), taps, dtype=torch.int32, device=dev)
        ctx.set_rir_bank(bank, lengths)
        for N in [int(x) for x in a.sizes.split(",")]:
            preps = []
            for _ in range(a.distinct):
                idx = starts[rng.integers(0, len(starts), N)]
                cols = dict(sound=rng.integers(0, a.sounds, N), t0=idx, rir=rng.integers(0, a.entries, N),
                            wrap=(idx >= taps).astype(np.uint8))
                if crossfade:                              # every unit carries its previous step's RIR (same length: same branch)
                    cols.update(last_rir=rng.integers(0, a.entries, N), last_wrap=cols["wrap"])
                preps.append(ctx.prepare(**cols))
            sg = torch.empty((N,) + sg_shape, device=dev)
            lm = torch.empty((N, a.n_mels, T, 2), device=dev)
            feat = ctx.features(lm, msd, mwd, EPS)
            for want_sg in (False, True):
                sgp = sg.data_ptr() if want_sg else None
                step = lambda k: ctx.observe_prepared_features(preps[k % a.distinct], sgp, None, STREAM, feat)
                if first:
                    spin_up(step)
                    first = False
                for pol in (ALWAYS, NEVER):                # both arms warm: window spectra cached, the scratch allocated
                    ctx.set_logmel_ss2_policy(*pol)
                    for k in range(a.distinct):
                        step(k)
                torch.cuda.synchronize()
                ta, tb = [], []
                for _ in range(a.rounds):
                    ctx.set_logmel_ss2_policy(*ALWAYS)
                    ta.append(timed(step, a.launches))
                    ctx.set_logmel_ss2_policy(*NEVER)
                    tb.append(timed(step, a.launches))
                ma, mb = float(np.median(ta)), float(np.median(tb))
                line = (f"{sr:6d} {'crossfade' if crossfade else 'plain':>9s} {taps:8d} {N:5d} {'mel+sgram' if want_sg else 'mel':>10s} "
                        f"{ma:8.1f} ({min(ta):5.1f}) {mb:8.1f} ({min(tb):5.1f}) {ma / mb:9.3f}")
                lines.append(line)
                print(line, flush=True)
        torch.cuda.synchronize()
        ctx.close()
        del bank
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
