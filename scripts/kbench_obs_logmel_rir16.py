#!/usr/bin/env python
"""One-launch log-mel from half-precision time-domain RIR rows: kernel time per step of three arms on identical units, in one
process:

  (a) today's route    what a context bound to half rows does under the default policy: the half convolution into a waveform -
                       ss_fftconv_binaural_rir16[_buckets]_f32 for log-mel alone; with the spectrogram asked as well
                       ss_audio_obs_rir16[_buckets]_f32 at 16 kHz, ss_audio_obs_rows_rir16_f32 at 44.1 kHz - then
                       ss_audio_features_f32 (k_features) over it.  The yardstick.
  (b) one launch       ss_audio_obs_logmel_rir16_f32 / _rir16_buckets_f32 / _rows_rir16_f32, no waveform anywhere
  (c) fp32 rows        ss_audio_obs_logmel_f32 / _buckets_f32 / _rows_f32 on the fp32 rows the halves were quantised from, for
                       orientation

at 16 kHz on one allocation and on three length buckets (a mixed step: about 10 % of the units, at least one, outside bucket 0), and
at 44.1 kHz on one allocation; log-mel alone and log-mel + pooled spectrogram.  Launch k of an arm takes the entries behind those of
launch k - 1, modulo the bank (per bucket), in every arm alike, so every row is read from HBM; the window spectra of the sounds
are cache hits in every arm, as in the product.  Stateless entries through bound ctypes calls, HIP events on the launch stream,
the arms ALTERNATING after a warm-up of the shape; the table gives the median and the minimum over the rounds in us per step and
the ratios (b)/(a), (b)/(c).

usage: python scripts/kbench_obs_logmel_rir16.py [--out FILE] [--rounds 5] [--launches 20]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="steps per arm and round")
ap.add_argument("--warm", type=int, default=6, help="warm-up steps per arm and point")
ap.add_argument("--sounds", type=int, default=102)
ap.add_argument("--entries16", type=int, default=4096, help="entries of the 16 kHz bank (one allocation)")
ap.add_argument("--entries44", type=int, default=1536, help="entries of the 44.1 kHz bank")
ap.add_argument("--slots", default="4096,512,256", help="entries per bucket")
ap.add_argument("--caps", default="16000,49152,65536", help="samples per row of each bucket")
ap.add_argument("--units16", default="1,16,32,128,256,512")
ap.add_argument("--units44", default="5,10,42,43,128")
ap.add_argument("--out", default="")
a = ap.parse_args()

import ctypes

import numpy as np
import torch
from bench import synth_rir_bank_device
from oracle import ss_oracle as O
from ss_amd import _lib, ops, planning as P
from ss_amd.renderer import BatchedAudioRenderer, BucketedRirBank, RirBank

assert torch.cuda.is_available(), "kbench_obs_logmel_rir16 needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream
NAMES = ("(a) conv + features", "(b) one launch", "(c) fp32 one launch")
EPS = 1e-6
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(launches):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


def renderer(sr):
    r = BatchedAudioRenderer(sr, device=dev)
    for i, c in enumerate(O.synth_sources(rng, sr, k=a.sounds)):
        r.add_source(str(i), c)
    ms, mw, max_len = P.mel_filterbank_sparse(sr, 64)
    mel = (torch.from_numpy(np.ascontiguousarray(ms, np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(mw, np.float32)).to(dev), int(max_len))
    return r, mel


def features(ag, lm, n, sr, mel):
    assert LIB.ss_audio_features_f32(ag, n, sr, 0, None, lm, mel[0].data_ptr(), mel[1].data_ptr(), 64, mel[2], EPS, None, 1, 1.0, STREAM) == 0


def single(sr, entries):
    """one allocation: -> arms(plan, bufs, want_sg) and a walker over the entries"""
    r, mel = renderer(sr)
    rows = synth_rir_bank_device(torch, entries, sr, sr, dev, 7)
    lengths = torch.full((entries,), sr, dtype=torch.int32, device=dev)
    q, s = ops.rir_rows16(rows)
    r.set_rir_bank(RirBank(rows, lengths))
    long_rows = sr > P.KB
    obs16 = LIB.ss_audio_obs_rows_rir16_f32 if long_rows else LIB.ss_audio_obs_rir16_f32
    mel16 = LIB.ss_audio_obs_logmel_rows_rir16_f32 if long_rows else LIB.ss_audio_obs_logmel_rir16_f32
    mel32 = LIB.ss_audio_obs_logmel_rows_f32 if long_rows else LIB.ss_audio_obs_logmel_f32
    state = dict(at=0)

    def indices(n):
        idx = (state["at"] + np.arange(n)) % entries
        state["at"] = (state["at"] + n) % entries
        return idx

    def arms(plan, ag, sg, lm, want_sg):
        n = len(plan)
        sp, ln, ds = r._spec.data_ptr(), lengths.data_ptr(), plan.desc.data_ptr()
        nv, ol, fl = r.n_valid, r.out_len, plan.flags
        sgp = sg.data_ptr() if want_sg else None
        ms, mw, ml = mel[0].data_ptr(), mel[1].data_ptr(), mel[2]

        def today():
            if want_sg:
                assert obs16(sp, q.data_ptr(), s.data_ptr(), ln, ds, ag.data_ptr(), sgp, n, sr, nv, ol, 0, fl, STREAM) == 0
            else:
                assert LIB.ss_fftconv_binaural_rir16_f32(sp, q.data_ptr(), s.data_ptr(), ln, ds, ag.data_ptr(), n, sr, nv, ol, fl, STREAM) == 0
            features(ag.data_ptr(), lm.data_ptr(), n, sr, mel)

        def one():
            assert mel16(sp, q.data_ptr(), s.data_ptr(), ln, ds, None, sgp, lm.data_ptr(), ms, mw, 64, ml, EPS, n, sr, nv, ol, 0, fl, STREAM) == 0

        def fp32():
            assert mel32(sp, rows.data_ptr(), ln, ds, None, sgp, lm.data_ptr(), ms, mw, 64, ml, EPS, n, 2 * sr, sr, 1, sr, nv, ol, 0, fl,
                         STREAM) == 0
        return today, one, fp32
    keep = (rows, lengths, q, s)
    return r, arms, indices, keep, f"one allocation of {entries} entries x {sr} samples"


def bucketed(sr):
    r, mel = renderer(sr)
    slots = [int(x) for x in a.slots.split(",")]
    caps = [int(x) for x in a.caps.split(",")]
    first = [0, slots[0], slots[0] + slots[1]]
    lengths = torch.cat([torch.full((n,), c, dtype=torch.int32, device=dev) for n, c in zip(slots, caps)])
    views = [lengths[f:f + n] for f, n in zip(first, slots)]
    rows = [synth_rir_bank_device(torch, n, sr, c, dev, 3 + b) for b, (n, c) in enumerate(zip(slots, caps))]
    halves = [ops.rir_rows16(x) for x in rows]
    bank32 = BucketedRirBank([RirBank(x, v) for x, v in zip(rows, views)], lengths, first)
    bank16 = BucketedRirBank([RirBank(q, v, scales=s) for (q, s), v in zip(halves, views)], lengths, first)
    r.set_rir_bank(bank16)
    arr32, arr16 = bank32.c_array(False), bank16.rir16_c_array()
    walk = [0, 0, 0]

    def indices(n):
        n_out = max(1, int(round(n / 10))) if n > 1 else 0
        idx = np.empty(n, np.int64)
        for u in range(n):
            b = 0 if u >= n_out else 1 + (u & 1)
            idx[u] = first[b] + walk[b]
            walk[b] = (walk[b] + 1) % slots[b]
        return rng.permutation(idx)

    def arms(plan, ag, sg, lm, want_sg):
        n = len(plan)
        sp, ln, ds = r._spec.data_ptr(), lengths.data_ptr(), plan.desc.data_ptr()
        nv, ol, fl = r.n_valid, r.out_len, plan.flags
        sgp = sg.data_ptr() if want_sg else None
        ms, mw, ml = mel[0].data_ptr(), mel[1].data_ptr(), mel[2]
        p32, p16 = ctypes.cast(arr32, ctypes.c_void_p), ctypes.cast(arr16, ctypes.c_void_p)

        def today():
            if want_sg:
                assert LIB.ss_audio_obs_rir16_buckets_f32(sp, p16, 3, ln, ds, ag.data_ptr(), sgp, n, nv, ol, 0, fl, STREAM) == 0
            else:
                assert LIB.ss_fftconv_binaural_rir16_buckets_f32(sp, p16, 3, ln, ds, ag.data_ptr(), n, nv, ol, fl, STREAM) == 0
            features(ag.data_ptr(), lm.data_ptr(), n, sr, mel)

        def one():
            assert LIB.ss_audio_obs_logmel_rir16_buckets_f32(sp, p16, 3, ln, ds, None, sgp, lm.data_ptr(), ms, mw, 64, ml, EPS, n, nv, ol, 0,
                                                             fl, STREAM) == 0

        def fp32():
            assert LIB.ss_audio_obs_logmel_buckets_f32(sp, p32, 3, ln, ds, None, sgp, lm.data_ptr(), ms, mw, 64, ml, EPS, n, nv, ol, 0, fl,
                                                       STREAM) == 0
        return today, one, fp32
    keep = (rows, halves, lengths, bank32, bank16, arr32, arr16)
    return r, arms, indices, keep, f"buckets of {slots} entries x {caps} samples, mixed steps (about 10 % of the units outside bucket 0)"


emit(f"# kbench_obs_logmel_rir16, {torch.cuda.get_device_name(0)}; {a.sounds} sounds, {a.rounds} rounds x {a.launches} steps per arm, arms "
     f"alternating, every step reads entries not read since the whole bank went by; ONE pass; us per step: median (min)")
spun = False
for label, sr, build, units in (("16 kHz", 16000, lambda: single(16000, a.entries16), a.units16), ("16 kHz buckets", 16000, lambda: bucketed(16000), a.units16),
                                ("44.1 kHz", 44100, lambda: single(44100, a.entries44), a.units44)):
    r, arms, indices, keep, what = build()
    torch.cuda.synchronize()
    emit(f"## {label}: {what}")
    emit(f"{'outputs':>14s} {'units':>5s} " + " ".join(f"{nm:>20s}" for nm in NAMES) + f" {'b/a':>6s} {'b/c':>6s} {'b vs a log-mel':>14s}")
    for want_sg in (False, True):
        for N in [int(x) for x in units.split(",")]:
            n_plans = a.warm + 1 + a.rounds * a.launches
            plans = [r.plan_arrays(rng.integers(0, a.sounds, N), np.zeros(N, np.int64), indices(N)) for _ in range(n_plans)]
            ag = torch.empty((N, 2, sr), device=dev)
            sg = torch.empty((N,) + r.spectrogram_shape, device=dev)
            lm = torch.empty((N, 64, 1 + sr // 160, 2), device=dev)
            trio = [arms(p, ag, sg, lm, want_sg) for p in plans]
            if not spun:                                                 # clocks up before the first timed window
                t0, k = time.perf_counter(), 0
                while time.perf_counter() - t0 < 0.06:
                    trio[k % a.warm][1](); k += 1
                torch.cuda.synchronize()
                spun = True
            for k in range(a.warm):                                      # the shape of the timed window, every arm
                for arm in range(3):
                    trio[k][arm]()
            torch.cuda.synchronize()
            trio[a.warm][0](); ref = lm.clone()
            trio[a.warm][1](); got = lm.clone()
            torch.cuda.synchronize()
            diff = float(((got - ref).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))).max())
            t = [[], [], []]
            for rd in range(a.rounds):
                k0 = a.warm + 1 + rd * a.launches
                for arm in range(3):
                    t[arm].append(timed(lambda k: trio[k0 + k][arm](), a.launches))
            m = [float(np.median(x)) for x in t]
            emit(f"{'log-mel + sgram' if want_sg else 'log-mel':>14s} {N:5d} " + " ".join(f"{m[i]:12.1f} ({min(t[i]):5.1f})" for i in range(3)) +
                 f" {m[1] / m[0]:6.3f} {m[1] / m[2]:6.3f} {diff:14.2e}")
            del trio, plans, ag, sg, lm
    del r, arms, indices, keep
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
