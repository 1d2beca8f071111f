#!/usr/bin/env python
"""Spectral-only RIR bank (AudioEngine(rir_spectral="only")) against the both-forms bank (rir_spectral=True), same box, same
process, alternating: HBM per entry (torch.cuda.memory_allocated of the store) and entries per GiB; the 128-env 16 kHz dependent
step and a 5-env 44.1 kHz step (context path, resident poses: the same kernels for both forms); and the miss path of 128 envs
with 1 / 5 / 25 % new poses per step (RirStore.load_files from float32 wav files: read + the store's staged scatter - one
k_stage_spectra launch against k_scatter_rows + k_source_windows - + the step).  Prints one JSON line per measurement.
Usage: python scripts/bench_spectral_only.py [--reps 200] [--tmp DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]
from oracle import ss_oracle as O  # noqa: E402
from ss_amd import planning as P  # noqa: E402
from ss_amd.renderer import AudioEngine, RirStore  # noqa: E402

DEV = "cuda:0"
MODES = (("both", True), ("only", "only"))


def hbm(sr):
    out = {}
    for name, mode in MODES:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(DEV)
        st = RirStore(1024, sr, DEV, spectral=mode)
        torch.cuda.synchronize()
        per = (torch.cuda.memory_allocated(DEV) - before) / 1024
        out[name] = dict(bytes_per_entry=per, entries_per_gib=(1 << 30) / per)
        del st
        torch.cuda.empty_cache()
    out["ratio_only_vs_both"] = out["only"]["entries_per_gib"] / out["both"]["entries_per_gib"]
    print(json.dumps(dict(what="hbm_per_entry", sr=sr, **out)), flush=True)


def engine(sr, mode, n_rirs, slots):
    rng = np.random.default_rng(1)
    eng = AudioEngine(sr, device=DEV, rir_slots=slots, rir_spectral=mode)
    src = O.synth_sources(rng, sr, k=8)
    for i, s in enumerate(src):
        eng.source_id(f"s{i}", s)
    rirs = [np.ascontiguousarray(O.synth_rir(rng, sr, length=sr, n=1)[0].T) for _ in range(n_rirs)]
    sl = [eng.rir_slot(i, (lambda h=h: h)) for i, h in enumerate(rirs)]
    return eng, sl


def step_time(sr, n_env, reps):
    res = {}
    engs = {name: engine(sr, mode, 64, 256) for name, mode in MODES}
    rng = np.random.default_rng(2)
    for name, (eng, sl) in engs.items():
        ctx = eng._sync_context_bank(n_env, False)
        cols = dict(sound=rng.integers(0, 8, n_env).astype(np.int32), t0=np.zeros(n_env, np.int32),
                    rir=np.asarray(sl, np.int32)[rng.integers(0, len(sl), n_env)])
        prep = ctx.prepare(**cols)
        sg = torch.empty((n_env,) + ctx.spectrogram_shape, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        res[name] = (ctx, prep, sg, stream)
    times = {name: [] for name in res}
    for r in range(reps):                                       # alternating, one dependent step at a time
        for name, (ctx, prep, sg, stream) in res.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            ctx.observe_prepared(prep, sg.data_ptr(), None, stream)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t)
    out = {k: dict(median_us=float(np.median(v[reps // 10:]) * 1e6), p10_us=float(np.percentile(v[reps // 10:], 10) * 1e6))
           for k, v in times.items()}
    print(json.dumps(dict(what="dependent_step", sr=sr, n_env=n_env, reps=reps, **out)), flush=True)


def miss_path(tmp, reps):
    from scipy.io import wavfile
    sr, n_env = 16000, 128
    rng = np.random.default_rng(3)
    paths = []
    for i in range(4096):
        p = os.path.join(tmp, f"r{i}.wav")
        if not os.path.exists(p):
            wavfile.write(p, sr, np.ascontiguousarray(O.synth_rir(np.random.default_rng(i), sr, length=16000, n=1)[0].T))
        paths.append(p)
    for frac in (0.01, 0.05, 0.25):
        k = max(1, int(round(frac * n_env)))
        times = {}
        for name, mode in MODES + (("only_device_staging", "only"),):
            eng, _ = engine(sr, mode, 1, 1024)
            st = eng.store
            st.scatter_from_host = name != "only_device_staging"     # (A/B: the store's policy, or every block copied first)
            ctx = eng._sync_context_bank(n_env, False)
            resident = st.load_files(paths[:n_env], paths[:n_env])
            nxt = n_env
            sg = torch.empty((n_env,) + ctx.spectrogram_shape, device=DEV)
            stream = torch.cuda.current_stream().cuda_stream
            ts = []
            for r in range(reps):
                new = [paths[(nxt + j) % len(paths)] for j in range(k)]
                nxt += k
                torch.cuda.synchronize()
                t = time.perf_counter()
                slots = st.load_files(new, new)
                resident = resident[k:] + slots
                ctx = eng._sync_context_bank(n_env, False)
                ctx.observe(np.zeros(n_env, np.int32), np.zeros(n_env, np.int32), np.asarray(resident, np.int32), spectrogram_out=sg,
                            stream=stream)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            times[name] = dict(median_us=float(np.median(ts[reps // 10:]) * 1e6))
            del eng
        print(json.dumps(dict(what="miss_path_load_files_plus_step", sr=sr, n_env=n_env, new_poses=k, reps=reps, **times)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    for sr in (16000, 44100):
        hbm(sr)
    step_time(16000, 128, a.reps)
    step_time(44100, 5, a.reps)
    tmp = a.tmp or tempfile.mkdtemp(prefix="ss_specbench_")
    miss_path(tmp, max(20, a.reps // 4))


if __name__ == "__main__":
    main()
