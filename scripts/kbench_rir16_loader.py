#!/usr/bin/env python
"""Pose misses on half-precision time-domain RIR rows: the last hop alone, and whole deferred-mode steps, in one process.

  1. KERNELS.  k_scatter_rows16 (ss_bank_scatter_rows16_f32: one workgroup per row, the row read twice; the reference) against
     k_scatter_rows16_max (ss_bank_scatter_rows16_max_f32: ceil(cap / 512) workgroups per row, the row read once, its maxima
     given) for 1 / 8 / 64 full rows at 16 kHz and 44.1 kHz, the rows, slots, lengths and maxima in PINNED HOST memory - what the
     in-call loader hands the kernel.  HIP events on the launch stream around `--launches` launches, the two arms ALTERNATING after
     a warm-up of the shape; median and minimum over the rounds in us per launch, and the ratio new / old.  The two banks are
     compared once per point (0 differing bytes expected).  The maxima are not part of the kernel time: the reader takes them on
     its own thread while it reads (section 2 includes that).

  2. STEPS.  128 envs at 16 kHz, deferred mode (the trainer half of scripts/bench_loader.py's miss steps: float32 stereo wav files on
     tmpfs, 4 x 128 poses resident before the clock starts, then round(rate x 128) envs on a never-seen pose per step) at 1 / 5 /
     25 %, three arms ALTERNATING in blocks of `--steps` steps:
       (a) half rows, three calls   AudioEngine(rir_rows="half"), native_miss_path=False: report -> load_files -> call again
                                    (what every step with a miss did on this form before; the reference)
       (b) half rows, in call       the same engine, the misses served inside ss_ctx_observe_requests_load
       (c) fp32 rows, in call       AudioEngine() as it is
     Per arm: the median host time of the resolver's call per step (the figure README quotes for the fp32 form) and the wall time
     per step of each block, ended by a device synchronise (median over the blocks).

usage: python scripts/kbench_rir16_loader.py [--out FILE] [--rounds 7] [--launches 20] [--steps 20] [--blocks 5]"""
import argparse
import os
import shutil
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd"), os.path.join(ROOT, "scripts")]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=20, help="launches per arm and round")
ap.add_argument("--rows", default="1,8,64")
ap.add_argument("--caps", default="16000,44100")
ap.add_argument("--envs", type=int, default=128)
ap.add_argument("--rates", default="0.01,0.05,0.25")
ap.add_argument("--steps", type=int, default=20, help="steps per arm and block")
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--files", type=int, default=512, help="distinct wav files (hard-linked to the scene's names)")
ap.add_argument("--skip-steps", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()

import numpy as np
import torch
from oracle import ss_oracle as O
from ss_amd import _lib, planning as P

assert torch.cuda.is_available(), "kbench_rir16_loader needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
LIB = _lib.load()
STREAM = torch.cuda.current_stream().cuda_stream
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------------
emit(f"# kbench_rir16_loader, {torch.cuda.get_device_name(0)}; 1. the scatter kernels from pinned host staging, full rows; "
     f"{a.rounds} rounds x {a.launches} launches per arm, arms alternating; us per launch: median (min)")
emit(f"{'cap':>6s} {'rows':>5s} {'k_scatter_rows16':>18s} {'k_scatter_rows16_max':>21s} {'new/old':>8s} {'differing bytes':>15s}")
rng = np.random.default_rng(0)
spun = False
for cap in [int(x) for x in a.caps.split(",")]:
    for n in [int(x) for x in a.rows.split(",")]:
        entries = 4 * n
        stage = torch.from_numpy((rng.standard_normal((n, cap, 2)) * 0.05).astype(np.float32)).pin_memory()
        slots = torch.from_numpy(rng.permutation(entries)[:n].astype(np.int32)).pin_memory()
        lens = torch.full((n,), cap, dtype=torch.int32).pin_memory()
        mx = stage.abs().amax(1).contiguous().pin_memory()
        banks = [(torch.zeros((entries, 2, cap), dtype=torch.float16, device=dev), torch.zeros((entries, 2), device=dev),
                  torch.zeros((entries,), dtype=torch.int32, device=dev)) for _ in range(2)]

        def old(b=banks[0]):
            assert LIB.ss_bank_scatter_rows16_f32(stage.data_ptr(), 2 * cap, slots.data_ptr(), lens.data_ptr(), n, b[0].data_ptr(),
                                                  b[1].data_ptr(), cap, b[2].data_ptr(), STREAM) == 0

        def new(b=banks[1]):
            assert LIB.ss_bank_scatter_rows16_max_f32(stage.data_ptr(), 2 * cap, slots.data_ptr(), lens.data_ptr(), mx.data_ptr(), n,
                                                      b[0].data_ptr(), b[1].data_ptr(), cap, b[2].data_ptr(), STREAM) == 0
        if not spun:                                                     # clocks up before the first timed window
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.06:
                new()
            torch.cuda.synchronize()
            spun = True
        for _ in range(5):
            old(); new()
        torch.cuda.synchronize()
        differing = sum(int((x.view(torch.uint8) != y.view(torch.uint8)).sum()) for x, y in zip(*banks))
        t = [[], []]
        for rd in range(a.rounds):
            for arm, fn in enumerate((old, new)):
                t[arm].append(timed(fn, a.launches))
        m = [float(np.median(x)) for x in t]
        emit(f"{cap:6d} {n:5d} {m[0]:10.1f} ({min(t[0]):5.1f}) {m[1]:13.1f} ({min(t[1]):5.1f}) {m[1] / m[0]:8.3f} {differing:15d}")
        del stage, slots, lens, mx, banks


# ---- 2. steps ---------------------------------------------------------------------------------------------------------------------
def make_arm(name, root, sr, n_nodes, n_envs, m, n_steps, sources, in_call, engine_kw):
    from bench import SyntheticSim
    from ss_amd.deferred import DeferredResolver, attach_deferred
    from ss_amd.renderer import AudioEngine
    from ss_amd.rollout import RolloutStorage
    from ss_amd.sim_audio import wav_rir_reader
    NS = types.SimpleNamespace
    arng = np.random.default_rng(3)                                      # the same walk in every arm
    sounds = {"sound%d" % i: c for i, c in enumerate(sources)}

    class DSim(SyntheticSim):
        config = NS(AUDIO=NS(RIR_SAMPLING_RATE=sr, HAS_DISTRACTOR_SOUND=False), USE_RENDERED_OBSERVATIONS=True)
        binaural_rir_dir = root
        azimuth_angle = property(lambda self: -(self._rotation_angle + 0) % 360)
        current_source_sound = property(lambda self: self._source_sound_dict[self._current_sound])
        _audio_length = property(lambda self: self.current_source_sound.shape[0] // sr)

    poses = [(r, s, az) for r in range(n_nodes) for s in range(n_nodes) for az in range(4)]
    arng.shuffle(poses)
    n_res = 4 * n_envs
    assert len(poses) >= n_res + n_steps * m, "scene too small for this miss rate"
    eng = AudioEngine(sr, device=dev, rir_slots=n_res + (n_steps + 1) * m + 64, **engine_kw)
    sims = [DSim(sounds, n_nodes, arng) for _ in range(n_envs)]
    for s_ in sims:
        s_._duration = 10 ** 9
    space = NS(spaces={"spectrogram": NS(shape=P.spectrogram_shape(sr))})

    class ActionSpace:
        pass
    rollouts = RolloutStorage(16, n_envs, space, ActionSpace(), 8, device=dev)
    res = DeferredResolver(eng, rir_reader=wav_rir_reader, fast=True)
    res.native_miss_path = bool(in_call)
    for i, sim in enumerate(sims):
        attach_deferred(sim, env_rank=i)

    def place(sim, pose):
        sim._receiver_position_index, sim._source_position_index, sim._rotation_angle = pose[0], pose[1], 90 * pose[2]
        sim._episode_step_count += 1

    def step():
        obs = [{"spectrogram": sim.get_current_spectrogram_observation(None)} for sim in sims]
        t0 = time.perf_counter()
        res.resolve_observations(obs, rollouts, replace=False)
        dt = time.perf_counter() - t0
        rollouts.step = (rollouts.step + 1) % 16
        return dt
    resident = poses[:n_res]
    for lo in range(0, n_res, n_envs):                                   # the resident set
        for sim, pose in zip(sims, resident[lo:lo + n_envs]):
            place(sim, pose)
        step()
    fresh = iter(poses[n_res:])
    torch.cuda.synchronize()

    def miss_step():
        movers = set(arng.choice(n_envs, m, replace=False).tolist())
        for i, sim in enumerate(sims):
            place(sim, next(fresh) if i in movers else resident[int(arng.integers(0, len(resident)))])
        return step()
    return types.SimpleNamespace(name=name, step=miss_step, res=res, eng=eng, host=[], wall=[])


if not a.skip_steps:
    from bench_loader import make_scene
    sr = 16000
    tmp = "/dev/shm/ss_rir16_loader_bench" if os.path.isdir("/dev/shm") else "/tmp/ss_rir16_loader_bench"
    root = os.path.join(tmp, f"scene{sr}")
    rates = [float(x) for x in a.rates.split(",")]
    n_steps = a.warm + a.blocks * a.steps
    need = 4 * a.envs + n_steps * max(1, int(round(max(rates) * a.envs)))
    try:
        n_nodes = make_scene(root, sr, a.files, need + 64, np.random.default_rng(0))
        sources = O.synth_sources(np.random.default_rng(1), sr, k=8)
        emit(f"# 2. deferred-mode steps, {a.envs} envs at {sr} Hz, files on {tmp}; {a.blocks} blocks x {a.steps} steps per arm, arms "
             f"alternating block by block after {a.warm} warm-up steps each; us per step: host time of the resolver's call, median over "
             f"the steps | wall time of a block / steps, device synchronised, median (min) over the blocks")
        emit(f"{'rate':>5s} {'new poses':>9s} {'(a) half, three calls':>30s} {'(b) half, in call':>30s} {'(c) fp32 rows, in call':>30s} "
             f"{'b/a host':>8s} {'b/a wall':>8s} {'b/c wall':>8s} {'loaded in call a/b/c':>20s}")
        for rate in rates:
            m = max(1, int(round(rate * a.envs)))
            arms = [make_arm("a", root, sr, n_nodes, a.envs, m, n_steps, sources, False, dict(rir_rows="half")),
                    make_arm("b", root, sr, n_nodes, a.envs, m, n_steps, sources, True, dict(rir_rows="half")),
                    make_arm("c", root, sr, n_nodes, a.envs, m, n_steps, sources, True, {})]
            for arm in arms:
                for _ in range(a.warm):
                    arm.step()
            torch.cuda.synchronize()
            for blk in range(a.blocks):
                for arm in arms:
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        arm.host.append(arm.step())
                    torch.cuda.synchronize()
                    arm.wall.append((time.perf_counter() - t0) / a.steps)
            h = [1e6 * float(np.median(x.host)) for x in arms]
            w = [1e6 * float(np.median(x.wall)) for x in arms]
            wm = [1e6 * min(x.wall) for x in arms]
            emit(f"{rate:5.2f} {m:9d} " + " ".join(f"{h[i]:9.1f} | {w[i]:8.1f} ({wm[i]:7.1f})" for i in range(3)) +
                 f" {h[1] / h[0]:8.3f} {w[1] / w[0]:8.3f} {w[1] / w[2]:8.3f} " +
                 f"{'/'.join(str(int(x.res.library_loaded)) for x in arms):>20s}")
            assert arms[0].res.library_loaded == 0 and arms[1].res.library_loaded > 0
            del arms
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
