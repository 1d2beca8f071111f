#!/usr/bin/env python
"""Captured steps against eager launches: one step = ss_source_windows_f32 + ss_audio_obs_f32 (the stateless entries, bound ctypes
calls) on ONE side stream, over the same tensors, in two arms:

  (e) eager    the two calls issued on the stream
  (g) replay   the same two calls captured once with ss_amd.graphs.capture (ss_stream_reserve, then a torch.cuda.CUDAGraph on that
               stream; a captured k_obs_blocks launch is k_sync_next + k_obs_blocks) and replayed with Captured.replay(fence=False)

at 5 and 10 units of 44.1 kHz (k_obs_blocks, fp32 time-domain rows of 44 100 taps) and at 16 units of 16 kHz (the fused one-block
kernel; warm-up call instead of the reserve).  Two figures per arm, both in us per step, median (min) over the rounds:

  chain    `--launches` steps issued back to back, HIP events around them on the stream: the stream's throughput
  step     ONE step issued, then the host waits for the stream (perf_counter around both): the dependent step a trainer sees

One pass, the arms ALTERNATING round by round in one process after a warm-up of both.  The replay's spectrogram is compared with
the eager one once per point (equal bits expected).

--parent-lib FILE: a libss_hip.so built from the PARENT commit, loaded next to this tree's.  The eager ss_audio_obs_f32 step at
5 units of 44.1 kHz (k_obs_blocks; the only device-side change to an eager launch is the test of a null pointer) is then timed
through both libraries, alternating, events on the stream, same tensors: median (min) and the ratio.

usage: python scripts/kbench_graph_replay.py [--out FILE] [--rounds 9] [--launches 40] [--parent-lib FILE]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--launches", type=int, default=40, help="steps per arm and round of the chain figure")
ap.add_argument("--singles", type=int, default=40, help="steps per arm and round of the dependent-step figure")
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()

import numpy as np
import torch
from oracle import ss_oracle as O
from ss_amd import _lib, graphs
from ss_amd import planning as P
from ss_amd.ops import FLAG_NO_DISTRACTOR

assert torch.cuda.is_available(), "kbench_graph_replay needs the GPU: there is no CPU timing of this path"
dev = torch.device("cuda:0")
LIB = _lib.load()
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def bind(lib):
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.ss_audio_obs_f32.argtypes = [vp, vp, vp, vp, vp, vp, ci, ll, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.ss_audio_obs_f32.restype = ci
    return lib


N_SOUNDS, N_BANK = 8, 64


def point(sr, n_units, rng):
    """-> the tensors of one step of n_units units at sr: 1-s clips, t0 = 0, every unit a sound and a bank entry of its own pick,
    one window set per unit (what the step's first launch transforms), RIRs of sr taps"""
    clips = O.synth_sources(rng, sr, k=N_SOUNDS)
    cap = sr + (sr & 1)
    rows = torch.from_numpy(np.ascontiguousarray(np.pad(O.synth_rir(rng, sr, n=N_BANK), ((0, 0), (0, 0), (0, cap - sr))))).to(dev)
    nbh, nby = P.ceil_div(cap, P.KB), P.ceil_div(sr, P.KB)
    wds, desc, slot = [], np.zeros((n_units, 8), np.int32), 0
    for n in range(n_units):
        s = int(rng.integers(0, N_SOUNDS))
        ws = P.plan_window_set(sr, 0, nbh, nby)
        wds.append(P.window_desc_rows(ws, s * sr, sr))
        desc[n] = P.unit_desc_row(int(rng.integers(0, N_BANK)), slot, ws)
        slot += ws.count
    wd = np.ascontiguousarray(np.concatenate(wds), np.int32)
    return dict(src=torch.from_numpy(np.ascontiguousarray(clips.reshape(-1))).to(dev), wd=torch.from_numpy(wd).to(dev),
                spec=torch.empty((len(wd), P.SPEC_FLOATS), device=dev), desc=torch.from_numpy(desc).to(dev), rows=rows,
                lengths=torch.full((N_BANK,), sr, dtype=torch.int32, device=dev),
                sg=torch.empty((n_units,) + P.spectrogram_shape(sr), device=dev), cap=cap, sr=sr, n=n_units)


def obs_of(lib, pt, stream_of):
    """the observation call through `lib` on stream_of() (a raw handle, asked per call: the capture runs the same closure)"""
    sp, ln, ds, o = pt["spec"].data_ptr(), pt["lengths"].data_ptr(), pt["desc"].data_ptr(), pt["sg"].data_ptr()
    rows, cap, n, sr = pt["rows"].data_ptr(), pt["cap"], pt["n"], pt["sr"]

    def obs():
        assert lib.ss_audio_obs_f32(sp, rows, ln, ds, None, o, n, 2 * cap, cap, 1, cap, sr, sr, 0, FLAG_NO_DISTRACTOR, stream_of()) == 0
    return obs


def windows_of(lib, pt, stream_of):
    src, wd, sp, w = pt["src"].data_ptr(), pt["wd"].data_ptr(), pt["spec"].data_ptr(), int(pt["wd"].shape[0])

    def windows():
        assert lib.ss_source_windows_f32(src, wd, sp, w, stream_of()) == 0
    return windows


def events(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3


def singles(fn, count, stream):
    ts = []
    with torch.cuda.stream(stream):
        for _ in range(count):
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def fmt(x):
    return f"{float(np.median(x)):7.1f} ({min(x):6.1f})"


rng = np.random.default_rng(0)
emit(f"# kbench_graph_replay on {torch.cuda.get_device_name(0)}: {a.rounds} rounds, arms alternating; chain: {a.launches} steps back to "
     f"back between two events; step: {a.singles} single steps, each followed by a stream synchronise; us per step, median (min)")
emit(f"{'rate':>6s} {'units':>5s} {'eager chain':>16s} {'replay chain':>16s} {'g/e':>6s} {'eager step':>16s} {'replay step':>16s} {'g/e':>6s} {'bits':>5s}")
side = torch.cuda.Stream()
for sr, n_units in ((44100, 5), (44100, 10), (16000, 16)):
    pt = point(sr, n_units, rng)
    raw = lambda: torch._C._cuda_getCurrentRawStream(0)
    obs, windows = obs_of(LIB, pt, raw), windows_of(LIB, pt, raw)

    def step():
        windows()
        obs()

    with torch.cuda.stream(side):
        for _ in range(a.warm):
            step()
    torch.cuda.synchronize()
    ref = pt["sg"].clone()
    reserve = dict(out_len=sr, rir_cap=pt["cap"], n_terms=1) if sr > P.KB else None
    capd = graphs.capture(step, stream=side, reserve=reserve)
    pt["sg"].fill_(float("nan"))
    capd.replay()
    torch.cuda.synchronize()
    same = torch.equal(pt["sg"], ref)
    replay = lambda: capd.replay(fence=False)
    for _ in range(a.warm):
        replay()
    torch.cuda.synchronize()
    t = dict(ec=[], gc=[], es=[], gs=[])
    for _ in range(a.rounds):
        t["ec"].append(events(step, a.launches, side))
        t["gc"].append(events(replay, a.launches, side))
        t["es"].append(singles(step, a.singles, side))
        t["gs"].append(singles(replay, a.singles, side))
    emit(f"{sr:6d} {n_units:5d} {fmt(t['ec'])} {fmt(t['gc'])} {np.median(t['gc']) / np.median(t['ec']):6.3f} "
         f"{fmt(t['es'])} {fmt(t['gs'])} {np.median(t['gs']) / np.median(t['es']):6.3f} {'equal' if same else 'DIFF':>5s}")
    if sr == 44100 and n_units == 5 and a.parent_lib:
        par = bind(ctypes.CDLL(os.path.abspath(a.parent_lib)))
        assert par.ss_init() == 0
        obs_par = obs_of(par, pt, raw)
        with torch.cuda.stream(side):
            for _ in range(a.warm):
                obs_par(); obs()
        torch.cuda.synchronize()
        tp, tn = [], []
        for _ in range(a.rounds):
            tp.append(events(obs_par, a.launches, side))
            tn.append(events(obs, a.launches, side))
        emit(f"# eager ss_audio_obs_f32 (k_obs_blocks), 5 units of 44.1 kHz, events on the stream: parent {fmt(tp)}  this tree {fmt(tn)}  "
             f"this / parent = {np.median(tn) / np.median(tp):.3f}")
        emit(f"#   the rounds: parent {min(tp):.1f} .. {max(tp):.1f} (spread {(max(tp) - min(tp)) / np.median(tp):.3f} of its median)  "
             f"this tree {min(tn):.1f} .. {max(tn):.1f}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
