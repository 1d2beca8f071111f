#!/usr/bin/env python
"""The reference-exact pose-cache mode of the column observer, two ways on the same box in the same process:

  python   FastVectorAudioObserver(pose_cache=True): per-env dicts walked in Python, index tensors built from lists, two torch
           index dispatches per output and direction, a join under overlap (the comparator: unchanged code)
  native   ... native_pose_cache=True: the memo inside the step's C call (ss_ctx_observe_sims_memo), the row copies one
           k_memo_rows launch behind the render

16 / 128 / 256 envs at 16 kHz, 3-s sounds, a seeded walk over 128 poses per env in which about half the env-steps stand still
(hits) and the rest move to a random pose (a miss unless the env has been there in this episode); every env starts a new episode
with the other 3-s sound now and then (its map is dropped).  The two modes alternate, --reps times each, over the SAME walk; per
block of --steps steps after --warmup:
  host us / step       wall clock inside observe() only, no synchronise between steps (what the trainer's thread pays)
  us / dependent step  observe() then a device synchronise, per step (what a consumer that needs the rows waits for)
and the last step's rows of the two modes are compared bit for bit.  Needs the GPU.
usage: bench_pose_memo.py [--envs 16,128,256] [--steps 200] [--warmup 20] [--reps 3] [--out profiles/r7/pose_memo.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sound-spaces_amd")]
import numpy as np

SR, NODES = 16000, 32


def world(dev):
    from oracle import ss_oracle as O
    from ss_amd.renderer import RirStore
    from ss_amd.vector import RirIndex
    rng = np.random.default_rng(3)
    clips = [O.synth_sources(rng, SR, k=1, seconds=3)[0] for _ in range(2)]
    store = RirStore(slots=4 * NODES, cap=SR, device=dev, group=4)
    index = RirIndex(4)
    index.add_scene("scene", NODES)
    groups = [[np.ascontiguousarray(O.synth_rir(rng, SR, length=int(rng.integers(3000, 9000)), n=1)[0].T) for _ in range(4)]
              for _ in range(NODES)]
    bases = store.slot_many(list(range(NODES)), [(lambda g=g: g) for g in groups])
    for r, b in enumerate(bases):
        index.set(0, r, 0, b)
    return clips, store, index


def walk(n, steps, seed):
    """per step: (recv, rot, sound index, new-episode mask)"""
    rng = np.random.default_rng(seed)
    recv, rot, snd = rng.integers(0, NODES, n), rng.integers(0, 4, n) * 90, rng.integers(0, 2, n)
    out = []
    for _ in range(steps):
        move = rng.uniform(size=n) < 0.5
        recv = np.where(move, rng.integers(0, NODES, n), recv)
        rot = np.where(move, rng.integers(0, 4, n) * 90, rot)
        new = rng.uniform(size=n) < 0.02
        snd = np.where(new, 1 - snd, snd)
        out.append((recv.copy(), rot.copy(), snd.copy(), new))
    return out


def block(mode, n, clips, store, index, script, warmup, dev, dependent):
    import torch
    from ss_amd.context import AudioContext
    from ss_amd.vector import FastVectorAudioObserver, VectorSimState
    ctx = AudioContext(SR)
    ctx.set_rir_bank(store.bank.data, store.bank.lengths)
    ids = np.asarray([ctx.add_source(f"snd{k}", c) for k, c in enumerate(clips)])
    st = VectorSimState(n)
    st.audio_index[:] = 0
    st.src[:] = 0
    st.scene[:] = 0
    st.step_count[:] = 0
    st.duration[:] = 1 << 30
    obs = FastVectorAudioObserver(ctx, st, index, SR, pose_cache=True, native_pose_cache=(mode == "native"))
    assert obs.native_memo == (mode == "native")
    sg = torch.empty((n, 65, 26, 2), device=dev)
    spent, t_block = 0.0, 0.0
    for k, (recv, rot, snd, new) in enumerate(script):
        if k == warmup:
            torch.cuda.synchronize()
            spent, h0, m0 = 0.0, obs.pose_hits, obs.pose_misses
            t_block = time.perf_counter()
        st.recv[:], st.rot[:], st.sound[:] = recv, rot, ids[snd]
        st.audio_index[new] = 0
        st.dirty[:] = False
        t0 = time.perf_counter()
        obs.observe(spectrogram_out=sg)
        spent += time.perf_counter() - t0
        if dependent:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    t_block = time.perf_counter() - t_block
    steps = len(script) - warmup
    hits, misses = obs.pose_hits - h0, obs.pose_misses - m0
    return dict(host_us=1e6 * spent / steps, step_us=1e6 * t_block / steps, hit_share=hits / max(1, hits + misses),
                last=sg.clone(), audio_index=st.audio_index.copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="16,128,256")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "pose_memo.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pose_memo.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    clips, store, index = world(dev)
    lines = [f"# bench_pose_memo.py on {torch.cuda.get_device_name(0)}: {a.steps} steps after {a.warmup}, {a.reps} alternating blocks per mode, "
             f"16 kHz, spectrogram rows, 3-s sounds, {4 * NODES} poses",
             "# envs mode    hit_share  host_us/step (median [min..max])   us/dependent_step (median [min..max])"]
    for n in (int(v) for v in a.envs.split(",")):
        script = walk(n, a.warmup + a.steps, 100 + n)
        res = {"python": {"host": [], "dep": []}, "native": {"host": [], "dep": []}}
        share = {}
        for rep in range(a.reps):
            last = {}
            for mode in ("python", "native"):
                free = block(mode, n, clips, store, index, script, a.warmup, dev, dependent=False)
                dep = block(mode, n, clips, store, index, script, a.warmup, dev, dependent=True)
                res[mode]["host"].append(free["host_us"])
                res[mode]["dep"].append(dep["step_us"])
                share[mode] = free["hit_share"]
                last[mode] = free
            assert torch.equal(last["python"]["last"], last["native"]["last"]), "the two modes disagree"
            assert np.array_equal(last["python"]["audio_index"], last["native"]["audio_index"])
        for mode in ("python", "native"):
            h, d = np.asarray(res[mode]["host"]), np.asarray(res[mode]["dep"])
            lines.append(f"{n:6d} {mode:7s} {share[mode]:9.3f}  {np.median(h):8.1f} [{h.min():.1f}..{h.max():.1f}]"
                         f"{'':10s}{np.median(d):8.1f} [{d.min():.1f}..{d.max():.1f}]")
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
