"""Randomised parity sweep of the waveform-side entry points against the oracle (test infrastructure).

Every trial draws N (1-300), a row length (1 ... 70 000 samples: rows of a few samples, odd lengths, lengths not a multiple of 4
or of the hop, rows shorter than one STFT frame's reach), a pad mode, a sampling rate / mel-band count for the filter bank,
GCC-PHAT's lag range, an eps for log-mel and one for GCC-PHAT from {default, 1e-4, 1e-2, 1} and a level per row, log-uniform
over 1e-6 ... 1e2; fills [N, 2, len] with noise (some rows silent, some ears silent) and compares `ops.spectrogram`
(nav.py:86-100), `ops.logmel`, `ops.gccphat`, every subset of `ops.audio_features` (k_features) and `ops.intensity`
(avwan_sensors.py:91-100, rows of at least its 150 samples) with the float64 oracle, every row, at 1e-4 of the row's own peak
(GCC-PHAT too: a regularised row peaks far below the full scale 1.0; log-mel: of max(peak, 1), the log passes through 0).

What keeps the comparison well-conditioned (see level_cap): a regulariser only regularises when it outweighs the float32
rounding noise of the loudest bins, about 1e-2 level^2 for GCC-PHAT and 1e-4 level^2 for log-mel.  Rows shorter than one frame
(periodic under reflect padding, so most bins are empty), every draw of a non-default GCC-PHAT eps and reflect-padded rows under
2 s (masked_regime) get their level capped accordingly; nothing is then left out of the comparison.  GCC-PHAT's cap binds only
the rows GCC-PHAT is compared on: where it is the lower one, the same noise goes in twice, at the uncapped level for spectrogram,
log-mel and intensity and at the capped one for GCC-PHAT (stand-alone and fused).  The other rows at the
default eps = 1e-8 keep the whole level range and the
ill-conditioned-frame mask, which may drop at most 1 frame in 1000 of a trial (asserted; --oracle-only checks the draws on a CPU).

    python scripts/gpu_fuzz_features.py --trials 200 --seed 1 [--out profiles/r8/fuzz_features.txt]
    python scripts/gpu_fuzz_features.py --trials 200 --seed 1 --oracle-only      # no GPU: the draws and the mask's share only
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sound-spaces_amd"))

from oracle import ss_oracle as O                      # noqa: E402
from ss_amd import ops, planning as P                  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


def rel(got, ref, floor=0.0):
    """max |got - ref| / the row's own peak (at least `floor`)"""
    scale = max(np.abs(ref).max(), floor) if ref.size else 0.0
    if not got.size:
        return 0.0
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())


GCC_EPS_DEFAULT, MEL_EPS_DEFAULT = 1e-8, 1e-6
MASK_CAP = 1e-3                                            # share of a trial's frames the ill-conditioned-frame mask may drop
SHORT = 512                                                # rows below one frame: no mask, level capped
REFLECT_MASK_MIN, MASK_MIN_FRAMES = 32000, 5000            # see masked_regime


def masked_regime(n, pad, gcc_eps, frames):
    """where the ill-conditioned-frame mask applies: the default eps on rows of at least one frame.  Under reflect padding frame 0
    is symmetric about sample 0, so ALL its bins are real and about 1 such frame in 20 has a bin below the mask's threshold
    (measured with the oracle): that stays well under the cap only on rows of some 200 frames, so shorter reflect rows
    take the regularised regime (level_cap, nothing left out) instead - as do trials that compare fewer than MASK_MIN_FRAMES
    frames, where the cap would round to no frame at all."""
    return gcc_eps == GCC_EPS_DEFAULT and n >= (REFLECT_MASK_MIN if pad == "reflect" else SHORT) and frames >= MASK_MIN_FRAMES


def level_cap(n, pad, mel_eps, gcc_eps, frames):
    """-> (cap for the rows that spectrogram, log-mel and intensity see, cap for the rows GCC-PHAT sees): the largest level at
    which mel_eps / gcc_eps still outweigh the float32 noise of near-empty bins - needed where such bins are the rule (short
    rows) or where no frame may be left out (GCC-PHAT outside masked_regime).  GCC-PHAT's cap binds GCC-PHAT's rows only."""
    cap = min(1e2, 100.0 * np.sqrt(mel_eps)) if n < SHORT else 1e2
    return cap, (cap if masked_regime(n, pad, gcc_eps, frames) else min(cap, 10.0 * np.sqrt(gcc_eps)))


def draw(rng):
    N = int(rng.choice([1, 2, 3, 5, 16, 31, 64, 128, 129, 256, 300]))
    kind = rng.integers(0, 5)
    n = (int(rng.integers(1, 300)) if kind == 0 else int(rng.integers(300, 3000)) if kind == 1
         else int(rng.integers(3000, 70000)) if kind == 2
         else int(rng.choice([16000, 44100, 48000, 22050, 4000, 16001, 15999, 1, 2, 3, 159, 160, 161, 256, 257])))
    if N * n > 8_000_000:
        N = max(1, 8_000_000 // n)
    pad = str(rng.choice(["reflect", "constant"]))
    sr = int(rng.choice([16000, 44100, 48000, 22050]))
    n_mels = int(rng.choice([64, 40, 32]))                  # (bands wider than 64 bins - 20-band banks - are outside the ABI's
                                                            #  stated limit, include/ss_hip.h: SS_EINVAL)
    max_lag = int(rng.choice([32, 16, 8, 1]))
    mel_eps = float(rng.choice([MEL_EPS_DEFAULT, 1e-4, 1e-2, 1.0]))
    gcc_eps = float(rng.choice([GCC_EPS_DEFAULT, 1e-4, 1e-2, 1.0]))
    rows = list(range(N)) if N <= 48 else sorted(set(rng.integers(0, N, 48).tolist()))       # the rows that are compared
    frames = len(rows) * (1 + n // 160)
    hi, hi_gcc = level_cap(n, pad, mel_eps, gcc_eps, frames)
    level = 10.0 ** rng.uniform(-6.0, np.log10(hi), (N, 1, 1))          # log-uniform, per row
    level_gcc = level if hi_gcc == hi else 10.0 ** rng.uniform(-6.0, np.log10(hi_gcc), (N, 1, 1))
    x = rng.standard_normal((N, 2, n))
    if masked_regime(n, pad, gcc_eps, frames):
        # Unregularised PHAT: correlated ears (ear 1 = ear 0 delayed and scaled, plus 10 % noise), so that the row has a peak
        # near 0.9 to be measured against.  Bins 0 and 256 of a real frame are REAL: of white noise they fall below the mask's
        # threshold in about 1 frame per 1000 (measured with the oracle), more than the mask may drop - a pedestal and a
        # Nyquist tone of half the noise's level keep both bins 8 sigma away from zero.
        delay = int(rng.integers(0, 12))
        x[:, 1, delay:] = 0.7 * x[:, 0, :n - delay] + 0.1 * x[:, 1, delay:]
        x += 0.5 + 0.5 * (1 - 2 * (np.arange(n) & 1))
    xg = None if level_gcc is level else (x * level_gcc).astype(np.float32)   # the same noise at GCC-PHAT's own level
    x = (x * level).astype(np.float32)
    if level_gcc is level:
        xg = x
    if N > 2:
        for a in ((x,) if xg is x else (x, xg)):
            a[int(rng.integers(0, N))] = 0.0                 # a silent row
            a[int(rng.integers(0, N)), int(rng.integers(0, 2))] = 0.0  # a silent ear
    return dict(xg=xg, frames=frames, N=N, n=n, pad=pad, sr=sr, n_mels=n_mels, max_lag=max_lag, mel_eps=mel_eps, gcc_eps=gcc_eps, x=x, rows=rows)


def well_conditioned(row, d):
    """PHAT divides every bin by its own magnitude, so a bin whose spectrum is empty in either ear carries an arbitrary unit
    phase in ANY float32 evaluation: the rounding noise of a 512-point float32 STFT is a few 1e-7 of the frame's typical bin,
    so a bin at 1e-4 of the frame's median is off by a few 1e-3 rad, 1e-5 of the output.  At the default eps = 1e-8 frames with
    a bin below that are left out of the comparison (masked_regime); elsewhere eps regularises them (level_cap) and every frame
    is compared."""
    T = 1 + d["n"] // 160
    if not masked_regime(d["n"], d["pad"], d["gcc_eps"], d["frames"]):
        return np.ones(T, bool)
    row = row.astype(np.float64)
    X = [np.abs(O.stft(row[c], pad_mode=d["pad"])) for c in range(2)]
    return np.minimum(X[0].min(axis=0) / np.median(X[0], axis=0), X[1].min(axis=0) / np.median(X[1], axis=0)) > 1e-4


def describe(d):
    return (f"N={d['N']:3d} len={d['n']:5d} pad={d['pad']:8s} sr={d['sr']} mels={d['n_mels']} lag={d['max_lag']:2d} "
            f"mel_eps={d['mel_eps']:g} gcc_eps={d['gcc_eps']:g}")


def run_trial(rng, oracle_only=False):
    d = draw(rng)
    N, n, pad, sr, n_mels, max_lag, mel_eps, gcc_eps, x = (d[k] for k in ("N", "n", "pad", "sr", "n_mels", "max_lag", "mel_eps",
                                                                          "gcc_eps", "x"))
    names = ("spectrogram", "logmel", "gccphat")
    xg = d["xg"]                                             # the rows GCC-PHAT is compared on (x itself where no cap binds)
    if not oracle_only:
        xd = torch.from_numpy(x).to(DEV)
        xgd = xd if xg is x else torch.from_numpy(xg).to(DEV)
        ms, mw, _ = P.mel_filterbank_sparse(sr, n_mels)
        msd, mwd = torch.from_numpy(ms).to(DEV), torch.from_numpy(mw).to(DEV)
        got = {"spectrogram": ops.spectrogram(xd, pad).cpu().numpy(), "logmel": ops.logmel(xd, msd, mwd, mel_eps, pad).cpu().numpy(),
               "gccphat": ops.gccphat(xgd, max_lag, gcc_eps, pad).cpu().numpy()}
        fused = {}
        for k in range(1, 4):
            for want in itertools.combinations(names, k):
                out = ops.audio_features(xd, want, msd, mwd, mel_eps, max_lag, gcc_eps, pad)
                fused[want] = {w: out[w].cpu().numpy() for w in want}
                if "gccphat" in want and xg is not x:        # the same launch on GCC-PHAT's rows: its gccphat output counts
                    fused[want]["gccphat"] = ops.audio_features(xgd, want, msd, mwd, mel_eps, max_lag, gcc_eps,
                                                                pad)["gccphat"].cpu().numpy()
        inten = ops.intensity(xd).cpu().numpy() if n >= 150 else None
    worst, frames, masked = 0.0, 0, 0
    where = describe(d)
    for i in d["rows"]:
        both = bool(xg[i, 0].any() and xg[i, 1].any())
        well = well_conditioned(xg[i], d) if both else None
        if both:
            frames += well.size
            masked += int((~well).sum())
        if oracle_only:
            continue
        x64 = x[i].astype(np.float64)
        ref = {"spectrogram": O.compute_spectrogram(x64, pad_mode=pad), "logmel": O.compute_logmel(x64, sr, n_mels, mel_eps, pad),
               "gccphat": O.compute_gcc_phat(xg[i].astype(np.float64), max_lag, gcc_eps, pad)}
        for w in names:
            if w == "gccphat" and not both:
                continue                                       # 0 / (0 + eps): both sides are exact zeros or eps-noise
            if w == "gccphat":
                ref[w] = ref[w][:, well]                       # scale: the row's OWN oracle peak (over the frames compared)
                got_w = got[w][i][:, well]
            else:
                got_w = got[w][i]
            floor = 1.0 if w == "logmel" else 0.0            # log(mel + eps) passes through 0 (eps = 1): 1e-4 absolute there
            e = rel(got_w, ref[w], floor)
            assert e <= TOL, f"{w} row {i}: {e:.3e} ({where})"
            worst = max(worst, e)
            for want, outs in fused.items():
                if w in outs:
                    e = rel(outs[w][i][:, well] if w == "gccphat" else outs[w][i], ref[w], floor)
                    assert e <= TOL, f"audio_features{want}.{w} row {i}: {e:.3e} ({where})"
                    worst = max(worst, e)
        if inten is not None and x[i].max() > 0:
            r = float(O.intensity(x64)[0])
            e = abs(float(inten[i]) - r) / max(r, 1e-30)
            assert e <= TOL, f"intensity row {i}: {e:.3e} ({where})"
    assert masked <= MASK_CAP * frames, f"the mask dropped {masked} of {frames} frames ({where})"
    return where, worst, frames, masked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--oracle-only", action="store_true", help="no GPU: run the draws and the mask through the oracle alone")
    args = ap.parse_args()
    if not args.oracle_only:
        ops.init()
    lines, fails, worst_all, frames_all, masked_all = [], 0, 0.0, 0, 0
    t_start = time.time()
    for t in range(args.trials):
        rng = np.random.default_rng([args.seed, t])
        try:
            where, worst, frames, masked = run_trial(rng, args.oracle_only)
            worst_all = max(worst_all, worst)
            frames_all += frames
            masked_all += masked
            lines.append(f"trial {t:4d} ok   {where} worst={worst:.2e} masked={masked}/{frames}")
        except Exception as e:                          # noqa: BLE001 - a sweep reports every failing trial
            fails += 1
            lines.append(f"trial {t:4d} FAIL {type(e).__name__}: {e}")
        print(lines[-1], flush=True)
    tail = f"# features, {args.trials} trials, seed {args.seed}{' (oracle only)' if args.oracle_only else ''}: {fails} failed, " \
           f"worst relative error {worst_all:.2e} (tolerance {TOL:.0e}), masked frames {masked_all} of {frames_all} " \
           f"({masked_all / max(frames_all, 1):.1e}; cap per trial {MASK_CAP:.0e}), {time.time() - t_start:.0f} s"
    print(tail)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + [tail]) + "\n")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
