"""Sensitivity guard for parity tests with multi-block RIRs.

A parity check passes when max|got - ref| <= 1e-4 max|ref| per unit.  With a decaying RIR the partition blocks after the
first one or two (planning.KB taps each) lie far below that, so a kernel that skipped or misplaced them would still pass.
The guard proves, for the inputs a test actually renders, that this cannot happen.  The oracle output is linear in the
RIR, so it is computed one partition block at a time (the RIR with every other block zeroed, at its full length so the
oracle takes the same branch) and then checks:

  (a) the block contributions sum to the reference within 1e-6 of its peak;
  (b) every block of every ear of every RIR reaches BLOCK_FLOOR of the unit's peak in some unit;
  (c) every block-edge tap (first and last of each block) of every ear reaches EDGE_FLOOR of the peak in some unit,
      computed directly as |h[k]| * max_t |x[t0 + t - k]|.

Everything is float64; ``check`` returns the float64 references of the units, which the tests compare against.
"""
import hashlib

import numpy as np

from oracle import ss_oracle as O

KB = 16384
BLOCK_FLOOR = 1e-2          # 100 x the parity tolerance
EDGE_FLOOR = 1e-3
SUM_TOL = 1e-6

_CACHE = {}


def _digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.blake2b(a.tobytes() + str((a.dtype, a.shape)).encode(), digest_size=12).hexdigest()


class Term:
    """One RIR applied to one source window.  kind "sim": SS1.0 window (conv_window_fft at t0, out_len samples);
    kind "cont": SS2.0 step (convolve_with_rir at sample_index, step_time; out_len = sr).  ``weight`` [out_len] is a
    per-sample gain applied after the convolution (the two halves of a cross-fade); ``name`` labels failures."""

    def __init__(self, source, rir_wav, kind="sim", t0=0, out_len=None, sr=None, sample_index=0, step_time=0.25,
                 weight=None, name=None):
        assert kind in ("sim", "cont")
        self.source = np.asarray(source, np.float32)
        self.rir = np.asarray(rir_wav, np.float32)              # [L, 2] wav layout
        assert self.rir.ndim == 2 and self.rir.shape[1] == 2
        self.kind, self.t0, self.sr, self.sample_index, self.step_time = kind, int(t0), sr, int(sample_index), step_time
        self.out_len = int(sr if kind == "cont" else out_len)
        self.weight = None if weight is None else np.asarray(weight, np.float64)
        self.rir_key = _digest(self.rir)
        self.name = name or f"rir[{self.rir.shape[0]} taps #{self.rir_key[:6]}]"

    def _window_key(self):
        return (_digest(self.source), self.rir_key, self.kind, self.t0, self.out_len, self.sr, self.sample_index,
                self.step_time, None if self.weight is None else _digest(self.weight))

    def _oracle(self, h):
        x = self.source.astype(np.float64)
        if self.kind == "sim":
            return O.conv_window_fft(x, h, self.t0, self.out_len).astype(np.float64)
        return O.convolve_with_rir(x, h, self.sr, self.sample_index, self.step_time).astype(np.float64)

    def _shifted(self, k):
        """x[t0 + t - k] for the output samples t this term writes (zeros elsewhere), float64 [out_len]."""
        S, out = len(self.source), np.zeros(self.out_len)
        if self.kind == "sim":
            n = self.t0 + np.arange(self.out_len) - k
            ok = (n >= 0) & (n < S)
        else:
            num = int(self.sr * self.step_time)
            n = self.sample_index + np.arange(num) - k
            if self.sample_index - self.rir.shape[0] >= 0:     # steady branch: wraps around the clip end
                n = np.where(n >= S, n - S, n)
            ok = (n >= 0) & (n < S)
            ok = np.concatenate([ok, np.zeros(self.out_len - num, bool)])
            n = np.concatenate([n, np.zeros(self.out_len - num, int)])
        out[ok] = self.source[n[ok]]
        return out

    def blocks(self):
        """(contributions [nb, 2, out_len], full oracle [2, out_len], edge [nb, 2 taps, 2 ears] = |h[k]| max|x(k)|),
        weighted, cached per (source, window, RIR)."""
        key = self._window_key()
        if key not in _CACHE:
            h = self.rir.astype(np.float64)
            L = h.shape[0]
            nb = max(1, -(-L // KB))
            w = 1.0 if self.weight is None else self.weight
            full = self._oracle(h) * w
            parts = np.zeros((nb,) + full.shape)
            edge = np.zeros((nb, 2, 2))
            for b in range(nb):
                lo, hi = b * KB, min(L, (b + 1) * KB)
                hb = np.zeros_like(h)
                hb[lo:hi] = h[lo:hi]
                parts[b] = self._oracle(hb) * w
                for e, k in enumerate((lo, hi - 1)):
                    edge[b, e] = np.abs(h[k]) * np.abs(self._shifted(k) * w).max()
            _CACHE[key] = (parts, full, edge)
        return _CACHE[key]


def check(units, block_floor=BLOCK_FLOOR, edge_floor=EDGE_FLOOR):
    """units: list of units, each a Term or a list of Terms (summed: distractor, cross-fade halves).  Asserts (a)-(c)
    (module docstring) and returns the float64 reference [2, out_len] of each unit."""
    refs, best_block, best_edge, names = [], {}, {}, {}
    for u, terms in enumerate(units):
        terms = [terms] if isinstance(terms, Term) else list(terms)
        got = [t.blocks() for t in terms]
        ref = sum(g[1] for g in got)
        peak = np.abs(ref).max()
        assert peak > 0, f"unit {u}: the reference is all zeros"
        for t, (parts, full, edge) in zip(terms, got):
            err = np.abs(parts.sum(axis=0) - full).max()
            assert err <= SUM_TOL * peak, f"unit {u}, {t.name}: block contributions miss the reference by {err / peak:.2e}"
            names[t.rir_key] = t.name
            bb = np.abs(parts).max(axis=2) / peak                     # [nb, ear]
            be = edge / peak                                          # [nb, tap, ear]
            best_block[t.rir_key] = np.maximum(best_block.get(t.rir_key, 0.0), bb)
            best_edge[t.rir_key] = np.maximum(best_edge.get(t.rir_key, 0.0), be)
        refs.append(ref)
    for key, bb in best_block.items():
        for b, c in zip(*np.nonzero(bb < block_floor)):
            raise AssertionError(f"{names[key]}: block {b} (taps {b * KB}..) of ear {c} reaches only {bb[b, c]:.2e} of "
                                 f"peak in any unit (< {block_floor:g}): a kernel could drop it unnoticed")
        be = best_edge[key]
        for b, e, c in zip(*np.nonzero(be < edge_floor)):
            raise AssertionError(f"{names[key]}: the {'first' if e == 0 else 'last'} tap of block {b} (ear {c}) reaches "
                                 f"only {be[b, e, c]:.2e} of peak in any unit (< {edge_floor:g})")
    return refs


def crossfade_weights(sr, out_len=None):
    """Per-sample gains (previous, current) of the oracle's crossfade() (continuous_simulator.py:47-53), out_len = sr."""
    n = int(0.05 * sr)
    out_len = sr if out_len is None else out_len
    w2 = np.ones(out_len)
    w2[:n + 1] = np.arange(n + 1) / n
    w1 = np.zeros(out_len)
    w1[:n + 1] = np.flip(np.arange(n + 1) / n)
    return w1, w2


def wav(planar_rir):
    """[2, L] planar -> [L, 2] wav layout (contiguous)."""
    return np.ascontiguousarray(np.asarray(planar_rir).T)
