"""Numpy references of the half-precision time-domain RIR rows (include/ss_hip.h "Half-precision time-domain rows"), shared by
tests/test_rir16_host.py and tests/test_gpu_time_rir16.py:

  quantise / dequantise   the format's rule - tests/spec_half_ref.py's, applied per (entry, ear) ROW instead of per block spectrum
  model_audiogoal         float64 convolution of the DEQUANTISED row, windowed as the oracle windows it (the unified formula of
                          oracle/ss_oracle.py: out[c, t] = sum_k h[c, k] x[t0 + t - k], x zero outside the clip); quant=False: the
                          same model on the row as it is
  model_spectrogram       the oracle's pooled log1p spectrogram of a model waveform
"""
import numpy as np
from scipy.signal import fftconvolve

from oracle import ss_oracle as O

from spec_half_ref import quantise as _quantise_blocks

KB = 16384
DIRECT_MACS = 600_000_000        # np.convolve (the direct sum) up to here; beyond, scipy's FFT path in float64 (~1e-15 of peak)


def quantise(rows):
    """fp32 rows [..., cap] (zero behind their length) -> (fp16 [..., cap], fp32 scales [...]): mx = max |v| of a row; mx == 0:
    halves +0, scale 1; else mx in [2^(e-1), 2^e): q = RNE_fp16(v * 2^(15-e)), scale = 2^(e-15)."""
    return _quantise_blocks(rows)


def dequantise(q, scale):
    """float(q) * scale, exact in fp32"""
    return q.astype(np.float32) * np.asarray(scale, np.float32)[..., None]


def _conv64(x, h):
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    if len(x) * len(h) <= DIRECT_MACS:
        return np.convolve(x, h)
    return fftconvolve(x, h)


def model_audiogoal(source, rir, t0, out_len, quant=True, n_valid=None):
    """source [S], rir float32 [2, L] -> float64 [2, out_len]: samples t < n_valid (default out_len) of the unified formula on
    the row put through the half format (quant) or as it is, zeros behind."""
    rir = np.asarray(rir, np.float32)
    if quant and rir.shape[1]:
        q, s = quantise(rir)
        rir = dequantise(q, s)
    n_valid = out_len if n_valid is None else n_valid
    L = rir.shape[1]
    src = np.asarray(source, np.float64)
    out = np.zeros((2, out_len), np.float64)
    lo, hi = max(0, t0 - L + 1), min(len(src), t0 + n_valid)         # the samples of x a row of n_valid outputs can see
    if L == 0 or hi <= lo:
        return out
    for c in range(2):
        full = _conv64(src[lo:hi], rir[c])                            # full[n] = sum_k h[k] x[lo + n - k]
        a = full[t0 - lo:t0 - lo + n_valid]
        out[c, :len(a)] = a
    return out


def model_spectrogram(wave):
    """[2, T] -> [65, T4, 2], the oracle's pooled log1p spectrogram (nav.py:86-100) of a float64 waveform"""
    return O.compute_spectrogram(np.asarray(wave, np.float64))
