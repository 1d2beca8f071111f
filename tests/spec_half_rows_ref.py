"""The float64 model of tests/spec_half_ref.py for rows of up to three partition blocks (44.1 / 48 kHz), shared by
tests/test_spec_half_rows_host.py and tests/test_gpu_spec_half_rows.py.  The quantiser is spec_half_ref's, by import.

The model either quantises the block spectra it transforms itself (in float64, rounded to fp32), or - ``spectra=`` - takes the
halves and scales a bank holds (``bank_spectra``), i.e. the quantiser's decisions as they were made on the kernel's own fp32
spectra: the two differ in the few components per block (about 80 of 32 768) whose fp32 and fp64 values lie on either side of an
fp16 rounding boundary."""
import numpy as np

from spec_half_ref import KB, dequantise, quantise  # noqa: F401  (re-exported: the tests take all three from here)


def natural_components(rir_row):
    """rir_row [L] -> float32 [nbh, 2 kB]: the stored components of H'_i = 2 rFFT_{2kB}(rir[i kB:(i+1) kB]) in NATURAL order -
    (DC, Nyquist), then (re, im) of bins 1 .. kB - 1 - transformed in float64 and rounded to fp32"""
    rir_row = np.asarray(rir_row, np.float32)
    nbh = max(1, -(-len(rir_row) // KB))
    out = np.empty((nbh, 2 * KB), np.float32)
    for i in range(nbh):
        blk = np.zeros((2 * KB,), np.float64)
        seg = rir_row[i * KB:(i + 1) * KB]
        blk[:len(seg)] = seg
        hf = 2.0 * np.fft.rfft(blk)
        out[i, 0], out[i, 1] = hf[0].real, hf[KB].real
        out[i, 2::2], out[i, 3::2] = hf[1:KB].real, hf[1:KB].imag
    return out


def kernel_order(spectra_of):
    """The kernels store a block spectrum in the register order of their item stage.  -> int array perm [2 kB] with
    natural[n] = stored[perm[n]], found by transforming four random probe blocks with ``spectra_of`` (rows float32 [2, 2, kB] ->
    the library's fp32 block spectra [2, 2, 1, 2 kB]: ss_rir_spectra_f32 or its host build) and matching every natural component's
    four values to the stored position that holds them (nearest neighbour in four dimensions; checked to be a bijection)."""
    from scipy.spatial import cKDTree
    rows = np.random.default_rng(20240).standard_normal((2, 2, KB)).astype(np.float32)
    stored = np.asarray(spectra_of(rows), np.float64).reshape(4, 2 * KB).T
    nat = np.stack([natural_components(rows[e, c])[0] for e in range(2) for c in range(2)]).astype(np.float64).T
    dist, perm = cKDTree(stored).query(nat)
    assert np.array_equal(np.sort(perm), np.arange(2 * KB)) and dist.max() <= 1e-5 * np.abs(nat).max(), dist.max()
    return perm


def bank_spectra(q, scale, perm):
    """halves [..., 2 kB] and scales [...] of a half bank -> float32 [..., 2 kB]: float(q) * scale in natural order"""
    return dequantise(np.asarray(q), np.asarray(scale))[..., perm]


def _to_complex(v):
    h = np.empty(v.shape[:-1] + (KB + 1,), np.complex128)
    h[..., 0], h[..., KB] = v[..., 0], v[..., 1]
    h[..., 1:KB] = v[..., 2::2].astype(np.float64) + 1j * v[..., 3::2].astype(np.float64)
    return h


def block_spectra(rir_row, quant=True):
    """rir_row [L] -> float64 complex [nbh, kB + 1]: H'_i = 2 rFFT_{2kB}(rir[i kB:(i+1) kB]) rounded to fp32 and - quant - put
    through the half format (one scale per block, the 32768 stored components: (DC, Nyquist) packed, then the bins)"""
    rir_row = np.asarray(rir_row, np.float32)
    nbh = max(1, -(-len(rir_row) // KB))
    out = np.empty((nbh, KB + 1), np.complex128)
    for i in range(nbh):
        blk = np.zeros((2 * KB,), np.float64)
        seg = rir_row[i * KB:(i + 1) * KB]
        blk[:len(seg)] = seg
        hf = 2.0 * np.fft.rfft(blk)
        v = np.empty((2 * KB,), np.float32)
        v[0], v[1] = hf[0].real, hf[KB].real
        v[2::2], v[3::2] = hf[1:KB].real, hf[1:KB].imag
        if quant:
            q, s = quantise(v)
            v = dequantise(q, s)
        out[i, 0], out[i, KB] = v[0], v[1]
        out[i, 1:KB] = v[2::2].astype(np.float64) + 1j * v[3::2].astype(np.float64)
    return out


def model_audiogoal(source, rir, t0, out_len, quant=True, spectra=None):
    """out[c, t] = sum_k rir[c, k] x[t0 + t - k] (x zero outside the clip) for t < out_len <= 3 kB, as uniformly partitioned
    overlap-save with block kB: output block j is the last kB samples of irFFT(sum_i H'_i S_{j-i}),
    S_m = rFFT(x[t0 + (m-1) kB : t0 + (m+1) kB]) / 2.  source [S], rir [2, L] -> float64 [2, out_len].
    spectra (float32 [2, nbh, 2 kB], natural order: ``bank_spectra``) replaces the model's own transform and quantiser; rir is
    then not read."""
    assert out_len <= 3 * KB
    if spectra is None:
        rir = np.asarray(rir, np.float32)
        nbh = max(1, -(-rir.shape[1] // KB))
    else:
        nbh = spectra.shape[1]
    nby = -(-out_len // KB)
    lo = t0 - nbh * KB                                               # x[lo : t0 + nby kB], zero outside the clip
    x = np.zeros(((nbh + nby) * KB,), np.float64)
    src = np.asarray(source, np.float64)
    a, b = max(lo, 0), min(t0 + nby * KB, len(src))
    if b > a:
        x[a - lo:b - lo] = src[a:b]
    S = {m: np.fft.rfft(x[(m - 1 + nbh) * KB:(m + 1 + nbh) * KB]) / 2.0 for m in range(1 - nbh, nby)}
    out = np.zeros((2, nby * KB), np.float64)
    for c in range(2):
        h = block_spectra(rir[c], quant) if spectra is None else _to_complex(np.asarray(spectra[c], np.float32))
        for j in range(nby):
            y = np.zeros((KB + 1,), np.complex128)
            for i in range(nbh):
                y += h[i] * S[j - i]
            out[c, j * KB:(j + 1) * KB] = np.fft.irfft(y, 2 * KB)[KB:]
    return out[:, :out_len]
