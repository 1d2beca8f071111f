"""Numpy references of the half-precision spectral RIR bank (include/ss_hip.h "Half-precision spectral bank"), shared by
tests/test_spec_half_host.py and tests/test_gpu_spec_half.py:

  quantise / dequantise   the format's rule applied to fp32 block spectra [..., SPEC_FLOATS]
  model_audiogoal         the partitioned overlap-save convolution the kernels compute, in float64, with the quantiser applied to
                          every block spectrum 2*rFFT_{2kB}(rir block) (quant=False: the same model without it)
"""
import numpy as np

KB = 16384


def quantise(spec):
    """fp32 block spectra [..., F] -> (fp16 [..., F], fp32 scales [...]).  mx = max |v| of a block; mx == 0: halves +0, scale 1;
    else mx in [2^(e-1), 2^e) (frexp): q = RNE_fp16(v * 2^(15-e)), scale = 2^(e-15)."""
    spec = np.asarray(spec, np.float32)
    mx = np.abs(spec).max(axis=-1)
    _, e = np.frexp(mx)
    e = np.where(mx > 0, e, 15).astype(np.int32)
    with np.errstate(over="raise"):
        q = np.ldexp(spec, (15 - e)[..., None]).astype(np.float32).astype(np.float16)      # astype(float16): round to nearest even
    q = np.where((mx > 0)[..., None], q, np.float16(0))
    return q, np.ldexp(np.float32(1), e - 15).astype(np.float32)


def dequantise(q, scale):
    """float(q) * scale, exact in fp32"""
    return q.astype(np.float32) * np.asarray(scale, np.float32)[..., None]


def model_audiogoal(source, rir, t0, out_len, quant=True):
    """out[c, t] = sum_k rir[c, k] x[t0 + t - k] (x zero outside the clip) for t < out_len <= kB, as uniformly partitioned
    overlap-save with block kB: Y = sum_i H'_i S_{-i}, H'_i = 2 rFFT_{2kB}(rir[c, i kB:(i+1) kB]) rounded to fp32 and - quant - put
    through the half format, S_m = rFFT(x[t0 + (m-1) kB : t0 + (m+1) kB]) / 2; out = the last kB samples of irFFT(Y).
    source [S], rir [2, L] -> float64 [2, out_len]"""
    assert out_len <= KB
    rir = np.asarray(rir, np.float32)
    L = rir.shape[1]
    nbh = max(1, -(-L // KB))
    x = np.zeros(((nbh + 1) * KB + 0,), np.float64)                  # x[t0 - nbh kB : t0 + kB], zero outside the clip
    lo = t0 - nbh * KB
    src = np.asarray(source, np.float64)
    a, b = max(lo, 0), min(t0 + KB, len(src))
    if b > a:
        x[a - lo:b - lo] = src[a:b]
    out = np.zeros((2, out_len), np.float64)
    for c in range(2):
        y = np.zeros((KB + 1,), np.complex128)
        for i in range(nbh):
            blk = np.zeros((2 * KB,), np.float64)
            seg = rir[c, i * KB:(i + 1) * KB]
            blk[:len(seg)] = seg
            hf = 2.0 * np.fft.rfft(blk)
            v = np.empty((2 * KB,), np.float32)                      # the 32768 stored components: (DC, Nyquist) packed, then bins
            v[0], v[1] = hf[0].real, hf[KB].real
            v[2::2], v[3::2] = hf[1:KB].real, hf[1:KB].imag
            if quant:
                q, s = quantise(v)
                v = dequantise(q, s)
            h = np.empty((KB + 1,), np.complex128)
            h[0], h[KB] = v[0], v[1]
            h[1:KB] = v[2::2].astype(np.float64) + 1j * v[3::2].astype(np.float64)
            m = -i                                                   # S_m over x[t0 + (m-1) kB : t0 + (m+1) kB]
            w = x[(m - 1) * KB + nbh * KB:(m + 1) * KB + nbh * KB]
            y += h * (np.fft.rfft(w) / 2.0)
        out[c] = np.fft.irfft(y, 2 * KB)[KB:KB + out_len]
    return out
