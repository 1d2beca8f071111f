"""Tensor-level entry points of the HIP audio path + their registration as PyTorch custom ops
(``torch.ops.ss_hip.*``).  PyTorch is plumbing here: device memory, streams, dispatch.  Every op runs the
hand-written gfx950 kernels of csrc/ through the C ABI (include/ss_hip.h) on the caller's current stream;
nothing syncs the host.

Reference call sites replaced (facebookresearch/sound-spaces):
  fftconv_binaural  soundspaces/simulator.py:629-647,649-664  (scipy.signal.fftconvolve per ear + slicing)
  spectrogram       soundspaces/tasks/nav.py:86-100           (librosa.stft -> abs -> 4x4 mean -> log1p)
  audio_obs         soundspaces/simulator.py:690-701          (both, fused; cache-miss path)
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .planning import KB, SPEC_FLOATS, ceil_div, spectrogram_shape

PAD_REFLECT, PAD_CONSTANT = 0, 1
FLAG_NO_DISTRACTOR = 1      # SS_FLAG_NO_DISTRACTOR: every unit descriptor has term 1 absent
FLAG_CROSSFADE = 2          # SS_FLAG_CROSSFADE: term 1 = previous step's RIR, blended over the first int(0.05*sr)+1 samples
FLAG_FIRST_BUCKET = 4       # SS_FLAG_FIRST_BUCKET: every bank index of the launch lies in bucket 0 of a bucketed bank

_PAD = {"reflect": PAD_REFLECT, "constant": PAD_CONSTANT, 0: 0, 1: 1}


def _stream(t: "torch.Tensor" = None) -> int:
    """Raw handle of the current stream of ``t``'s device (of the current device without ``t``).  Not
    ``torch.cuda.current_stream(None).cuda_stream``: that is ~10 us of device-index plumbing and object construction per call,
    a tenth of an eager (batch-1) observation."""
    idx = t.device.index if (t is not None and t.device.index is not None) else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.SsHipError(f"{name} must live on the GPU (got {t.device}); this path has no CPU implementation")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


def _bank_strides(rir_bank: torch.Tensor, interleaved: bool):
    if rir_bank.dim() != 3:
        raise ValueError("rir_bank must be [R,2,L] (planar) or [R,L,2] (wav-interleaved)")
    if interleaved:
        R, cap, two = rir_bank.shape
        assert two == 2
        return 2 * cap, 1, 2, cap
    R, two, cap = rir_bank.shape
    assert two == 2
    return 2 * cap, cap, 1, cap


def init() -> None:
    """Build the per-device constant tables (idempotent); also the explicit 'is the HIP path alive' probe."""
    _lib.check(_lib.load().ss_init(), "ss_init")


def source_windows_into(src: torch.Tensor, win_desc: torch.Tensor, spec_out: torch.Tensor) -> None:
    _chk(src, torch.float32, "src"); _chk(win_desc, torch.int32, "win_desc"); _chk(spec_out, torch.float32, "spec_out")
    W = win_desc.shape[0]
    assert win_desc.shape == (W, 4) and spec_out.numel() >= W * SPEC_FLOATS
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().ss_source_windows_f32(src.data_ptr(), win_desc.data_ptr(), spec_out.data_ptr(), W,
                                                     _stream(src)), "ss_source_windows_f32")


def source_windows(src: torch.Tensor, win_desc: torch.Tensor) -> torch.Tensor:
    out = torch.empty((win_desc.shape[0], SPEC_FLOATS), dtype=torch.float32, device=src.device)
    source_windows_into(src, win_desc, out)
    return out


def fftconv_binaural_into(spec, rir_bank, rir_len, unit_desc, out, n_valid: int, interleaved: bool = False,
                          flags: int = 0) -> None:
    _chk(spec, torch.float32, "spec"); _chk(rir_bank, torch.float32, "rir_bank"); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(out, torch.float32, "out")
    N, two, out_len = out.shape
    assert two == 2 and unit_desc.shape == (N, 8)
    us, cs, es, cap = _bank_strides(rir_bank, interleaved)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().ss_fftconv_binaural_f32(spec.data_ptr(), rir_bank.data_ptr(), rir_len.data_ptr(),
                                                       unit_desc.data_ptr(), out.data_ptr(), N, us, cs, es, cap,
                                                       n_valid, out_len, flags, _stream(spec)), "ss_fftconv_binaural_f32")


def fftconv_binaural(spec, rir_bank, rir_len, unit_desc, n_valid: int, out_len: int, interleaved: bool = False,
                     flags: int = 0):
    out = torch.empty((unit_desc.shape[0], 2, out_len), dtype=torch.float32, device=spec.device)
    fftconv_binaural_into(spec, rir_bank, rir_len, unit_desc, out, n_valid, interleaved, flags)
    return out


def spectrogram_into(x: torch.Tensor, out: torch.Tensor, pad_mode="reflect") -> None:
    _chk(x, torch.float32, "x"); _chk(out, torch.float32, "out")
    N, two, n = x.shape
    assert two == 2 and tuple(out.shape) == (N,) + spectrogram_shape(n)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ss_spectrogram_f32(x.data_ptr(), out.data_ptr(), N, n, _PAD[pad_mode], _stream(x)),
                   "ss_spectrogram_f32")


def spectrogram(x: torch.Tensor, pad_mode="reflect") -> torch.Tensor:
    out = torch.empty((x.shape[0],) + spectrogram_shape(x.shape[2]), dtype=torch.float32, device=x.device)
    spectrogram_into(x, out, pad_mode)
    return out


def logmel_into(x: torch.Tensor, out: torch.Tensor, mel_start: torch.Tensor, mel_w: torch.Tensor, eps: float = 1e-6,
                pad_mode="reflect") -> None:
    """EXTENSION (not in the reference): out[n, j, t, c] = log(sum_i mel_w[j, i] |STFT(x[n, c])[mel_start[j]+i, t]|^2 + eps).
    mel_start int32 [n_mels], mel_w float32 [n_mels, max_len] on the device (planning.mel_filterbank_sparse)."""
    _chk(x, torch.float32, "x"); _chk(out, torch.float32, "out"); _chk(mel_start, torch.int32, "mel_start")
    _chk(mel_w, torch.float32, "mel_w")
    N, two, n = x.shape
    n_mels, max_len = mel_w.shape
    assert two == 2 and mel_start.shape == (n_mels,) and tuple(out.shape) == (N, n_mels, 1 + n // 160, 2)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ss_logmel_f32(x.data_ptr(), out.data_ptr(), N, n, _PAD[pad_mode], mel_start.data_ptr(),
                                             mel_w.data_ptr(), n_mels, max_len, float(eps), _stream(x)), "ss_logmel_f32")


def logmel(x: torch.Tensor, mel_start: torch.Tensor, mel_w: torch.Tensor, eps: float = 1e-6, pad_mode="reflect"):
    out = torch.empty((x.shape[0], mel_w.shape[0], 1 + x.shape[2] // 160, 2), dtype=torch.float32, device=x.device)
    logmel_into(x, out, mel_start, mel_w, eps, pad_mode)
    return out


def gccphat_into(x: torch.Tensor, out: torch.Tensor, max_lag: int = 32, eps: float = 1e-8, pad_mode="reflect") -> None:
    """EXTENSION (not in the reference): per-frame GCC-PHAT between the two ears,
    out[n, i, t] = irfft(G / (|G| + eps))[(i - max_lag) mod 512], G = STFT(x[n, 0]) conj(STFT(x[n, 1]))."""
    _chk(x, torch.float32, "x"); _chk(out, torch.float32, "out")
    N, two, n = x.shape
    assert two == 2 and tuple(out.shape) == (N, 2 * max_lag + 1, 1 + n // 160)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ss_gccphat_f32(x.data_ptr(), out.data_ptr(), N, n, _PAD[pad_mode], int(max_lag),
                                              float(eps), _stream(x)), "ss_gccphat_f32")


def gccphat(x: torch.Tensor, max_lag: int = 32, eps: float = 1e-8, pad_mode="reflect") -> torch.Tensor:
    out = torch.empty((x.shape[0], 2 * max_lag + 1, 1 + x.shape[2] // 160), dtype=torch.float32, device=x.device)
    gccphat_into(x, out, max_lag, eps, pad_mode)
    return out


def audio_features_into(x: torch.Tensor, spectrogram_out=None, logmel_out=None, gccphat_out=None, mel_start=None, mel_w=None,
                        mel_eps: float = 1e-6, max_lag: int = 32, gcc_eps: float = 1e-8, pad_mode="reflect") -> None:
    """EXTENSION: every STFT-derived feature from ONE pass over the waveform x [N, 2, n] (``ss_audio_features_f32``): any
    subset of the pooled spectrogram [N,65,T4,2] (nav.py:86-100), log-mel [N,n_mels,T,2] and GCC-PHAT [N,2*max_lag+1,T];
    same results as ``spectrogram_into`` / ``logmel_into`` / ``gccphat_into``, which each re-read x and redo the STFT."""
    _chk(x, torch.float32, "x")
    N, two, n = x.shape
    assert two == 2 and (spectrogram_out is not None or logmel_out is not None or gccphat_out is not None)
    n_mels = max_len = 0
    if spectrogram_out is not None:
        _chk(spectrogram_out, torch.float32, "spectrogram_out")
        assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(n)
    if logmel_out is not None:
        _chk(logmel_out, torch.float32, "logmel_out"); _chk(mel_start, torch.int32, "mel_start"); _chk(mel_w, torch.float32, "mel_w")
        n_mels, max_len = mel_w.shape
        assert mel_start.shape == (n_mels,) and tuple(logmel_out.shape) == (N, n_mels, 1 + n // 160, 2)
    if gccphat_out is not None:
        _chk(gccphat_out, torch.float32, "gccphat_out")
        assert tuple(gccphat_out.shape) == (N, 2 * max_lag + 1, 1 + n // 160)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ss_audio_features_f32(x.data_ptr(), N, n, _PAD[pad_mode], ptr(spectrogram_out), ptr(logmel_out),
                                                     ptr(mel_start), ptr(mel_w), int(n_mels), int(max_len), float(mel_eps),
                                                     ptr(gccphat_out), int(max_lag), float(gcc_eps), _stream(x)),
                   "ss_audio_features_f32")


def audio_features(x: torch.Tensor, want=("logmel", "gccphat"), mel_start=None, mel_w=None, mel_eps: float = 1e-6,
                   max_lag: int = 32, gcc_eps: float = 1e-8, pad_mode="reflect"):
    """-> dict of the wanted features ("spectrogram", "logmel", "gccphat"), one launch."""
    N, _, n = x.shape
    out = {}
    if "spectrogram" in want:
        out["spectrogram"] = torch.empty((N,) + spectrogram_shape(n), dtype=torch.float32, device=x.device)
    if "logmel" in want:
        out["logmel"] = torch.empty((N, mel_w.shape[0], 1 + n // 160, 2), dtype=torch.float32, device=x.device)
    if "gccphat" in want:
        out["gccphat"] = torch.empty((N, 2 * max_lag + 1, 1 + n // 160), dtype=torch.float32, device=x.device)
    audio_features_into(x, out.get("spectrogram"), out.get("logmel"), out.get("gccphat"), mel_start, mel_w, mel_eps, max_lag,
                        gcc_eps, pad_mode)
    return out


def audio_obs_into(spec, rir_bank, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int, out_len: int,
                   pad_mode="reflect", interleaved: bool = False, flags: int = 0) -> None:
    """Fused observation.  ``audiogoal`` may be None (the waveform then never leaves the CU).  Cross-faded rows longer
    than one partition block run as two launches when a buffer is given (faster), as one without."""
    _chk(spec, torch.float32, "spec"); _chk(rir_bank, torch.float32, "rir_bank"); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    us, cs, es, cap = _bank_strides(rir_bank, interleaved)
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_f32(spec.data_ptr(), rir_bank.data_ptr(), rir_len.data_ptr(),
                                                unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N, us, cs,
                                                es, cap, n_valid, out_len, _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_f32")


def audio_obs(spec, rir_bank, rir_len, unit_desc, n_valid: int, out_len: int, pad_mode="reflect",
              want_audiogoal: bool = False, interleaved: bool = False, flags: int = 0):
    N = unit_desc.shape[0]
    from .planning import wide_one_block
    need_ag = want_audiogoal or (out_len > KB and not wide_one_block(out_len, n_valid)
                                 and (bool(flags & FLAG_CROSSFADE) or out_len > 3 * KB))
    ag = torch.empty((N, 2, out_len), dtype=torch.float32, device=spec.device) if need_ag else None
    sg = torch.empty((N,) + spectrogram_shape(out_len), dtype=torch.float32, device=spec.device)
    audio_obs_into(spec, rir_bank, rir_len, unit_desc, ag, sg, n_valid, out_len, pad_mode, interleaved, flags)
    return ag, sg


# ---- spectral RIR bank ------------------------------------------------------------------------------------------
def _chk_spectra(hspec: torch.Tensor, hscale) -> bool:
    """the spectral bank argument of the *_spec_* ops: float32 [R,2,hb,SPEC_FLOATS], or - a HALF bank (include/ss_hip.h
    "Half-precision spectral bank") - float16 of the same shape with its float32 scales hscale [R,2,hb].  -> half?"""
    if hscale is None:
        _chk(hspec, torch.float32, "hspec")
        assert hspec.dim() == 4
        return False
    _chk(hspec, torch.float16, "hspec"); _chk(hscale, torch.float32, "hscale")
    assert hspec.dim() == 4 and hspec.shape[3] == SPEC_FLOATS and tuple(hscale.shape) == tuple(hspec.shape[:3])
    assert hscale.device == hspec.device
    return True


def rir_spectra_into(rir_bank: torch.Tensor, hspec: torch.Tensor, first: int = 0, count: Optional[int] = None) -> None:
    """Block spectra of bank entries [first, first+count) of a planar bank [R,2,cap] into hspec [R,2,hb,SPEC_FLOATS]
    (ss_rir_spectra_f32; one-off work at bank load, synchronous)."""
    _chk(rir_bank, torch.float32, "rir_bank"); _chk(hspec, torch.float32, "hspec")
    R, two, cap = rir_bank.shape
    hb = ceil_div(cap, KB)
    assert two == 2 and tuple(hspec.shape) == (R, 2, hb, SPEC_FLOATS)
    count = R - first if count is None else count
    assert 0 <= first and first + count <= R
    with torch.cuda.device(rir_bank.device):
        _lib.check(_lib.load().ss_rir_spectra_f32(rir_bank[first:].data_ptr(), hspec[first:].data_ptr(), count, 2 * cap, cap,
                                                  cap, _stream(rir_bank)), "ss_rir_spectra_f32")


def scatter_spectra_into(staged: torch.Tensor, planar: bool, slots: torch.Tensor, lens: torch.Tensor, n: int,
                         hspec: torch.Tensor, bank_len: torch.Tensor, hscale: Optional[torch.Tensor] = None) -> None:
    """Rows [0, n) of a staging block -> block spectra of entries slots[i] of the spectral-only bank hspec [R,2,hb,SPEC_FLOATS]
    and lens[i] into bank_len[slots[i]] (ss_bank_scatter_spectra_f32: one launch on the current stream of hspec's device).
    staged: float32 [*, cap, 2] (wav layout) or [*, 2, cap] (planar), pinned host or device memory; slots / lens: int32, pinned
    host or device memory.  The caller keeps all three alive and unchanged until the launch has run.
    hscale given: hspec is a HALF bank (float16) and hscale its scales (ss_bank_scatter_spectra16_f32)."""
    half = _chk_spectra(hspec, hscale); _chk(bank_len, torch.int32, "bank_len")
    for t, dt, name in ((staged, torch.float32, "staged"), (slots, torch.int32, "slots"), (lens, torch.int32, "lens")):
        if not (t.is_cuda or t.is_pinned()):
            raise ValueError(f"{name}: pinned host or device memory expected (the kernel reads it in place)")
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dt}, got {t.dtype} contiguous={t.is_contiguous()}")
    assert staged.dim() == 3 and staged.shape[2 if not planar else 1] == 2 and hspec.dim() == 4 and staged.shape[0] >= n
    if n == 0:
        return
    with torch.cuda.device(hspec.device):
        if half:
            _lib.check(_lib.load().ss_bank_scatter_spectra16_f32(staged.data_ptr(), staged[0].numel(), int(bool(planar)),
                                                                 slots.data_ptr(), lens.data_ptr(), n, hspec.data_ptr(),
                                                                 hscale.data_ptr(), hspec.shape[2], bank_len.data_ptr(),
                                                                 _stream(hspec)), "ss_bank_scatter_spectra16_f32")
            return
        _lib.check(_lib.load().ss_bank_scatter_spectra_f32(staged.data_ptr(), staged[0].numel(), int(bool(planar)), slots.data_ptr(),
                                                           lens.data_ptr(), n, hspec.data_ptr(), hspec.shape[2], bank_len.data_ptr(),
                                                           _stream(hspec)), "ss_bank_scatter_spectra_f32")


def rir_spectra(rir_bank: torch.Tensor) -> torch.Tensor:
    R, _, cap = rir_bank.shape
    hspec = torch.empty((R, 2, ceil_div(cap, KB), SPEC_FLOATS), dtype=torch.float32, device=rir_bank.device)
    rir_spectra_into(rir_bank, hspec)
    return hspec


def rir_spectra16(rir_bank: torch.Tensor):
    """Half form of a planar bank [R,2,cap] (ss_rir_spectra16_f32, on the current stream) -> (float16 [R,2,hb,SPEC_FLOATS],
    float32 scales [R,2,hb]): q = fp16(H' * 2^(15-e)) rounded to nearest even, scale = 2^(e-15), per block (include/ss_hip.h)."""
    _chk(rir_bank, torch.float32, "rir_bank")
    R, two, cap = rir_bank.shape
    assert two == 2
    hb = ceil_div(cap, KB)
    hspec16 = torch.zeros((R, 2, hb, SPEC_FLOATS), dtype=torch.float16, device=rir_bank.device)
    hscale = torch.zeros((R, 2, hb), dtype=torch.float32, device=rir_bank.device)
    if R:
        with torch.cuda.device(rir_bank.device):
            _lib.check(_lib.load().ss_rir_spectra16_f32(rir_bank.data_ptr(), hspec16.data_ptr(), hscale.data_ptr(), R, 2 * cap, cap,
                                                        cap, _stream(rir_bank)), "ss_rir_spectra16_f32")
    return hspec16, hscale


def fftconv_binaural_spec_into(spec, hspec, rir_len, unit_desc, out, n_valid: int, flags: int = 0, hscale=None) -> None:
    """hscale given: hspec is a HALF bank (ss_fftconv_binaural_spec16_f32)."""
    _chk(spec, torch.float32, "spec"); half = _chk_spectra(hspec, hscale); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(out, torch.float32, "out")
    N, two, out_len = out.shape
    assert two == 2 and unit_desc.shape == (N, 8) and hspec.dim() == 4
    with torch.cuda.device(out.device):
        if half:
            _lib.check(_lib.load().ss_fftconv_binaural_spec16_f32(spec.data_ptr(), hspec.data_ptr(), hscale.data_ptr(),
                                                                  rir_len.data_ptr(), unit_desc.data_ptr(), out.data_ptr(), N,
                                                                  hspec.shape[2], n_valid, out_len, flags, _stream(spec)),
                       "ss_fftconv_binaural_spec16_f32")
            return
        _lib.check(_lib.load().ss_fftconv_binaural_spec_f32(spec.data_ptr(), hspec.data_ptr(), rir_len.data_ptr(),
                                                            unit_desc.data_ptr(), out.data_ptr(), N, hspec.shape[2],
                                                            n_valid, out_len, flags, _stream(spec)),
                   "ss_fftconv_binaural_spec_f32")


def audio_obs_spec_into(spec, hspec, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int, out_len: int,
                        pad_mode="reflect", flags: int = 0, hscale=None) -> None:
    """hscale given: hspec is a HALF bank (ss_audio_obs_spec16_f32: rows of one partition block; ss_audio_obs_rows_spec16_f32:
    rows of 2 or 3, KB < out_len <= 3 KB)."""
    _chk(spec, torch.float32, "spec"); half = _chk_spectra(hspec, hscale); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len) and hspec.dim() == 4
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        if half:
            name = "ss_audio_obs_rows_spec16_f32" if out_len > KB else "ss_audio_obs_spec16_f32"
            _lib.check(getattr(_lib.load(), name)(spec.data_ptr(), hspec.data_ptr(), hscale.data_ptr(), rir_len.data_ptr(),
                                                  unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N, hspec.shape[2],
                                                  n_valid, out_len, _PAD[pad_mode], flags, _stream(spec)), name)
            return
        _lib.check(_lib.load().ss_audio_obs_spec_f32(spec.data_ptr(), hspec.data_ptr(), rir_len.data_ptr(),
                                                     unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N,
                                                     hspec.shape[2], n_valid, out_len, _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_spec_f32")


# ---- half-precision time-domain rows ------------------------------------------------------------------------------
def _chk_rows16(rir16: torch.Tensor, rscale: torch.Tensor) -> int:
    """the bank argument of the *_rir16_* ops (include/ss_hip.h "Half-precision time-domain rows"): float16 [R,2,cap] with its
    float32 scales [R,2].  -> cap"""
    _chk(rir16, torch.float16, "rir16"); _chk(rscale, torch.float32, "rscale")
    assert rir16.dim() == 3 and rir16.shape[1] == 2 and tuple(rscale.shape) == tuple(rir16.shape[:2])
    assert rscale.device == rir16.device
    return int(rir16.shape[2])


def rir_rows16(rir_bank: torch.Tensor):
    """Half form of a planar bank [R,2,cap] (``ss_rir_rows16_f32``, on the current stream) -> (float16 [R,2,cap], float32 scales
    [R,2]): per (entry, ear) row q = fp16(v * 2^(15-e)) rounded to nearest even, scale = 2^(e-15).  Opt-in and LOSSY: the waveform
    moves by about 2e-4 of its peak (include/ss_hip.h)."""
    _chk(rir_bank, torch.float32, "rir_bank")
    R, two, cap = rir_bank.shape
    assert two == 2
    rir16 = torch.zeros((R, 2, cap), dtype=torch.float16, device=rir_bank.device)
    rscale = torch.zeros((R, 2), dtype=torch.float32, device=rir_bank.device)
    if R:
        with torch.cuda.device(rir_bank.device):
            _lib.check(_lib.load().ss_rir_rows16_f32(rir_bank.data_ptr(), rir16.data_ptr(), rscale.data_ptr(), R, 2 * cap, cap, cap,
                                                     _stream(rir_bank)), "ss_rir_rows16_f32")
    return rir16, rscale


def scatter_rows16_into(staged: torch.Tensor, slots: torch.Tensor, lens: torch.Tensor, n: int, rir16: torch.Tensor,
                        rscale: torch.Tensor, bank_len: torch.Tensor) -> None:
    """Rows [0, n) of a wav-layout staging block (float32 [*, >= cap, 2], pinned host or device memory) -> halves + scales of
    entries slots[i] of the half-rows bank (rir16 [R,2,cap], rscale [R,2]) and lens[i] into bank_len[slots[i]]
    (``ss_bank_scatter_rows16_f32``: one launch on the current stream of the bank's device).  slots / lens: int32, pinned host
    or device memory.  The caller keeps all three alive and unchanged until the launch has run."""
    cap = _chk_rows16(rir16, rscale); _chk(bank_len, torch.int32, "bank_len")
    for t, dt, name in ((staged, torch.float32, "staged"), (slots, torch.int32, "slots"), (lens, torch.int32, "lens")):
        if not (t.is_cuda or t.is_pinned()):
            raise ValueError(f"{name}: pinned host or device memory expected (the kernel reads it in place)")
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dt}, got {t.dtype} contiguous={t.is_contiguous()}")
    assert staged.dim() == 3 and staged.shape[2] == 2 and staged.shape[1] >= cap and staged.shape[0] >= n
    if n == 0:
        return
    with torch.cuda.device(rir16.device):
        _lib.check(_lib.load().ss_bank_scatter_rows16_f32(staged.data_ptr(), staged[0].numel(), slots.data_ptr(), lens.data_ptr(), n,
                                                          rir16.data_ptr(), rscale.data_ptr(), cap, bank_len.data_ptr(),
                                                          _stream(rir16)), "ss_bank_scatter_rows16_f32")


def scatter_rows16_max_into(staged: torch.Tensor, slots: torch.Tensor, lens: torch.Tensor, row_max: torch.Tensor, n: int,
                            rir16: torch.Tensor, rscale: torch.Tensor, bank_len: torch.Tensor) -> None:
    """``scatter_rows16_into`` in one pass over each row, the rows' maxima given (``ss_bank_scatter_rows16_max_f32``,
    k_scatter_rows16_max): row_max float32 [*, 2], pinned host or device memory, row_max[i, c] = max |v| over ear c of the frames
    of row i in front of its (clamped) length, 0 for an empty row - what ``ss_wav_read_rirs_max_f32`` reports.  Same bits as
    ``scatter_rows16_into`` on the same samples."""
    cap = _chk_rows16(rir16, rscale); _chk(bank_len, torch.int32, "bank_len")
    for t, dt, name in ((staged, torch.float32, "staged"), (slots, torch.int32, "slots"), (lens, torch.int32, "lens"),
                        (row_max, torch.float32, "row_max")):
        if not (t.is_cuda or t.is_pinned()):
            raise ValueError(f"{name}: pinned host or device memory expected (the kernel reads it in place)")
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dt}, got {t.dtype} contiguous={t.is_contiguous()}")
    assert staged.dim() == 3 and staged.shape[2] == 2 and staged.shape[1] >= cap and staged.shape[0] >= n
    assert row_max.dim() == 2 and row_max.shape[1] == 2 and row_max.shape[0] >= n
    if n == 0:
        return
    with torch.cuda.device(rir16.device):
        _lib.check(_lib.load().ss_bank_scatter_rows16_max_f32(staged.data_ptr(), staged[0].numel(), slots.data_ptr(), lens.data_ptr(),
                                                              row_max.data_ptr(), n, rir16.data_ptr(), rscale.data_ptr(), cap,
                                                              bank_len.data_ptr(), _stream(rir16)), "ss_bank_scatter_rows16_max_f32")


def fftconv_binaural_rir16_into(spec, rir16, rscale, rir_len, unit_desc, out, n_valid: int, flags: int = 0) -> None:
    """``fftconv_binaural_into`` from a bank of half rows (``ss_fftconv_binaural_rir16_f32``); no cross-fade."""
    _chk(spec, torch.float32, "spec"); cap = _chk_rows16(rir16, rscale); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(out, torch.float32, "out")
    N, two, out_len = out.shape
    assert two == 2 and unit_desc.shape == (N, 8)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().ss_fftconv_binaural_rir16_f32(spec.data_ptr(), rir16.data_ptr(), rscale.data_ptr(), rir_len.data_ptr(),
                                                             unit_desc.data_ptr(), out.data_ptr(), N, cap, n_valid, out_len, flags,
                                                             _stream(spec)), "ss_fftconv_binaural_rir16_f32")


def audio_obs_rir16_into(spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int, out_len: int,
                         pad_mode="reflect", flags: int = 0) -> None:
    """The fused observation of one-block rows (257 <= out_len <= KB) from a bank of half rows (``ss_audio_obs_rir16_f32``);
    ``audiogoal`` may be None."""
    _chk(spec, torch.float32, "spec"); cap = _chk_rows16(rir16, rscale); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_rir16_f32(spec.data_ptr(), rir16.data_ptr(), rscale.data_ptr(), rir_len.data_ptr(),
                                                      unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N, cap, n_valid,
                                                      out_len, _PAD[pad_mode], flags, _stream(spec)), "ss_audio_obs_rir16_f32")


def audio_obs_rows_rir16_into(spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int, out_len: int,
                              pad_mode="reflect", flags: int = 0) -> None:
    """The fused observation of rows of 2 or 3 partition blocks (KB < out_len <= 3 KB: 44.1 / 48 kHz) from a bank of half rows
    (``ss_audio_obs_rows_rir16_f32``: k_obs_blocks for small steps, k_obs_rows beyond); ``audiogoal`` may be None - except with
    n_valid <= KB, which the library serves in two launches when it is given one and in one when it is not.  Captured into a
    graph: ``ss_amd.graphs.capture`` (include/ss_hip.h "Captured steps")."""
    _chk(spec, torch.float32, "spec"); cap = _chk_rows16(rir16, rscale); _chk(rir_len, torch.int32, "rir_len")
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_rows_rir16_f32(spec.data_ptr(), rir16.data_ptr(), rscale.data_ptr(), rir_len.data_ptr(),
                                                           unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N, cap, n_valid,
                                                           out_len, _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_rows_rir16_f32")


def _obs_logmel_rir16(entry: str, spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                      n_valid, out_len, mel_eps, pad_mode, flags) -> None:
    _chk(spec, torch.float32, "spec"); cap = _chk_rows16(rir16, rscale); _chk(rir_len, torch.int32, "rir_len")
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    with torch.cuda.device(spec.device):
        _lib.check(getattr(_lib.load(), entry)(spec.data_ptr(), rir16.data_ptr(), rscale.data_ptr(), rir_len.data_ptr(),
                                               unit_desc.data_ptr(), ag_ptr, sg_ptr, logmel_out.data_ptr(), mel_start.data_ptr(),
                                               mel_w.data_ptr(), int(n_mels), int(max_len), float(mel_eps), N, cap, n_valid, out_len,
                                               _PAD[pad_mode], flags, _stream(spec)), entry)


def audio_obs_logmel_rir16_into(spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                                n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect", flags: int = 0) -> None:
    """``audio_obs_logmel_into`` from a bank of half rows (``ss_audio_obs_logmel_rir16_f32``): ONE launch, whichever outputs are
    asked for next to ``logmel_out``.  Rows of one partition block (257 <= out_len <= KB), no cross-fade; anything else is
    refused (invalid argument)."""
    _obs_logmel_rir16("ss_audio_obs_logmel_rir16_f32", spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out,
                      logmel_out, mel_start, mel_w, n_valid, out_len, mel_eps, pad_mode, flags)


def audio_obs_logmel_rows_rir16_into(spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start,
                                     mel_w, n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect",
                                     flags: int = 0) -> None:
    """``audio_obs_logmel_rows_into`` from a bank of half rows (``ss_audio_obs_logmel_rows_rir16_f32``): rows of 2 or 3 partition
    blocks (KB < out_len <= 3 KB), at most 16 RIR blocks, no cross-fade.  Small steps run the one-workgroup-per-output-block
    kernel; captured into a graph: ``ss_amd.graphs.capture``."""
    _obs_logmel_rir16("ss_audio_obs_logmel_rows_rir16_f32", spec, rir16, rscale, rir_len, unit_desc, audiogoal, spectrogram_out,
                      logmel_out, mel_start, mel_w, n_valid, out_len, mel_eps, pad_mode, flags)


# ---- log-mel observation in one launch (no waveform buffer) ---------------------------------------------------------
def _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len):
    _chk(unit_desc, torch.int32, "unit_desc"); _chk(logmel_out, torch.float32, "logmel_out")
    _chk(mel_start, torch.int32, "mel_start"); _chk(mel_w, torch.float32, "mel_w")
    N = unit_desc.shape[0]
    n_mels, max_len = mel_w.shape
    assert mel_start.shape == (n_mels,) and tuple(logmel_out.shape) == (N, n_mels, 1 + out_len // 160, 2)
    ag_ptr = sg_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    if spectrogram_out is not None:
        _chk(spectrogram_out, torch.float32, "spectrogram_out")
        assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
        sg_ptr = spectrogram_out.data_ptr()
    return N, n_mels, max_len, ag_ptr, sg_ptr


def audio_obs_logmel_into(spec, rir_bank, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                          n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect", interleaved: bool = False,
                          flags: int = 0) -> None:
    """EXTENSION: log-mel observation in ONE launch (``ss_audio_obs_logmel_f32``): convolution -> framing -> window -> rFFT ->
    |.|^2 -> mel bands -> log on the row a workgroup holds in LDS; the waveform needs no buffer.  ``audiogoal`` and
    ``spectrogram_out`` may each be None.  Rows of one partition block (257 <= out_len <= KB) without a cross-fade only; mel
    arguments as ``audio_features_into``; anything else is refused (invalid argument)."""
    _chk(spec, torch.float32, "spec"); _chk(rir_bank, torch.float32, "rir_bank"); _chk(rir_len, torch.int32, "rir_len")
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    us, cs, es, cap = _bank_strides(rir_bank, interleaved)
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_logmel_f32(spec.data_ptr(), rir_bank.data_ptr(), rir_len.data_ptr(), unit_desc.data_ptr(),
                                                       ag_ptr, sg_ptr, logmel_out.data_ptr(), mel_start.data_ptr(), mel_w.data_ptr(),
                                                       int(n_mels), int(max_len), float(mel_eps), N, us, cs, es, cap, n_valid,
                                                       out_len, _PAD[pad_mode], flags, _stream(spec)), "ss_audio_obs_logmel_f32")


def audio_obs_logmel_spec_into(spec, hspec, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                               n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect", flags: int = 0,
                               hscale=None) -> None:
    """``audio_obs_logmel_into`` from the spectral RIR bank (``ss_audio_obs_logmel_spec_f32``); hscale given: from a HALF bank
    (``ss_audio_obs_logmel_spec16_f32``)."""
    _chk(spec, torch.float32, "spec"); half = _chk_spectra(hspec, hscale); _chk(rir_len, torch.int32, "rir_len")
    assert hspec.dim() == 4
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    with torch.cuda.device(spec.device):
        if half:
            _lib.check(_lib.load().ss_audio_obs_logmel_spec16_f32(spec.data_ptr(), hspec.data_ptr(), hscale.data_ptr(),
                                                                  rir_len.data_ptr(), unit_desc.data_ptr(), ag_ptr, sg_ptr,
                                                                  logmel_out.data_ptr(), mel_start.data_ptr(), mel_w.data_ptr(),
                                                                  int(n_mels), int(max_len), float(mel_eps), N, hspec.shape[2], n_valid,
                                                                  out_len, _PAD[pad_mode], flags, _stream(spec)),
                       "ss_audio_obs_logmel_spec16_f32")
            return
        _lib.check(_lib.load().ss_audio_obs_logmel_spec_f32(spec.data_ptr(), hspec.data_ptr(), rir_len.data_ptr(), unit_desc.data_ptr(),
                                                            ag_ptr, sg_ptr, logmel_out.data_ptr(), mel_start.data_ptr(),
                                                            mel_w.data_ptr(), int(n_mels), int(max_len), float(mel_eps), N,
                                                            hspec.shape[2], n_valid, out_len, _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_logmel_spec_f32")


def audio_obs_logmel_rows_into(spec, rir_bank, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                               n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect", interleaved: bool = False,
                               flags: int = 0) -> None:
    """``audio_obs_logmel_into`` for rows of 2 or 3 partition blocks (KB < out_len <= 3 KB: 44.1 / 48 kHz;
    ``ss_audio_obs_logmel_rows_f32``): ONE launch of the log-mel form of the fused row kernels, whichever outputs are asked for
    next to ``logmel_out``.  No cross-fade, at most 16 RIR blocks; anything else is refused (invalid argument).  Small steps run
    the one-workgroup-per-output-block kernel; captured into a graph: ``ss_amd.graphs.capture``."""
    _chk(spec, torch.float32, "spec"); _chk(rir_bank, torch.float32, "rir_bank"); _chk(rir_len, torch.int32, "rir_len")
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    us, cs, es, cap = _bank_strides(rir_bank, interleaved)
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_logmel_rows_f32(spec.data_ptr(), rir_bank.data_ptr(), rir_len.data_ptr(),
                                                            unit_desc.data_ptr(), ag_ptr, sg_ptr, logmel_out.data_ptr(),
                                                            mel_start.data_ptr(), mel_w.data_ptr(), int(n_mels), int(max_len),
                                                            float(mel_eps), N, us, cs, es, cap, n_valid, out_len, _PAD[pad_mode],
                                                            flags, _stream(spec)), "ss_audio_obs_logmel_rows_f32")


def audio_obs_logmel_ss2_into(spec, rir_bank, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                              n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect", interleaved: bool = False,
                              flags: int = 0) -> None:
    """``audio_obs_logmel_into`` for SoundSpaces 2.0 steps (``ss_audio_obs_logmel_ss2_f32``; time-domain bank only): ONE launch,
    whichever outputs are asked for next to ``logmel_out``.  Serves cross-faded rows of one partition block (257 <= out_len <=
    KB with ``FLAG_CROSSFADE``) and rows of 2 or 3 blocks of which only block 0 is rendered (KB < out_len <= 3 KB, n_valid <= KB
    and at most 26 live pooled blocks: 0.25 s of a 44.1 / 48 kHz row), cross-faded or not; anything else is refused (invalid
    argument)."""
    _chk(spec, torch.float32, "spec"); _chk(rir_bank, torch.float32, "rir_bank"); _chk(rir_len, torch.int32, "rir_len")
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    us, cs, es, cap = _bank_strides(rir_bank, interleaved)
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_logmel_ss2_f32(spec.data_ptr(), rir_bank.data_ptr(), rir_len.data_ptr(),
                                                           unit_desc.data_ptr(), ag_ptr, sg_ptr, logmel_out.data_ptr(),
                                                           mel_start.data_ptr(), mel_w.data_ptr(), int(n_mels), int(max_len),
                                                           float(mel_eps), N, us, cs, es, cap, n_valid, out_len, _PAD[pad_mode],
                                                           flags, _stream(spec)), "ss_audio_obs_logmel_ss2_f32")


def audio_obs_logmel_rows_spec_into(spec, hspec, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w,
                                    n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect", flags: int = 0,
                                    hscale=None) -> None:
    """``audio_obs_logmel_rows_into`` from the spectral RIR bank (``ss_audio_obs_logmel_rows_spec_f32``); hscale given: from a
    HALF bank (``ss_audio_obs_logmel_rows_spec16_f32``)."""
    _chk(spec, torch.float32, "spec"); half = _chk_spectra(hspec, hscale); _chk(rir_len, torch.int32, "rir_len")
    assert hspec.dim() == 4
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    with torch.cuda.device(spec.device):
        if half:
            _lib.check(_lib.load().ss_audio_obs_logmel_rows_spec16_f32(spec.data_ptr(), hspec.data_ptr(), hscale.data_ptr(),
                                                                       rir_len.data_ptr(), unit_desc.data_ptr(), ag_ptr, sg_ptr,
                                                                       logmel_out.data_ptr(), mel_start.data_ptr(), mel_w.data_ptr(),
                                                                       int(n_mels), int(max_len), float(mel_eps), N, hspec.shape[2],
                                                                       n_valid, out_len, _PAD[pad_mode], flags, _stream(spec)),
                       "ss_audio_obs_logmel_rows_spec16_f32")
            return
        _lib.check(_lib.load().ss_audio_obs_logmel_rows_spec_f32(spec.data_ptr(), hspec.data_ptr(), rir_len.data_ptr(),
                                                                 unit_desc.data_ptr(), ag_ptr, sg_ptr, logmel_out.data_ptr(),
                                                                 mel_start.data_ptr(), mel_w.data_ptr(), int(n_mels), int(max_len),
                                                                 float(mel_eps), N, hspec.shape[2], n_valid, out_len,
                                                                 _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_logmel_rows_spec_f32")


# ---- length-bucketed RIR bank ------------------------------------------------------------------------
def bucket_array(banks, firsts, spectral: bool):
    """ctypes array of ss_rir_bucket for per-bucket (data [n,2,cap], spectra or None) tensors; keep it alive with the
    tensors it points to."""
    arr = (_lib.SsRirBucket * len(banks))()
    for b, (bank, first) in enumerate(zip(banks, firsts)):
        _chk(bank.data, torch.float32, "bucket data")
        arr[b].rir = bank.data.data_ptr()
        arr[b].hspec = bank.spectra.data_ptr() if (spectral and bank.spectra is not None) else None
        arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = int(first), int(bank.data.shape[0]), int(bank.data.shape[2]), 0
    return arr


def audio_obs_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int,
                           out_len: int, pad_mode="reflect", flags: int = 0) -> None:
    """``audio_obs_into`` on a length-bucketed bank: ``buckets`` = ``bucket_array(...)``, rir_len int32 [total slots]."""
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len"); _chk(unit_desc, torch.int32, "unit_desc")
    N = unit_desc.shape[0]
    ag_ptr = sg_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        if spectrogram_out is None:
            _lib.check(_lib.load().ss_fftconv_binaural_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets,
                                                                   rir_len.data_ptr(), unit_desc.data_ptr(), ag_ptr, N, n_valid,
                                                                   out_len, flags, _stream(spec)), "ss_fftconv_binaural_buckets_f32")
            return
        _chk(spectrogram_out, torch.float32, "spectrogram_out")
        assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
        sg_ptr = spectrogram_out.data_ptr()
        _lib.check(_lib.load().ss_audio_obs_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets, rir_len.data_ptr(),
                                                        unit_desc.data_ptr(), ag_ptr, sg_ptr, N, n_valid, out_len,
                                                        _PAD[pad_mode], flags, _stream(spec)), "ss_audio_obs_buckets_f32")


# ---- half-precision time-domain rows in length buckets (include/ss_hip.h "... in length buckets") ---------------------------
def rir16_bucket_array(rows16, scales, firsts):
    """ctypes array of ss_rir16_bucket: per bucket its half rows [n,2,cap] (float16), its scales [n,2] (float32) and the global
    index of its entry 0.  Keep the array alive with the tensors it points to."""
    assert len(rows16) == len(scales) == len(firsts)
    arr = (_lib.SsRir16Bucket * len(rows16))()
    for b, (q, sc, first) in enumerate(zip(rows16, scales, firsts)):
        cap = _chk_rows16(q, sc)
        arr[b].rir16 = q.data_ptr()
        arr[b].rscale = sc.data_ptr()
        arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = int(first), int(q.shape[0]), cap, 0
    return arr


def fftconv_binaural_rir16_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, out, n_valid: int, flags: int = 0) -> None:
    """``fftconv_binaural_rir16_into`` on half rows in length buckets: ``buckets`` = ``rir16_bucket_array(...)``
    (ss_fftconv_binaural_rir16_buckets_f32); no cross-fade."""
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len"); _chk(unit_desc, torch.int32, "unit_desc")
    _chk(out, torch.float32, "out")
    N, two, out_len = out.shape
    assert two == 2 and unit_desc.shape == (N, 8)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().ss_fftconv_binaural_rir16_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets,
                                                                     rir_len.data_ptr(), unit_desc.data_ptr(), out.data_ptr(), N,
                                                                     n_valid, out_len, flags, _stream(spec)),
                   "ss_fftconv_binaural_rir16_buckets_f32")


def audio_obs_rir16_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int,
                                 out_len: int, pad_mode="reflect", flags: int = 0) -> None:
    """``audio_obs_rir16_into`` on half rows in length buckets (ss_audio_obs_rir16_buckets_f32: one-block rows, 257 <= out_len <=
    KB; ``audiogoal`` may be None).  spectrogram_out None: the waveform alone (ss_fftconv_binaural_rir16_buckets_f32)."""
    if spectrogram_out is None:
        fftconv_binaural_rir16_buckets_into(spec, buckets, n_buckets, rir_len, unit_desc, audiogoal, n_valid, flags)
        return
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len"); _chk(unit_desc, torch.int32, "unit_desc")
    _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_rir16_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets, rir_len.data_ptr(),
                                                              unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N, n_valid,
                                                              out_len, _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_rir16_buckets_f32")


# ---- spectral length buckets: a bucketed bank without time-domain rows (include/ss_hip.h "Spectral length buckets") --------
def spec_bucket_array(spectra, scales, firsts, caps):
    """ctypes array of ss_spec_bucket: per bucket its block spectra [n,2,hb,SPEC_FLOATS] (float32, or float16 of a HALF bank),
    its scales [n,2,hb] (half) or None (fp32), the global index of its entry 0 and its row capacity in samples.  One form in
    every bucket.  Keep the array alive with the tensors it points to."""
    scales = [None] * len(spectra) if scales is None else list(scales)
    assert len(spectra) == len(scales) == len(firsts) == len(caps)
    half = bool(scales) and scales[0] is not None
    arr = (_lib.SsSpecBucket * len(spectra))()
    for b, (hs, sc, first, cap) in enumerate(zip(spectra, scales, firsts, caps)):
        if (sc is not None) != half:
            raise ValueError("spec_bucket_array: every bucket carries scales (half) or none does (fp32)")
        _chk_spectra(hs, sc)
        assert hs.shape[1] == 2 and hs.shape[2] == ceil_div(int(cap), KB) and hs.shape[3] == SPEC_FLOATS
        arr[b].hspec = hs.data_ptr()
        arr[b].hscale = sc.data_ptr() if half else None
        arr[b].first, arr[b].n_entries, arr[b].cap, arr[b].reserved = int(first), int(hs.shape[0]), int(cap), 0
    return arr


def fftconv_binaural_spec_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, out, n_valid: int, flags: int = 0) -> None:
    """``fftconv_binaural_spec_into`` on spectral length buckets: ``buckets`` = ``spec_bucket_array(...)``
    (ss_fftconv_binaural_spec_buckets_f32)."""
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len"); _chk(unit_desc, torch.int32, "unit_desc")
    _chk(out, torch.float32, "out")
    N, two, out_len = out.shape
    assert two == 2 and unit_desc.shape == (N, 8)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().ss_fftconv_binaural_spec_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets,
                                                                    rir_len.data_ptr(), unit_desc.data_ptr(), out.data_ptr(), N,
                                                                    n_valid, out_len, flags, _stream(spec)),
                   "ss_fftconv_binaural_spec_buckets_f32")


def audio_obs_spec_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int,
                                out_len: int, pad_mode="reflect", flags: int = 0) -> None:
    """``audio_obs_spec_into`` on spectral length buckets (ss_audio_obs_spec_buckets_f32; spectrogram_out None: the waveform
    alone, ss_fftconv_binaural_spec_buckets_f32).  A half bank serves rows of one partition block here."""
    if spectrogram_out is None:
        fftconv_binaural_spec_buckets_into(spec, buckets, n_buckets, rir_len, unit_desc, audiogoal, n_valid, flags)
        return
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len"); _chk(unit_desc, torch.int32, "unit_desc")
    _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_spec_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets, rir_len.data_ptr(),
                                                             unit_desc.data_ptr(), ag_ptr, spectrogram_out.data_ptr(), N, n_valid,
                                                             out_len, _PAD[pad_mode], flags, _stream(spec)),
                   "ss_audio_obs_spec_buckets_f32")


def audio_obs_rows_spec16_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, n_valid: int,
                                       out_len: int, pad_mode="reflect", flags: int = 0) -> None:
    """``audio_obs_spec_buckets_into`` for rows of 2 or 3 partition blocks (KB < out_len <= 3 KB: 44.1 / 48 kHz) on HALF spectral
    length buckets (``ss_audio_obs_rows_spec16_buckets_f32``; ``buckets`` = ``spec_bucket_array(...)`` of a half bank).
    ``audiogoal`` may be None; spectrogram_out None: the waveform alone (ss_fftconv_binaural_spec_buckets_f32)."""
    if spectrogram_out is None:
        fftconv_binaural_spec_buckets_into(spec, buckets, n_buckets, rir_len, unit_desc, audiogoal, n_valid, flags)
        return
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len"); _chk(unit_desc, torch.int32, "unit_desc")
    _chk(spectrogram_out, torch.float32, "spectrogram_out")
    N = unit_desc.shape[0]
    assert tuple(spectrogram_out.shape) == (N,) + spectrogram_shape(out_len)
    ag_ptr = None
    if audiogoal is not None:
        _chk(audiogoal, torch.float32, "audiogoal")
        assert tuple(audiogoal.shape) == (N, 2, out_len)
        ag_ptr = audiogoal.data_ptr()
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().ss_audio_obs_rows_spec16_buckets_f32(spec.data_ptr(), ctypes_ref(buckets), n_buckets,
                                                                    rir_len.data_ptr(), unit_desc.data_ptr(), ag_ptr,
                                                                    spectrogram_out.data_ptr(), N, n_valid, out_len, _PAD[pad_mode],
                                                                    flags, _stream(spec)),
                   "ss_audio_obs_rows_spec16_buckets_f32")


def _obs_logmel_buckets(entry: str, spec, buckets, n_buckets, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start,
                        mel_w, n_valid, out_len, mel_eps, pad_mode, flags) -> None:
    _chk(spec, torch.float32, "spec"); _chk(rir_len, torch.int32, "rir_len")
    N, n_mels, max_len, ag_ptr, sg_ptr = _obs_logmel_args(unit_desc, audiogoal, spectrogram_out, logmel_out, mel_start, mel_w, out_len)
    with torch.cuda.device(spec.device):
        _lib.check(getattr(_lib.load(), entry)(spec.data_ptr(), ctypes_ref(buckets), n_buckets, rir_len.data_ptr(),
                                               unit_desc.data_ptr(), ag_ptr, sg_ptr, logmel_out.data_ptr(), mel_start.data_ptr(),
                                               mel_w.data_ptr(), int(n_mels), int(max_len), float(mel_eps), N, n_valid, out_len,
                                               _PAD[pad_mode], flags, _stream(spec)), entry)


def audio_obs_logmel_rir16_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out,
                                        mel_start, mel_w, n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect",
                                        flags: int = 0) -> None:
    """``audio_obs_logmel_rir16_into`` on half rows in length buckets (``ss_audio_obs_logmel_rir16_buckets_f32``; ``buckets`` =
    ``rir16_bucket_array(...)``): rows of one partition block only."""
    _obs_logmel_buckets("ss_audio_obs_logmel_rir16_buckets_f32", spec, buckets, n_buckets, rir_len, unit_desc, audiogoal,
                        spectrogram_out, logmel_out, mel_start, mel_w, n_valid, out_len, mel_eps, pad_mode, flags)


def audio_obs_logmel_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out,
                                  mel_start, mel_w, n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect",
                                  flags: int = 0) -> None:
    """``audio_obs_logmel_into`` / ``audio_obs_logmel_rows_into`` on a length-bucketed bank (``ss_audio_obs_logmel_buckets_f32``;
    ``buckets`` = ``bucket_array(...)``): ONE launch, whichever outputs are asked for next to ``logmel_out``.  Rows of one
    partition block, and of 2 or 3 blocks with at most 16 RIR blocks in the deepest bucket; no cross-fade."""
    _obs_logmel_buckets("ss_audio_obs_logmel_buckets_f32", spec, buckets, n_buckets, rir_len, unit_desc, audiogoal, spectrogram_out,
                        logmel_out, mel_start, mel_w, n_valid, out_len, mel_eps, pad_mode, flags)


def audio_obs_logmel_spec_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out, logmel_out,
                                       mel_start, mel_w, n_valid: int, out_len: int, mel_eps: float = 1e-6, pad_mode="reflect",
                                       flags: int = 0) -> None:
    """``audio_obs_logmel_buckets_into`` on spectral length buckets (``ss_audio_obs_logmel_spec_buckets_f32``; ``buckets`` =
    ``spec_bucket_array(...)``).  A half bank serves rows of one partition block here."""
    _obs_logmel_buckets("ss_audio_obs_logmel_spec_buckets_f32", spec, buckets, n_buckets, rir_len, unit_desc, audiogoal,
                        spectrogram_out, logmel_out, mel_start, mel_w, n_valid, out_len, mel_eps, pad_mode, flags)


def audio_obs_logmel_rows_spec16_buckets_into(spec, buckets, n_buckets: int, rir_len, unit_desc, audiogoal, spectrogram_out,
                                              logmel_out, mel_start, mel_w, n_valid: int, out_len: int, mel_eps: float = 1e-6,
                                              pad_mode="reflect", flags: int = 0) -> None:
    """``audio_obs_logmel_spec_buckets_into`` for rows of 2 or 3 partition blocks on HALF spectral length buckets
    (``ss_audio_obs_logmel_rows_spec16_buckets_f32``): ONE launch, whichever outputs are asked for next to ``logmel_out``."""
    _obs_logmel_buckets("ss_audio_obs_logmel_rows_spec16_buckets_f32", spec, buckets, n_buckets, rir_len, unit_desc, audiogoal,
                        spectrogram_out, logmel_out, mel_start, mel_w, n_valid, out_len, mel_eps, pad_mode, flags)


def memo_rows_(pairs, moves: torch.Tensor, n_store: int, n_fetch: int) -> None:
    """The row copies of a pose memo in ONE launch (ss_memo_rows_f32, k_memo_rows) on the current stream: ``pairs`` = up to 4
    (out, pool) pairs of contiguous float32 CUDA tensors with equal row shapes; ``moves`` int32 [n_store + n_fetch, 2] =
    (row, slot), device or pinned host memory, read in place (keep it alive and unchanged until the launch has run).  The first
    n_store moves store out[row] into pool[slot], the following n_fetch fetch pool[slot] into out[row]; rows are distinct and
    slots are distinct over the whole list.  In place; nothing is returned (like the ``*_into`` entry points, not a registered op)."""
    pairs = list(pairs)
    if not 1 <= len(pairs) <= 4:
        raise ValueError("memo_rows_: 1 to 4 (out, pool) pairs")
    io = (_lib.SsMemoIo * len(pairs))()
    dev = None
    for k, (out, pool) in enumerate(pairs):
        _chk(out, torch.float32, "out"); _chk(pool, torch.float32, "pool")
        if tuple(out.shape[1:]) != tuple(pool.shape[1:]) or out.dim() < 2 or out.device != pool.device:
            raise ValueError("memo_rows_: out and pool must be [rows, ...] tensors with equal row shapes on one device")
        if dev is not None and out.device != dev:
            raise ValueError("memo_rows_: all arrays must live on one device")
        dev = out.device
        io[k] = _lib.SsMemoIo(out.data_ptr(), pool.data_ptr(), out[0].numel(), 0)
    if not (moves.is_cuda or moves.is_pinned()):
        raise ValueError("moves: pinned host or device memory expected (the kernel reads it in place)")
    if moves.dtype != torch.int32 or not moves.is_contiguous() or moves.dim() != 2 or moves.shape[1] != 2 or \
            moves.shape[0] < n_store + n_fetch:
        raise ValueError("moves: contiguous int32 [n_store + n_fetch, 2] expected")
    if n_store + n_fetch > 0:                              # (rows / slots inside the arrays: a wrong index is a memory fault)
        m = moves[:n_store + n_fetch]
        lim_r, lim_s = min(o.shape[0] for o, _ in pairs), min(p.shape[0] for _, p in pairs)
        if not moves.is_cuda and (int(m[:, 0].min()) < 0 or int(m[:, 0].max()) >= lim_r or int(m[:, 1].min()) < 0 or
                                  int(m[:, 1].max()) >= lim_s):
            raise ValueError("moves: a row or slot outside the arrays")
    import ctypes
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ss_memo_rows_f32(ctypes.cast(io, ctypes.c_void_p), len(pairs), moves.data_ptr(), int(n_store),
                                                int(n_fetch), _stream(pairs[0][0])), "ss_memo_rows_f32")


def ctypes_ref(arr):
    import ctypes
    return ctypes.cast(arr, ctypes.c_void_p)


def intensity(audiogoal: torch.Tensor, num_frame: int = 150) -> torch.Tensor:
    """av_wan Intensity (ss_baselines/av_wan/avwan_sensors.py:91-100): [N,2,T] -> [N] mean-square of the 150 samples
    after the onset."""
    _chk(audiogoal, torch.float32, "audiogoal")
    N, two, n = audiogoal.shape
    assert two == 2
    out = torch.empty((N,), dtype=torch.float32, device=audiogoal.device)
    with torch.cuda.device(audiogoal.device):
        _lib.check(_lib.load().ss_intensity_f32(audiogoal.data_ptr(), out.data_ptr(), N, n, num_frame, _stream(audiogoal)),
                   "ss_intensity_f32")
    return out


# ---- torch.ops.ss_hip.* ------------------------------------------------------------------------------
def _load_native_ops() -> bool:
    """The TORCH_LIBRARY extension (csrc/ss_torch_ops.cpp, built in-tree by build.py): the hot ops - spectrogram, audio_obs,
    ctx_observe and the one-dispatch eager observation eager_obs - are C++ dispatches straight into libss_hip.so.  Without
    the file (a tree that was never built) the same schemas are registered from Python below, over ctypes."""
    import logging
    import os
    so = os.path.join(os.path.dirname(_lib.SO_PATH), "libss_torch_ops.so")
    if not os.path.exists(so):
        return False
    try:
        torch.ops.load_library(so)
        return True
    except OSError as e:                                    # e.g. built against another torch: keep the Python registrations
        logging.warning("ss_amd: %s did not load (%s); torch.ops.ss_hip.* stay on the Python registrations", so, e)
        return False


NATIVE_OPS = _load_native_ops()
# 2: the extension also defines source_windows / fftconv_binaural / rir_spectra / *_spec / audio_features / intensity
NATIVE_LEVEL = int(torch.ops.ss_hip.native_ops()) if NATIVE_OPS else 0


def _register():
    lib = torch.library.Library("ss_hip", "FRAGMENT" if NATIVE_OPS else "DEF")
    py2 = NATIVE_LEVEL < 2                                  # these ops are NOT defined by the C++ extension: register them here
    if py2:
        lib.define("source_windows(Tensor src, Tensor win_desc) -> Tensor")
        lib.define("fftconv_binaural(Tensor spec, Tensor rir_bank, Tensor rir_len, Tensor unit_desc, int n_valid, "
                   "int out_len, bool interleaved=False, int flags=0) -> Tensor")
    if not NATIVE_OPS:
        lib.define("spectrogram(Tensor x, int pad_mode=0) -> Tensor")
        lib.define("audio_obs(Tensor spec, Tensor rir_bank, Tensor rir_len, Tensor unit_desc, int n_valid, int out_len, "
                   "int pad_mode=0, bool interleaved=False, int flags=0) -> (Tensor, Tensor)")
    if py2:
        lib.define("intensity(Tensor audiogoal, int num_frame=150) -> Tensor")
    lib.define("gccphat(Tensor x, int max_lag=32, float eps=1e-8, int pad_mode=0) -> Tensor")
    lib.impl("gccphat", lambda x, max_lag=32, eps=1e-8, pad_mode=0: gccphat(x, max_lag, eps, pad_mode), "CUDA")
    lib.impl("gccphat", lambda x, max_lag=32, eps=1e-8, pad_mode=0:
             x.new_empty((x.shape[0], 2 * max_lag + 1, 1 + x.shape[2] // 160)), "Meta")
    lib.define("logmel(Tensor x, Tensor mel_start, Tensor mel_w, float eps=1e-6, int pad_mode=0) -> Tensor")
    lib.impl("logmel", lambda x, ms, mw, eps=1e-6, pad_mode=0: logmel(x, ms, mw, eps, pad_mode), "CUDA")
    lib.impl("logmel", lambda x, ms, mw, eps=1e-6, pad_mode=0:
             x.new_empty((x.shape[0], mw.shape[0], 1 + x.shape[2] // 160, 2)), "Meta")
    if py2:
        lib.define("audio_features(Tensor x, Tensor mel_start, Tensor mel_w, float mel_eps=1e-6, int max_lag=32, float gcc_eps=1e-8, "
                   "int pad_mode=0) -> (Tensor, Tensor)")

    def _audio_features(x, ms, mw, mel_eps=1e-6, max_lag=32, gcc_eps=1e-8, pad_mode=0):
        o = audio_features(x, ("logmel", "gccphat"), ms, mw, mel_eps, max_lag, gcc_eps, pad_mode)
        return o["logmel"], o["gccphat"]
    if py2:
        lib.impl("audio_features", _audio_features, "CUDA")
    lib.impl("audio_features", lambda x, ms, mw, mel_eps=1e-6, max_lag=32, gcc_eps=1e-8, pad_mode=0:
             (x.new_empty((x.shape[0], mw.shape[0], 1 + x.shape[2] // 160, 2)),
              x.new_empty((x.shape[0], 2 * max_lag + 1, 1 + x.shape[2] // 160))), "Meta")
    if py2:
        lib.impl("intensity", intensity, "CUDA")
        lib.impl("source_windows", source_windows, "CUDA")
        lib.impl("fftconv_binaural", fftconv_binaural, "CUDA")
    lib.impl("intensity", lambda a, num_frame=150: a.new_empty((a.shape[0],)), "Meta")
    def _audio_obs(spec, rir_bank, rir_len, unit_desc, n_valid, out_len, pad_mode=0, interleaved=False, flags=0):
        ag, sg = audio_obs(spec, rir_bank, rir_len, unit_desc, n_valid, out_len, pad_mode, True, interleaved, flags)
        return ag, sg
    if not NATIVE_OPS:
        lib.impl("spectrogram", lambda x, pad_mode=0: spectrogram(x, pad_mode), "CUDA")
        lib.impl("audio_obs", _audio_obs, "CUDA")

    # spectral RIR bank: the bank builder + the two *_spec entry points
    if py2:
        lib.define("rir_spectra(Tensor rir_bank) -> Tensor")
        lib.impl("rir_spectra", rir_spectra, "CUDA")
    lib.impl("rir_spectra", lambda b: b.new_empty((b.shape[0], 2, ceil_div(b.shape[2], KB), SPEC_FLOATS)), "Meta")
    if py2:
        lib.define("fftconv_binaural_spec(Tensor spec, Tensor hspec, Tensor rir_len, Tensor unit_desc, int n_valid, int out_len, "
                   "int flags=0) -> Tensor")

    def _conv_spec(spec, hspec, rir_len, unit_desc, n_valid, out_len, flags=0):
        out = torch.empty((unit_desc.shape[0], 2, out_len), dtype=torch.float32, device=spec.device)
        fftconv_binaural_spec_into(spec, hspec, rir_len, unit_desc, out, n_valid, flags)
        return out
    if py2:
        lib.impl("fftconv_binaural_spec", _conv_spec, "CUDA")
    lib.impl("fftconv_binaural_spec", lambda spec, h, l, d, n_valid, out_len, flags=0: spec.new_empty((d.shape[0], 2, out_len)),
             "Meta")
    if py2:
        lib.define("audio_obs_spec(Tensor spec, Tensor hspec, Tensor rir_len, Tensor unit_desc, int n_valid, int out_len, "
                   "int pad_mode=0, int flags=0) -> (Tensor, Tensor)")

    def _obs_spec(spec, hspec, rir_len, unit_desc, n_valid, out_len, pad_mode=0, flags=0):
        N = unit_desc.shape[0]
        ag = torch.empty((N, 2, out_len), dtype=torch.float32, device=spec.device)
        sg = torch.empty((N,) + spectrogram_shape(out_len), dtype=torch.float32, device=spec.device)
        audio_obs_spec_into(spec, hspec, rir_len, unit_desc, ag, sg, n_valid, out_len, pad_mode, flags)
        return ag, sg
    if py2:
        lib.impl("audio_obs_spec", _obs_spec, "CUDA")
    lib.impl("audio_obs_spec", lambda spec, h, l, d, n_valid, out_len, pad_mode=0, flags=0:
             (spec.new_empty((d.shape[0], 2, out_len)), spec.new_empty((d.shape[0],) + spectrogram_shape(out_len))), "Meta")
    # the observe-level op: one vector step through a context (planner + window cache + descriptor ring in the library).
    # `ctx` = AudioContext.handle (an integer registered by ss_amd.context); unit columns are int32 CPU tensors; the
    # spectrogram rows are written in place (rollout rows) and returned.
    def _ctx_observe(ctx, sound, t0, rir, spectrogram):
        from .context import AudioContext
        AudioContext.from_handle(ctx).observe(sound.numpy(), t0.numpy(), rir.numpy(), spectrogram_out=spectrogram)
        return spectrogram
    if not NATIVE_OPS:
        lib.define("ctx_observe(int ctx, Tensor sound, Tensor t0, Tensor rir, Tensor(a!) spectrogram) -> Tensor(a!)")
        lib.impl("ctx_observe", _ctx_observe, "CompositeExplicitAutograd")

    # shape functions (Meta) so the ops compose with tracing / fake tensors
    lib.impl("source_windows", lambda src, wd: src.new_empty((wd.shape[0], SPEC_FLOATS)), "Meta")
    lib.impl("fftconv_binaural", lambda spec, b, l, d, n_valid, out_len, interleaved=False, flags=0:
             spec.new_empty((d.shape[0], 2, out_len)), "Meta")
    lib.impl("spectrogram", lambda x, pad_mode=0: x.new_empty((x.shape[0],) + spectrogram_shape(x.shape[2])), "Meta")
    lib.impl("audio_obs", lambda spec, b, l, d, n_valid, out_len, pad_mode=0, interleaved=False, flags=0:
             (spec.new_empty((d.shape[0], 2, out_len)), spec.new_empty((d.shape[0],) + spectrogram_shape(out_len))),
             "Meta")
    return lib


_TORCH_LIB = _register()
