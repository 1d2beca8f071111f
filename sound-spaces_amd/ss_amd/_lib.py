"""ctypes binding of libss_hip.so (include/ss_hip.h).  There is NO fallback: if the HIP library is
missing or a call fails, the error is raised — the product never computes this path on the CPU."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.normpath(os.path.join(_HERE, "..", "csrc", "libss_hip.so"))

EXPORTS = ("ss_block_len", "ss_spec_floats", "ss_version", "ss_init", "ss_source_windows_f32",
           "ss_fftconv_binaural_f32", "ss_spectrogram_f32", "ss_audio_obs_f32", "ss_intensity_f32", "ss_logmel_f32", "ss_gccphat_f32",
           "ss_ctx_create", "ss_ctx_destroy", "ss_ctx_add_source", "ss_ctx_add_source_len", "ss_ctx_set_rir_bank",
           "ss_ctx_observe", "ss_ctx_plan", "ss_ctx_stats", "ss_ctx_ring_stats", "ss_ctx_set_rir_spectra",
           "ss_rir_spectra_f32", "ss_fftconv_binaural_spec_f32", "ss_audio_obs_spec_f32", "ss_ctx_observe_sims",
           "ss_ctx_sims_units", "ss_ctx_set_overlap", "ss_ctx_join", "ss_fftconv_binaural_buckets_f32",
           "ss_audio_obs_buckets_f32", "ss_ctx_set_rir_buckets", "ss_release_scratch",
           "ss_source_windows32_f32", "ss_audio_obs32_f32", "ss_ctx_observe_requests", "ss_ctx_requests_units", "ss_audio_features_f32", "ss_ctx_observe_features",
           "ss_wav_read_rirs_f32", "ss_rows_gather_f32", "ss_bank_scatter_rows_f32", "ss_ctx_set_chip_share", "ss_ctx_set_spectral_policy", "ss_ctx_observe_requests_load", "ss_ctx_load_rir_files",
           "ss_bank_scatter_spectra_f32", "ss_audio_obs_logmel_f32", "ss_audio_obs_logmel_spec_f32", "ss_ctx_set_logmel_policy",
           "ss_audio_obs_logmel_rows_f32", "ss_audio_obs_logmel_rows_spec_f32", "ss_ctx_set_logmel_rows_policy",
           "ss_audio_obs_logmel_ss2_f32", "ss_ctx_set_logmel_ss2_policy",
           "ss_rir_spectra16_f32", "ss_bank_scatter_spectra16_f32", "ss_fftconv_binaural_spec16_f32", "ss_audio_obs_spec16_f32",
           "ss_audio_obs_logmel_spec16_f32", "ss_ctx_set_rir_spectra16",
           "ss_audio_obs_rows_spec16_f32", "ss_audio_obs_logmel_rows_spec16_f32", "ss_ctx_set_rir_spectra16_rows",
           "ss_fftconv_binaural_spec_buckets_f32", "ss_audio_obs_spec_buckets_f32", "ss_ctx_set_rir_spec_buckets",
           "ss_audio_obs_logmel_buckets_f32", "ss_audio_obs_logmel_spec_buckets_f32", "ss_ctx_set_logmel_buckets_policy",
           "ss_audio_obs_rows_spec16_buckets_f32", "ss_audio_obs_logmel_rows_spec16_buckets_f32", "ss_ctx_set_rir_spec_buckets_rows",
           "ss_memo_rows_f32", "ss_ctx_memo_enable", "ss_ctx_memo_reset", "ss_ctx_memo_stats", "ss_ctx_observe_sims_memo",
           "ss_ctx_sims_memo_plan",
           "ss_rir_rows16_f32", "ss_bank_scatter_rows16_f32", "ss_fftconv_binaural_rir16_f32", "ss_audio_obs_rir16_f32",
           "ss_ctx_set_rir_bank16", "ss_audio_obs_rows_rir16_f32", "ss_ctx_set_rir_bank16_rows",
           "ss_fftconv_binaural_rir16_buckets_f32", "ss_audio_obs_rir16_buckets_f32", "ss_ctx_set_rir16_buckets",
           "ss_audio_obs_logmel_rir16_f32", "ss_audio_obs_logmel_rows_rir16_f32", "ss_audio_obs_logmel_rir16_buckets_f32",
           "ss_ctx_set_logmel_rir16_policy",
           "ss_bank_scatter_rows16_max_f32", "ss_wav_read_rirs_max_f32",
           "ss_stream_reserve", "ss_stream_replay_epoch")
# entries that return a size_t, not a status (EXPORTS: every `int ss_*` of include/ss_hip.h)
EXPORTS_SIZE = ("ss_ctx_wave_scratch_bytes",)


class SsRirBucket(ctypes.Structure):
    """struct ss_rir_bucket of include/ss_hip.h."""
    _fields_ = [("rir", ctypes.c_void_p), ("hspec", ctypes.c_void_p), ("first", ctypes.c_int), ("n_entries", ctypes.c_int),
                ("cap", ctypes.c_int), ("reserved", ctypes.c_int)]


class SsSpecBucket(ctypes.Structure):
    """struct ss_spec_bucket of include/ss_hip.h."""
    _fields_ = [("hspec", ctypes.c_void_p), ("hscale", ctypes.c_void_p), ("first", ctypes.c_int), ("n_entries", ctypes.c_int),
                ("cap", ctypes.c_int), ("reserved", ctypes.c_int)]


class SsRir16Bucket(ctypes.Structure):
    """struct ss_rir16_bucket of include/ss_hip.h."""
    _fields_ = [("rir16", ctypes.c_void_p), ("rscale", ctypes.c_void_p), ("first", ctypes.c_int), ("n_entries", ctypes.c_int),
                ("cap", ctypes.c_int), ("reserved", ctypes.c_int)]


class SsMissLoader(ctypes.Structure):
    """struct ss_miss_loader of include/ss_hip.h (ss_ctx_observe_requests_load: the miss path inside the call)."""
    _fields_ = [("table_dirs", ctypes.POINTER(ctypes.c_char_p)), ("n_table_dirs", ctypes.c_int),
                ("pair_keys", ctypes.c_void_p), ("pair_slots", ctypes.c_void_p), ("pair_cap", ctypes.c_int),
                ("free_slots", ctypes.c_void_p), ("n_free", ctypes.c_int),
                ("bank", ctypes.c_void_p), ("bank_unit_stride", ctypes.c_longlong), ("bank_chan_stride", ctypes.c_int),
                ("cap", ctypes.c_int), ("dev_len", ctypes.c_void_p), ("host_len", ctypes.c_void_p), ("clipped", ctypes.c_void_p),
                ("spec_stale", ctypes.c_void_p), ("keep", ctypes.c_int),
                ("stage", ctypes.c_void_p), ("stage_slot", ctypes.c_void_p), ("stage_len", ctypes.c_void_p),
                ("stage_desc", ctypes.c_void_p), ("stage_rows", ctypes.c_int), ("threads", ctypes.c_int),
                ("used", ctypes.c_void_p), ("use_seq", ctypes.c_void_p), ("evicted_slot", ctypes.c_void_p),
                ("n_evicted", ctypes.c_int), ("evict_cap", ctypes.c_int),
                ("loaded_key", ctypes.c_void_p), ("loaded_slot", ctypes.c_void_p), ("loaded_frames", ctypes.c_void_p),
                ("n_loaded", ctypes.c_int), ("loaded_cap", ctypes.c_int), ("stage_max", ctypes.c_void_p)]


class SsMemoIo(ctypes.Structure):
    """struct ss_memo_io of include/ss_hip.h."""
    _fields_ = [("out", ctypes.c_void_p), ("pool", ctypes.c_void_p), ("row_floats", ctypes.c_int), ("reserved", ctypes.c_int)]


class SsMemoPool(ctypes.Structure):
    """struct ss_memo_pool of include/ss_hip.h."""
    _fields_ = [("spectrogram", ctypes.c_void_p), ("audiogoal", ctypes.c_void_p), ("rows", ctypes.c_int), ("reserved", ctypes.c_int)]


class SsSimColumns(ctypes.Structure):
    """struct ss_sim_columns of include/ss_hip.h."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("sound", "audio_index", "step_count", "duration", "recv", "src", "rot", "scene",
                                              "dis_sound", "dis_src", "index_flat", "index_off", "index_dim")] + \
               [("n_scenes", ctypes.c_int), ("azimuths", ctypes.c_int)]


class SsRequestTables(ctypes.Structure):
    """struct ss_request_tables of include/ss_hip.h."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("sound_keys", "sound_ids", "table_keys", "table_ids", "pair_keys", "pair_slots",
                                              "stale")] + \
               [(n, ctypes.c_int) for n in ("n_sounds", "n_tables", "n_pairs", "n_slots")] + \
               [("last_used", ctypes.c_void_p), ("tick", ctypes.c_longlong)]


class SsFeatures(ctypes.Structure):
    """struct ss_features of include/ss_hip.h."""
    _fields_ = [("logmel", ctypes.c_void_p), ("mel_start", ctypes.c_void_p), ("mel_w", ctypes.c_void_p), ("n_mels", ctypes.c_int),
                ("max_len", ctypes.c_int), ("mel_eps", ctypes.c_float), ("gccphat", ctypes.c_void_p), ("max_lag", ctypes.c_int),
                ("gcc_eps", ctypes.c_float)]


class SsUnits(ctypes.Structure):
    """struct ss_units of include/ss_hip.h: host struct-of-arrays descriptors of one step."""
    _fields_ = [("sound", ctypes.c_void_p), ("t0", ctypes.c_void_p), ("rir", ctypes.c_void_p),
                ("dis_sound", ctypes.c_void_p), ("dis_rir", ctypes.c_void_p), ("last_rir", ctypes.c_void_p),
                ("wrap", ctypes.c_void_p), ("last_wrap", ctypes.c_void_p)]

_lib = None


class SsHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise SsHipError(f"{SO_PATH} not found: build it with `python sound-spaces_amd/build.py` "
                         "(or __graft_entry__.build()); there is no CPU fallback for this path")
    lib = ctypes.CDLL(SO_PATH)
    c_int, c_ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    lib.ss_block_len.restype = c_int
    lib.ss_spec_floats.restype = c_int
    lib.ss_version.restype = c_int
    lib.ss_init.restype = c_int
    lib.ss_source_windows_f32.argtypes = [vp, vp, vp, c_int, vp]
    lib.ss_fftconv_binaural_f32.argtypes = [vp, vp, vp, vp, vp, c_int, c_ll, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_spectrogram_f32.argtypes = [vp, vp, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_f32.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_ll, c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_intensity_f32.argtypes = [vp, vp, c_int, c_int, c_int, vp]
    lib.ss_gccphat_f32.argtypes = [vp, vp, c_int, c_int, c_int, c_int, ctypes.c_float, vp]
    lib.ss_logmel_f32.argtypes = [vp, vp, c_int, c_int, c_int, vp, vp, c_int, c_int, ctypes.c_float, vp]
    pp = ctypes.POINTER(ctypes.c_void_p)
    lib.ss_ctx_create.argtypes = [pp, c_int, c_int, c_int, c_int, c_int]
    lib.ss_ctx_destroy.argtypes = [vp]
    lib.ss_ctx_add_source.argtypes = [vp, vp, c_int, c_int]
    lib.ss_ctx_add_source_len.argtypes = [vp, c_int]
    lib.ss_ctx_set_rir_bank.argtypes = [vp, vp, vp, c_ll, c_int, c_int, c_int]
    lib.ss_ctx_observe.argtypes = [vp, ctypes.POINTER(SsUnits), c_int, vp, vp, vp]
    lib.ss_ctx_plan.argtypes = [vp, ctypes.POINTER(SsUnits), c_int, vp, vp, vp, vp, c_int]
    lib.ss_ctx_stats.argtypes = [vp, vp]
    lib.ss_ctx_ring_stats.argtypes = [vp, vp]
    lib.ss_ctx_observe_sims.argtypes = [vp, ctypes.POINTER(SsSimColumns), c_int, vp, vp, vp, vp, vp]
    lib.ss_ctx_sims_units.argtypes = [vp, ctypes.POINTER(SsSimColumns), c_int, vp, vp, vp]
    lib.ss_ctx_set_rir_spectra.argtypes = [vp, vp, c_int]
    lib.ss_ctx_set_overlap.argtypes = [vp, c_int]
    lib.ss_fftconv_binaural_buckets_f32.argtypes = [vp, vp, c_int, vp, vp, vp, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_buckets_f32.argtypes = [vp, vp, c_int, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_ctx_set_rir_buckets.argtypes = [vp, vp, c_int, vp]
    lib.ss_ctx_join.argtypes = [vp, vp]
    lib.ss_ctx_set_chip_share.argtypes = [vp, c_int]
    lib.ss_ctx_set_spectral_policy.argtypes = [vp, c_int]
    lib.ss_rir_spectra_f32.argtypes = [vp, vp, c_int, c_ll, c_int, c_int, vp]
    lib.ss_fftconv_binaural_spec_f32.argtypes = [vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_spec_f32.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_logmel_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, ctypes.c_float, c_int, c_ll, c_int, c_int,
                                            c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_logmel_spec_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, ctypes.c_float, c_int, c_int, c_int,
                                                 c_int, c_int, c_int, vp]
    lib.ss_ctx_set_logmel_policy.argtypes = [vp, c_int, c_int]
    lib.ss_audio_obs_logmel_rows_f32.argtypes = lib.ss_audio_obs_logmel_f32.argtypes
    lib.ss_audio_obs_logmel_rows_spec_f32.argtypes = lib.ss_audio_obs_logmel_spec_f32.argtypes
    lib.ss_ctx_set_logmel_rows_policy.argtypes = [vp, c_int, c_int]
    lib.ss_audio_obs_logmel_ss2_f32.argtypes = lib.ss_audio_obs_logmel_f32.argtypes
    lib.ss_ctx_set_logmel_ss2_policy.argtypes = [vp, c_int, c_int]
    lib.ss_ctx_wave_scratch_bytes.argtypes = [vp]
    lib.ss_source_windows32_f32.argtypes = [vp, vp, vp, c_int, vp]
    lib.ss_audio_obs32_f32.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_ll, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_features_f32.argtypes = [vp, c_int, c_int, c_int, vp, vp, vp, vp, c_int, c_int, ctypes.c_float, vp, c_int,
                                          ctypes.c_float, vp]
    lib.ss_ctx_observe_features.argtypes = [vp, ctypes.POINTER(SsUnits), c_int, vp, vp, ctypes.POINTER(SsFeatures), vp]
    lib.ss_ctx_observe_requests.argtypes = [vp, vp, c_int, vp, vp, vp, vp, vp, vp]
    lib.ss_ctx_requests_units.argtypes = [vp, vp, c_int, vp, vp, vp, vp]
    lib.ss_ctx_observe_requests_load.argtypes = [vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.ss_ctx_load_rir_files.argtypes = [vp, vp, vp, c_int, vp, c_ll, c_int, vp]
    lib.ss_wav_read_rirs_f32.argtypes = [vp, c_int, vp, c_ll, c_int, c_int, c_int, vp, vp, vp, c_int]
    lib.ss_rows_gather_f32.argtypes = [vp, vp, c_int, vp, c_ll, c_int, c_int]
    lib.ss_bank_scatter_rows_f32.argtypes = [vp, c_ll, vp, vp, c_int, vp, c_ll, c_int, c_int, vp, vp]
    lib.ss_bank_scatter_spectra_f32.argtypes = [vp, c_ll, c_int, vp, vp, c_int, vp, c_int, vp, vp]
    # the half bank (fp16 block spectra + scales): the _spec_f32 siblings' arguments plus hscale behind the bank
    lib.ss_rir_spectra16_f32.argtypes = [vp, vp, vp, c_int, c_ll, c_int, c_int, vp]
    lib.ss_bank_scatter_spectra16_f32.argtypes = [vp, c_ll, c_int, vp, vp, c_int, vp, vp, c_int, vp, vp]
    lib.ss_fftconv_binaural_spec16_f32.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_spec16_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_logmel_spec16_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, ctypes.c_float, c_int, c_int,
                                                   c_int, c_int, c_int, c_int, vp]
    lib.ss_ctx_set_rir_spectra16.argtypes = [vp, vp, vp, c_int]
    # ... for rows of 2 or 3 partition blocks (44.1 / 48 kHz)
    lib.ss_audio_obs_rows_spec16_f32.argtypes = lib.ss_audio_obs_spec16_f32.argtypes
    lib.ss_audio_obs_logmel_rows_spec16_f32.argtypes = lib.ss_audio_obs_logmel_spec16_f32.argtypes
    lib.ss_ctx_set_rir_spectra16_rows.argtypes = [vp, vp, vp, c_int]
    # spectral length buckets (ss_spec_bucket): the ss_*_buckets_f32 arguments
    lib.ss_fftconv_binaural_spec_buckets_f32.argtypes = lib.ss_fftconv_binaural_buckets_f32.argtypes
    lib.ss_audio_obs_spec_buckets_f32.argtypes = lib.ss_audio_obs_buckets_f32.argtypes
    lib.ss_ctx_set_rir_spec_buckets.argtypes = [vp, vp, c_int, vp]
    # log-mel from length buckets of either kind: the bucket array, the outputs and mel arguments of ss_audio_obs_logmel_f32
    lib.ss_audio_obs_logmel_buckets_f32.argtypes = [vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, ctypes.c_float, c_int,
                                                    c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_logmel_spec_buckets_f32.argtypes = lib.ss_audio_obs_logmel_buckets_f32.argtypes
    lib.ss_ctx_set_logmel_buckets_policy.argtypes = [vp, c_int, c_int]
    # half spectral length buckets for rows of 2 or 3 partition blocks (44.1 / 48 kHz)
    lib.ss_audio_obs_rows_spec16_buckets_f32.argtypes = lib.ss_audio_obs_spec_buckets_f32.argtypes
    lib.ss_audio_obs_logmel_rows_spec16_buckets_f32.argtypes = lib.ss_audio_obs_logmel_spec_buckets_f32.argtypes
    lib.ss_ctx_set_rir_spec_buckets_rows.argtypes = [vp, vp, c_int, vp]
    # half-precision time-domain rows (fp16 rows + one scale per (entry, ear))
    lib.ss_rir_rows16_f32.argtypes = [vp, vp, vp, c_int, c_ll, c_int, c_int, vp]
    lib.ss_bank_scatter_rows16_f32.argtypes = [vp, c_ll, vp, vp, c_int, vp, vp, c_int, vp, vp]
    lib.ss_fftconv_binaural_rir16_f32.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_rir16_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_ctx_set_rir_bank16.argtypes = [vp, vp, vp, vp, c_int]
    lib.ss_audio_obs_rows_rir16_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]
    lib.ss_ctx_set_rir_bank16_rows.argtypes = [vp, vp, vp, vp, c_int]
    # ... in length buckets (ss_rir16_bucket): the ss_*_buckets_f32 arguments
    lib.ss_fftconv_binaural_rir16_buckets_f32.argtypes = lib.ss_fftconv_binaural_buckets_f32.argtypes
    lib.ss_audio_obs_rir16_buckets_f32.argtypes = lib.ss_audio_obs_buckets_f32.argtypes
    lib.ss_ctx_set_rir16_buckets.argtypes = [vp, vp, c_int, vp]
    # ... and their one-launch log-mel forms
    lib.ss_audio_obs_logmel_rir16_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, c_int, c_int, ctypes.c_float, c_int, c_int,
                                                  c_int, c_int, c_int, c_int, vp]
    lib.ss_audio_obs_logmel_rows_rir16_f32.argtypes = lib.ss_audio_obs_logmel_rir16_f32.argtypes
    lib.ss_audio_obs_logmel_rir16_buckets_f32.argtypes = lib.ss_audio_obs_logmel_buckets_f32.argtypes
    lib.ss_ctx_set_logmel_rir16_policy.argtypes = [vp, c_int, c_int]
    # ... their one-pass scatter (the rows' maxima given) and the reader that takes the maxima
    lib.ss_bank_scatter_rows16_max_f32.argtypes = [vp, c_ll, vp, vp, vp, c_int, vp, vp, c_int, vp, vp]
    lib.ss_wav_read_rirs_max_f32.argtypes = [vp, c_int, vp, c_ll, c_int, c_int, vp, vp, vp, c_int, vp]
    # captured steps: what a stream's first rows launches would allocate, and the replay epoch of its hand-off area
    lib.ss_stream_reserve.argtypes = [vp, c_int, c_int, c_int]
    lib.ss_stream_replay_epoch.argtypes = [vp, vp]
    # pose memo of the column path
    lib.ss_memo_rows_f32.argtypes = [vp, c_int, vp, c_int, c_int, vp]
    lib.ss_ctx_memo_enable.argtypes = [vp, c_int]
    lib.ss_ctx_memo_reset.argtypes = [vp]
    lib.ss_ctx_memo_stats.argtypes = [vp, vp]
    lib.ss_ctx_observe_sims_memo.argtypes = [vp, ctypes.POINTER(SsSimColumns), c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.ss_ctx_sims_memo_plan.argtypes = [vp, ctypes.POINTER(SsSimColumns), c_int, c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    for name in EXPORTS:
        getattr(lib, name).restype = c_int
    for name in EXPORTS_SIZE:
        getattr(lib, name).restype = ctypes.c_size_t
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        kind = "invalid argument" if rc == -1 else f"hipError_t {-rc}"
        raise SsHipError(f"{what} failed: {kind}")


WAV_OK, WAV_UNSUPPORTED, WAV_EMPTY, WAV_MISSING, WAV_TOO_LONG = 0, 1, 2, 3, 4


_n_threads = 0


def _default_threads() -> int:
    """threads of the library's host pool for this process (asked once: the affinity mask is a system call)"""
    global _n_threads
    if _n_threads <= 0:
        _n_threads = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    return _n_threads


def wav_read_rirs(paths, dst, cap: int, keep: int = -1, planar: bool = False, threads: int = 0):
    """ss_wav_read_rirs_f32: the float32 stereo wav files `paths` -> rows of the HOST float32 numpy array `dst`
    ([n, cap, 2] wav-interleaved, or [n, 2, cap] with planar=True; C-contiguous, typically the numpy view of a pinned
    torch tensor).  -> (kept, frames, status) int32 arrays (include/ss_hip.h).  Host-only: works without a GPU."""
    import numpy as np
    n = len(paths)
    assert dst.dtype == np.float32 and dst.flags.c_contiguous and dst.shape[0] >= n and dst[0].size == 2 * cap
    kept, frames, status = (np.zeros((n,), np.int32) for _ in range(3))
    if n == 0:
        return kept, frames, status
    arr = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    if threads <= 0:
        threads = _default_threads()
    check(load().ss_wav_read_rirs_f32(ctypes.cast(arr, ctypes.c_void_p), n, dst.ctypes.data, 2 * cap, cap, keep, int(planar),
                                      kept.ctypes.data, frames.ctypes.data, status.ctypes.data, threads), "ss_wav_read_rirs_f32")
    return kept, frames, status
