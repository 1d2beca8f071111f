/* ss_hip.h — C ABI of libss_hip.so: the MI355X (gfx950) audio-observation path of SoundSpaces.
 *
 * Every entry point replaces one piece of reference Python (paths relative to the
 * facebookresearch/sound-spaces checkout) and is what a ctypes/cffi binding on the
 * reference side would bind:
 *
 *   ss_fftconv_binaural_f32  <- SoundSpacesSim._compute_audiogoal: the two
 *                               scipy.signal.fftconvolve calls + slicing, all three windowing
 *                               branches, the distractor add and the silent / empty-RIR zeros
 *                               (soundspaces/simulator.py:608-666); also
 *                               ContinuousSoundSpacesSim._convolve_with_rir
 *                               (soundspaces/continuous_simulator.py:428-456)
 *   ss_spectrogram_f32       <- SpectrogramSensor.compute_spectrogram
 *                               (soundspaces/tasks/nav.py:86-100): librosa.stft(512,160,400) ->
 *                               abs -> block_reduce(4,4,mean) -> log1p -> stack(axis=-1)
 *   ss_audio_obs_f32         <- get_current_spectrogram_observation on a cache miss
 *                               (soundspaces/simulator.py:690-701), both stages fused
 *   ss_intensity_f32         <- Intensity.get_observation (ss_baselines/av_wan/avwan_sensors.py:91-100)
 *   ss_gccphat_f32           <- extension, not in the reference (GCC-PHAT inter-aural feature of configs[4])
 *   ss_logmel_f32            <- extension, not in the reference (log-mel front end named by the north star)
 *   ss_source_windows_f32    <- the FFT of the source clip that fftconvolve recomputes on every
 *                               call (simulator.py:630) hoisted out and cached per (sound, window)
 *
 * Conventions: all pointers are DEVICE pointers owned by the caller (no torch types, no host
 * buffers); `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 * asynchronous on that stream; return 0 on success, SS_EINVAL for bad arguments, or the negated
 * hipError_t of the failing runtime call.  The library keeps only immutable per-device twiddle /
 * window tables, built on first use (thread-safe).
 */
#ifndef SS_HIP_H
#define SS_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_EINVAL (-1)
#define SS_PAD_REFLECT 0   /* librosa < 0.10 default (the reference's era), torch.stft default */
#define SS_PAD_CONSTANT 1  /* librosa >= 0.10 default */
/* flags: promises from the caller that let the library pick a leaner kernel */
#define SS_FLAG_NO_DISTRACTOR 1  /* term 1 of every unit descriptor is absent ([4] == -1); it is then ignored */
/* SoundSpaces 2.0 CROSSFADE (soundspaces/continuous_simulator.py:47-53, 422-424): term 1 of a unit descriptor is the
 * PREVIOUS step's RIR (`_last_rir`), not a distractor: where it is present the row is
 *   out[:, n] = conv(term 1)[n] * (F - n)/F + conv(term 0)[n] * n/F   for n <= F = int(0.05 * out_len),
 *   out[:, n] = conv(term 0)[n]                                         beyond
 * (rows are 1 s long in both simulators, so out_len is the sampling rate); units whose term 1 is absent
 * (first step of an episode, `_last_rir is None`) are not blended.  One launch; with ss_audio_obs_f32 the spectrogram
 * is taken from the blended row.  F <= 2414 (sampling rates up to 48 kHz): the ramp waits in LDS while the row is convolved
 * with the current RIR; longer ramps are refused (SS_EINVAL). */
#define SS_FLAG_CROSSFADE 2
/* length-bucketed banks (ss_rir_bucket): every bank index the launch references lies in bucket 0, so the loop-free
 * kernels may serve it (the context's planner sets it per step) */
#define SS_FLAG_FIRST_BUCKET 4

/* Geometry constants of the partitioned convolution. */
int ss_block_len(void);        /* kB = 16384 real samples per partition block                     */
int ss_spec_floats(void);      /* floats per stored window spectrum = 2 * 16384                   */
int ss_version(void);

/* Build (idempotent) the constant tables for the current HIP device. */
int ss_init(void);
/* Rows longer than kB (44.1 kHz) make the library keep a scratch per (device, stream) for the block spectra of the rows in
 * flight (96 MiB per stream at 44.1 kHz without distractors), allocated by the stream's first such call (inside a
 * hipGraph capture that call is refused with SS_EINVAL: see "Captured steps" below).  This frees all of them (after a device
 * synchronise), and the contexts' waveform scratches of ss_ctx_observe_features (which grow again on demand).  A graph
 * captured before this call holds pointers to what it freed: capture again. */
int ss_release_scratch(void);

/* ---- Captured steps (hipGraph / torch.cuda.graph) ------------------------------------------------------------------------
 * The stateless entries (everything that is not ss_ctx_*) may be captured into a graph and replayed, on every route, on a
 * stream that was RESERVED (ss_stream_reserve) or WARMED UP (one eager call of the same shape on that stream).  What a first
 * call allocates cannot be allocated inside a capture: the scratch and the hand-off area of rows longer than kB - a call that
 * would have to allocate or grow one while its stream is being captured is refused with SS_EINVAL, nothing is allocated,
 * nothing is enqueued - and the device's constant tables (ss_init, ss_stream_reserve or any earlier call has built them: the
 * library does not check this one).  The scratches belong to the (device, stream) pair, so capture on the stream that was prepared, and as ONE linear
 * chain on that ONE stream: a graph whose branches could run two of these launches at once would share one scratch between
 * them.  Replays and eager calls may alternate on the stream.
 * Small steps of rows longer than kB (k_obs_blocks, see ss_audio_obs_f32) hand samples between workgroups through flags that
 * carry the launch's epoch.  An eager launch gets a positive epoch from a host counter as a kernel argument; a captured launch
 * is enqueued as TWO kernels, k_sync_next and k_obs_blocks: the first moves a word of the hand-off area on to the next replay
 * epoch (-1, -2, ...), the second reads its epoch from that word - so every replay has an epoch of its own, and the two kinds
 * never meet.
 * The context entries (ss_ctx_*) are NOT part of this: their descriptor ring waits on events on the host.
 *
 * ss_stream_reserve allocates what the rows entries (ss_audio_obs_f32 and its siblings on rows of out_len samples, kB <
 * out_len <= 3 kB) would allocate on their first use on `stream` for banks of up to rir_cap samples per row and n_terms terms
 * per unit (1: every launch carries SS_FLAG_NO_DISTRACTOR; 2 otherwise): the hand-off area and the scratch at its largest
 * size for that shape, and the constant tables.  SS_EINVAL, before a device is touched: hipStreamPerThread, out_len outside
 * (kB, 3 kB], rir_cap < 1, n_terms outside {1, 2}.  SS_EINVAL on a stream that is being captured. */
int ss_stream_reserve(void* stream, int out_len, int rir_cap, int n_terms);
/* Synchronises the stream and returns the replay epoch word of its hand-off area: 0 = no replay yet, -k after the k-th replay
 * of a captured k_obs_blocks launch.  SS_EINVAL when the stream has no hand-off area.  For tests and diagnostics. */
int ss_stream_replay_epoch(void* stream, int* out);

/* Source-window spectra.  win_desc[w] = {src_offset, src_len, start, wrap} (int32 x4):
 * window w holds samples src[src_offset + start + n], n in [0, 2*kB), zero outside [0, src_len)
 * (wrap != 0: indices >= src_len continue from the start of the clip, SS2.0 semantics).
 * For the convolution out[t] = sum_k h[k] x[t0+t-k] the window of partition offset m starts at
 * start = t0 + (m-1)*kB.  spec_out receives W * ss_spec_floats() floats (opaque kernel order). */
int ss_source_windows_f32(const float* src, const int* win_desc, float* spec_out, int n_windows,
                          void* stream);

/* Batched binaural convolution.  One unit = one (env, rotation) observation.
 * unit_desc[n] = 8 x int32, two terms k = 0 (source), 1 (distractor):
 *   [4k+0] RIR bank index, or -1 if the term is absent (both absent = silent unit -> exact zeros)
 *   [4k+1] slot (index into spec, in windows) of the spectrum for partition offset m_min
 *   [4k+2] m_min   [4k+3] number of consecutive offsets stored
 * RIR bank addressing: sample j of ear c of entry r is
 *   rir[r*rir_unit_stride + c*rir_chan_stride + j*rir_elem_stride], j < rir_len[r]
 *   (planar [R,2,L]: (2L, L, 1);  wav-interleaved [R,L,2]: (2L, 1, 2)).
 * Bank rows must be ZERO for rir_len[r] <= j < rir_cap (rir_cap = L of the bank): the kernel reads
 * up to rir_cap without per-sample length checks; rir_len only selects how many blocks are transformed.
 * out: [n_units, 2, out_len]; the first n_valid samples of every row are computed, the rest zeroed
 * (SS2.0 pads 0.25 s steps to 1 s).  n_valid <= 3*kB. */
int ss_fftconv_binaural_f32(const float* spec, const float* rir, const int* rir_len,
                            const int* unit_desc, float* out, int n_units,
                            long long rir_unit_stride, int rir_chan_stride, int rir_elem_stride,
                            int rir_cap, int n_valid, int out_len, int flags, void* stream);

/* Spectrogram of x [n_units, 2, len] -> out [n_units, 65, ceil((1+len/160)/4), 2] (channel-last).
 * Any len >= 1 (len <= 0: SS_EINVAL).  Centre padding (256 samples at each end) with SS_PAD_REFLECT follows
 * np.pad(mode="reflect") at EVERY length: padded position i reads sample (i mod 2(len-1)) folded back at len-1, so rows
 * shorter than 257 samples are reflected more than once and a row of one sample is repeated - what librosa.stft computes. */
int ss_spectrogram_f32(const float* x, float* out, int n_units, int len, int pad_mode, void* stream);

/* Fused observation: convolution + spectrogram in ONE launch for rows of up to 3*kB samples (16 kHz: 1 block; 44.1 /
 * 48 kHz, the reference's Replica rate: 3 blocks, STFT streamed behind the output blocks).  audiogoal may be NULL: the
 * waveform then never leaves the CU - cross-faded rows (SS_FLAG_CROSSFADE) included, at either length.  Rows longer than kB
 * of which ONE block is rendered (n_valid <= kB: every SoundSpaces 2.0 step at 44.1 kHz) are served by the fused loop kernel
 * in one launch, audiogoal buffer or not (block spectra accumulated in registers; time-domain banks).  With an audiogoal
 * buffer, cross-faded rows with more than one rendered block take two launches (convolution, spectrogram), which is 20 %
 * faster than their one-launch form.  Pooled blocks that lie behind the rendered samples of a short step are exact zeros
 * and are written, not computed.  For rows longer than kB the library keeps a per-(device, stream) scratch for the block spectra of
 * the rows in flight (<= 2 x ceil(rir_cap/kB) x 128 KiB per CU), allocated on the stream's first such call.
 * Small steps of such rows (rows x output blocks <= the launch's share of the CUs: <= 42 units at 44.1 kHz) are rendered by one
 * workgroup per OUTPUT BLOCK (k_obs_blocks): the samples in front of a block boundary are handed to the next block's workgroup
 * through a per-(device, stream) area of 1.3 MB whose flags carry the launch's epoch - a host counter for an eager launch, a
 * word of the area for a launch captured into a hipGraph, so that such a launch may be replayed ("Captured steps" above).
 * out_len >= 257 (SS_EINVAL below, here and in the *_spec_ / *_buckets_ / 32 forms): the fused kernels reflect the centre
 * padding once.  Shorter rows: ss_fftconv_binaural_f32, then ss_spectrogram_f32 (any length). */
int ss_audio_obs_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc,
                     float* audiogoal, float* spectrogram, int n_units,
                     long long rir_unit_stride, int rir_chan_stride, int rir_elem_stride,
                     int rir_cap, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* ---- Spectral RIR bank ("store the RIR bank as half-spectra: x2 bytes, -50 % FLOPs") -----------------------
 * SoundSpaces 1.0 RIRs are static files (simulator.py:615-618), so the forward FFT of the RIR that fftconvolve repeats
 * on every step (:630) can be done ONCE when the bank is built.  ss_rir_spectra_f32 turns a planar time-domain bank
 * (sample j of ear c of entry r at rir[r*rir_unit_stride + c*rir_chan_stride + j], rows zero beyond their length up to
 * rir_cap) into hspec_out = n_entries * 2 * h_blocks * ss_spec_floats() floats, h_blocks = ceil(rir_cap / kB): the
 * block spectra of every (entry, ear) in the kernels' register order (opaque).  Synchronous (one-off, at bank load).
 * The *_spec_* entry points are ss_fftconv_binaural_f32 / ss_audio_obs_f32 reading that bank: same unit descriptors,
 * same rir_len (it still says how many blocks of an entry are non-zero), same results to fp32 rounding, no forward
 * FFT.  They read 2x the bytes per RIR; SS_FLAG_CROSSFADE is not supported (live SS2.0 RIRs have no static bank). */
int ss_rir_spectra_f32(const float* rir, float* hspec_out, int n_entries, long long rir_unit_stride,
                       int rir_chan_stride, int rir_cap, void* stream);
int ss_fftconv_binaural_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                                 float* out, int n_units, int h_blocks, int n_valid, int out_len, int flags,
                                 void* stream);
int ss_audio_obs_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                          float* audiogoal, float* spectrogram, int n_units, int h_blocks, int n_valid, int out_len,
                          int pad_mode, int flags, void* stream);

/* Log-mel observation in ONE launch, without a waveform buffer (EXTENSION): the fused kernels' STFT phase goes on from the
 * power spectrum to the mel bands, logmel[n, j, tf, c] = exactly what ss_logmel_f32 of the row ss_audio_obs_f32 writes would
 * give (samples >= n_valid zero, centre padding by pad_mode), and - when `spectrogram` is given - the pooled spectrogram of the
 * same frames (equal to ss_audio_obs_f32's to rounding).  `logmel` [n, n_mels, 1 + out_len/160, 2] is required; `audiogoal`
 * and `spectrogram` may each be NULL (an audiogoal buffer is written as by ss_audio_obs_f32).  mel arguments as
 * ss_audio_features_f32: n_mels <= 64, max_len <= 64 and a multiple of 4, n_mels * max_len <= 3072, mel_start[j] multiples of 4
 * in [0, 256], mel_w 16-byte aligned, mel_eps > 0.  Served shapes: rows of one partition block, 257 <= out_len <= kB (16 kHz),
 * without SS_FLAG_CROSSFADE; any RIR length and distractor terms are fine.  Everything else is SS_EINVAL from the argument
 * checks, before a device is touched: this level owns no scratch to fall back on (ss_ctx_observe_features does). */
int ss_audio_obs_logmel_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc,
                            float* audiogoal, float* spectrogram, float* logmel, const int* mel_start, const float* mel_w,
                            int n_mels, int max_len, float mel_eps, int n_units, long long rir_unit_stride,
                            int rir_chan_stride, int rir_elem_stride, int rir_cap, int n_valid, int out_len, int pad_mode,
                            int flags, void* stream);
int ss_audio_obs_logmel_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                                 float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                 const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int h_blocks,
                                 int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* ---- Half-precision spectral bank (EXTENSION, opt-in, LOSSY) ----------------------------------------------------------------
 * The block spectra of the bank above stored as IEEE fp16 with one power-of-two fp32 scale per (entry r, ear c, block b): half
 * the bytes of the fp32 spectral form, i.e. what the time-domain row costs.  For each block, v[0 .. ss_spec_floats()) being the
 * fp32 block spectrum exactly as ss_rir_spectra_f32 / ss_bank_scatter_spectra_f32 store it (same element order; the packed
 * (DC, Nyquist) item is a pair of components like any other):
 *     mx = max |v[k]|;  mx == 0: every half is +0 and hscale = 1;
 *     otherwise, 2^(e-1) <= mx < 2^e:  q[k] = fp16(v[k] * 2^(15-e)) rounded to nearest even,  hscale = 2^(e-15)
 * (the scaled maximum lies in [2^14, 2^15]: nothing overflows, whatever the scale of the RIR file).  hspec16 is
 * [entries][2][h_blocks][ss_spec_floats()] halves (8-byte aligned), hscale [entries][2][h_blocks] floats; float(q) * hscale is
 * the value the kernels use, exact in fp32.  BOTH arrays of a bank must be zero-initialised: an unused or empty entry has to
 * multiply out to exact zeros (the loop-free kernel never reads rir_len).
 * Accuracy: against the fp32 path the waveform moves by about 2e-4 of its peak and the pooled log1p spectrogram by about 1e-4
 * (1.5-2.2e-4 and 0.9-1.0e-4 over the RIRs tried; INTEGRATION.md "Half-precision spectral banks" says which figure was measured
 * how) - outside the library's 1e-4 parity budget, which is why the format is never a default.
 * Producers: ss_rir_spectra16_f32 (a planar device bank -> its half form, entry r to entry r; asynchronous on `stream`) and
 * ss_bank_scatter_spectra16_f32 (staged rows, see ss_bank_scatter_spectra_f32).  Both quantise the bit-identical fp32 values.
 * Consumers: the three entries below = their _spec_f32 siblings reading a half bank (k_conv_spec<.., HALF>), same results as
 * those fed float(q) * hscale.  ss_fftconv_binaural_spec16_f32 serves every row length its sibling serves;
 * ss_audio_obs_spec16_f32 rows of ONE partition block, 257 <= out_len <= kB (16 kHz); ss_audio_obs_logmel_spec16_f32 the shapes
 * of ss_audio_obs_logmel_spec_f32.  No SS_FLAG_CROSSFADE; one allocation (a half bank in length buckets has entries of its own:
 * "Spectral length buckets" below, ss_spec_bucket).  Everything else (longer fused rows, NULL hscale,
 * h_blocks < 1, a misaligned bank, the mel limits) is SS_EINVAL from the argument checks, before a device is touched.  Rows of
 * 2 or 3 partition blocks (44.1 / 48 kHz) have entries of their own, below (ss_audio_obs_rows_spec16_f32).  Not provided: a half
 * form of the persistent k_conv_spec_rows (launches of more rows than CUs run one workgroup per row). */
int ss_rir_spectra16_f32(const float* rir, void* hspec16_out, float* hscale_out, int n_entries, long long rir_unit_stride,
                         int rir_chan_stride, int rir_cap, void* stream);
int ss_fftconv_binaural_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                   const int* unit_desc, float* out, int n_units, int h_blocks, int n_valid, int out_len,
                                   int flags, void* stream);
int ss_audio_obs_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                            const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int h_blocks, int n_valid,
                            int out_len, int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                   const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                   const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                   int h_blocks, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* The half bank for rows of 2 or 3 partition blocks (kB < out_len <= 3 kB: 44.1 / 48 kHz; EXTENSION, opt-in, LOSSY as above).
 * Same format: a 44.1 kHz entry is 3 blocks x 2 ears x (65 536 + 4) + 4 = 393 244 bytes (fp32 spectral-only: 786 436; rows and
 * spectra: 1 139 236; the bare time-domain row: 352 800).  Format loss at 44.1 kHz: INTEGRATION.md "Half-precision spectral banks".
 * ss_audio_obs_rows_spec16_f32 = ss_audio_obs_spec_f32 on such rows reading a half bank, routed as that entry routes them:
 * k_obs_blocks<.., HALF> while the grid fits the chip, k_obs_rows<.., HALF> beyond (one launch, `audiogoal` may be NULL); the
 * shapes that entry renders unfused (n_valid <= kB with a waveform buffer) go to ss_fftconv_binaural_spec16_f32 + the
 * spectrogram kernel.  ss_audio_obs_logmel_rows_spec16_f32 = ss_audio_obs_logmel_rows_spec_f32 (below) reading a half bank:
 * `audiogoal` and `spectrogram` may each be NULL.  Same results as the siblings fed float(q) * hscale.  SS_EINVAL before a device
 * is touched: SS_FLAG_CROSSFADE, NULL or misaligned (& 7) halves, NULL scales, h_blocks outside 1..16, out_len <= kB or > 3 kB,
 * the mel limits.  n_units == 0 returns 0. */
int ss_audio_obs_rows_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                 const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int h_blocks,
                                 int n_valid, int out_len, int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_rows_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                        const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                        const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps,
                                        int n_units, int h_blocks, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* ---- Half-precision time-domain rows (EXTENSION, opt-in, LOSSY) ---------------------------------------------------------------
 * The TIME-DOMAIN bank stored as IEEE fp16 with one power-of-two fp32 scale per (entry r, ear c): half the bytes of the plain row,
 * the cheapest form a bank has.  rir16 is [entries][2][cap] halves, planar, cap even, the base 4-byte aligned; rscale is
 * [entries][2] floats.  For a row v[0 .. cap), zero behind its length (the rule of the half spectral bank above, per row):
 *     mx = max |v[k]|;  mx == 0: every half is +0 and rscale = 1;
 *     otherwise, 2^(e-1) <= mx < 2^e:  q[k] = fp16(v[k] * 2^(15-e)) rounded to nearest even,  rscale = 2^(e-15).
 * float(q) * rscale is the sample the kernels transform, exact in fp32.  BOTH arrays of a bank must be zero-initialised: an unused
 * or empty entry then multiplies out to exact zeros (the table-form kernel never reads rir_len).  Rows are finite.
 * Bytes per entry: 16 kHz (cap 16 000) 2 x 32 000 + 8 = 64 008 (fp32 row 128 000, half spectra 131 080, fp32 spectra only 262 144,
 * rows and spectra 390 144); 44.1 kHz (cap 44 100) 176 408 (fp32 row 352 800, half spectra 393 244).  Rows are not padded to whole
 * partition blocks as the spectral forms are.
 * Accuracy (a property of the FORMAT, measured on a float64 model on the CPU - tests/rir16_ref.py: direct convolution of synthetic
 * clips with synthetic RIRs put through the rule above, against the same RIRs unquantised; 16 kHz at 9 000 / 16 000 taps and
 * 44.1 kHz at 9 000 / 44 100 taps, entries scaled by 1, 32 768 and 1e-6): the waveform moves by 1.7-2.3e-4 of its peak, the pooled
 * log1p spectrogram by 0.4-1.8e-4 (INTEGRATION.md "Half-precision time-domain rows") - outside the library's 1e-4 parity budget,
 * which is why the form is never a default.
 * Producers: ss_rir_rows16_f32 (a planar fp32 device bank -> its half form, entry r to entry r; k_rows_half) and
 * ss_bank_scatter_rows16_f32 (staged rows, the contract of ss_bank_scatter_rows_f32; below) and its one-pass form
 * ss_bank_scatter_rows16_max_f32 (the rows' maxima given).  All give the same bits for the same rows.
 * Consumers (k_conv<.., HALF>: only the loads in front of the first FFT pass differ, so the results equal those of the fp32
 * entries fed float(q) * rscale):
 *   ss_fftconv_binaural_rir16_f32   every shape ss_fftconv_binaural_f32 serves on a planar bank without SS_FLAG_CROSSFADE;
 *   ss_audio_obs_rir16_f32          the one-launch fused form, 257 <= out_len <= kB (and at most 26 pooled blocks); `audiogoal` may
 *                                   be NULL.  Longer rows: ss_fftconv_binaural_rir16_f32 + ss_spectrogram_f32 (what a context
 *                                   bound by ss_ctx_set_rir_bank16 does), or
 *   ss_audio_obs_rows_rir16_f32     rows of 2 or 3 partition blocks (kB < out_len <= 3 kB: 44.1 / 48 kHz) in one launch, as
 *                                   ss_audio_obs_rows_spec16_f32 serves them from half spectra: small steps take k_obs_blocks (one
 *                                   workgroup per output block, launch_obs_blocks' rule), larger ones k_obs_rows - the ROWS16
 *                                   instantiations, whose forward transforms load halves; the stash, the products, the inverse
 *                                   passes and the STFT phases are the fp32 time-domain form's.  `audiogoal` may be NULL.  Given a
 *                                   waveform buffer and n_valid <= kB (one rendered block) the step takes the half convolution +
 *                                   k_spectrogram, as the fp32 entry does (obs_rows_ok); that shape needs `audiogoal`.  Small steps
 *                                   run k_obs_blocks; captured into a graph on a reserved or warmed-up stream they may be
 *                                   replayed ("Captured steps").
 *   ss_audio_obs_logmel_rir16_f32   ss_audio_obs_logmel_f32 from half rows (k_conv<.., MEL, HALF>: loop-free when
 *                                   SS_FLAG_NO_DISTRACTOR and rir_cap <= kB, else the loop kernel): 257 <= out_len <= kB, the mel
 *                                   arguments and their limits as there; `audiogoal` and `spectrogram` may each be NULL, any
 *                                   combination is ONE launch.  Silent units, empty entries and pooled blocks behind n_valid give
 *                                   log(mel_eps), with exact zeros in the pooled spectrogram; a waveform buffer is written exactly
 *                                   as ss_audio_obs_rir16_f32 writes it.
 *   ss_audio_obs_logmel_rows_rir16_f32  the same for rows of 2 or 3 partition blocks (kB < out_len <= 3 kB, at most 16 RIR
 *                                   blocks): k_obs_blocks / k_obs_rows<.., MEL, .., ROWS16>, chosen by the rule of
 *                                   ss_audio_obs_rows_rir16_f32 (same stash, same hand-off area); a waveform buffer is written as
 *                                   that entry writes it.  Capture and replay: as that entry ("Captured steps").
 *                                   The results of both equal those of ss_audio_obs_logmel_f32 / _rows_f32 fed float(q) * rscale.
 * Length buckets: the section "Half-precision time-domain rows in length buckets" below (entries of their own).
 * Not served, by any entry: SS_FLAG_CROSSFADE (log-mel included), k_conv_rows, the wide form and the 512-thread core, the
 * TORCH_LIBRARY ops; no default selects the form, its row kernels or its log-mel forms.  The in-call loaders serve the two
 * single-allocation bindings (ss_ctx_set_rir_bank16 / _rows, given ss_miss_loader.stage_max), not the length-bucketed one.
 * SS_EINVAL before a device is touched: NULL halves or scales, a base that is not 4-byte aligned, odd rir_cap or rir_cap < 2, more
 * than 16 partition blocks, SS_FLAG_CROSSFADE, out_len outside the entry's range, a bad pad_mode, a NULL required output, mel
 * arguments outside the limits of ss_audio_features_f32.
 * n_units == 0 (n_entries == 0) returns 0. */
int ss_rir_rows16_f32(const float* rir, void* rir16_out, float* rscale_out, int n_entries, long long rir_unit_stride,
                      int rir_chan_stride, int rir_cap, void* stream);
int ss_fftconv_binaural_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len,
                                  const int* unit_desc, float* out, int n_units, int rir_cap, int n_valid, int out_len, int flags,
                                  void* stream);
int ss_audio_obs_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                           float* audiogoal, float* spectrogram, int n_units, int rir_cap, int n_valid, int out_len, int pad_mode,
                           int flags, void* stream);
int ss_audio_obs_rows_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                                float* audiogoal, float* spectrogram, int n_units, int rir_cap, int n_valid, int out_len,
                                int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                                  float* audiogoal, float* spectrogram, float* logmel, const int* mel_start, const float* mel_w,
                                  int n_mels, int max_len, float mel_eps, int n_units, int rir_cap, int n_valid, int out_len,
                                  int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_rows_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len,
                                       const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                       const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                       int rir_cap, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* The same for rows of 2 or 3 partition blocks (kB < out_len <= 3 kB: 44.1 / 48 kHz, the reference's Replica rate; EXTENSION):
 * the log-mel form of the fused row kernels (k_obs_rows / k_obs_blocks), the STFT phase behind every output block emits the
 * frames it completes.  Arguments and outputs as ss_audio_obs_logmel_f32 / _spec_f32 (which keep refusing rows longer than kB);
 * `audiogoal` and `spectrogram` may each be NULL and ANY combination of the three outputs is ONE launch - at this level the
 * caller chose the entry.  A waveform buffer is written exactly as ss_audio_obs_f32 / _spec_f32 write it on the same kernel.
 * Units that are silent or whose RIR is empty, and the frames of pooled blocks behind n_valid, come out as log(mel_eps) (exact
 * zeros in the pooled spectrogram).  Served shapes: kB < out_len <= 3 kB, 0 <= n_valid <= out_len, at most 16 RIR blocks
 * (rir_cap <= 16 kB / 1 <= h_blocks <= 16), no SS_FLAG_CROSSFADE, mel arguments under the limits above.  Everything else is
 * SS_EINVAL from the argument checks, before a device is touched.  The choice between the two kernels, the per-stream stash and
 * hand-off area are those of ss_audio_obs_f32 on such rows; like there, a launch that takes the one-workgroup-per-output-block
 * kernel (small steps: the whole grid fits the chip) may be captured on a reserved or warmed-up stream and replayed - its
 * hand-off flags then carry the replay's epoch ("Captured steps"). */
int ss_audio_obs_logmel_rows_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc,
                                 float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                 const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                 long long rir_unit_stride, int rir_chan_stride, int rir_elem_stride, int rir_cap, int n_valid,
                                 int out_len, int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_rows_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                                      float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                      const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int h_blocks,
                                      int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* SoundSpaces 2.0 steps (the reference's CONTINUOUS mode: 0.25 s of a 1-s row, cross-faded from the previous step's RIR in every
 * step but the first of an episode; EXTENSION): the log-mel form of the fused loop kernel with the cross-fade and / or its WIDE
 * form (only block 0 of a longer row is rendered).  Arguments and outputs as ss_audio_obs_logmel_f32, time-domain bank only (live
 * RIRs have no spectral form); `audiogoal` and `spectrogram` may each be NULL and ANY combination of the three outputs is ONE
 * launch, one workgroup per (unit, ear) row.  A waveform buffer and the pooled spectrogram are written exactly as
 * ss_audio_obs_f32 writes them on the same kernel.  Served shapes:
 *   (A) 257 <= out_len <= kB WITH SS_FLAG_CROSSFADE (term 1 of a unit = the previous RIR; units without one are not blended),
 *       0 <= n_valid <= out_len;
 *   (B) kB < out_len <= 3 kB, 0 <= n_valid <= kB and at most 26 live pooled blocks (44.1 / 48 kHz: n_valid = sr / 4), with or
 *       without SS_FLAG_CROSSFADE (then int(0.05 out_len) in [1, 2414]); without the flag distractor terms are fine.  The frames
 *       of pooled blocks behind the live ones come out as log(mel_eps), the spectrogram's columns there as zeros.
 * Any RIR length is accepted.  Silent units and units whose RIR is empty give log(mel_eps) in every band and exact zeros in the
 * pooled spectrogram.  Everything else - plain one-block rows (ss_audio_obs_logmel_f32), rows with more than one rendered block
 * (ss_audio_obs_logmel_rows_f32), mel arguments outside the limits above, a bad pad_mode - is SS_EINVAL from the argument
 * checks, before a device is touched. */
int ss_audio_obs_logmel_ss2_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc,
                                float* audiogoal, float* spectrogram, float* logmel, const int* mel_start, const float* mel_w,
                                int n_mels, int max_len, float mel_eps, int n_units, long long rir_unit_stride,
                                int rir_chan_stride, int rir_elem_stride, int rir_cap, int n_valid, int out_len, int pad_mode,
                                int flags, void* stream);

/* ---- Length-bucketed RIR bank ------------------------------------------------------------------------
 * The reference's RIRs are variable-length wav files (soundspaces/README.md:38-42, read at simulator.py:615-618; SS2.0's
 * ray-traced RIRs run to 4 s).  One capacity for every row means one long RIR reallocates the whole bank, multiplies the
 * HBM of every slot and pushes every launch off the loop-free kernel.  A bucketed bank keeps entries of similar length
 * together: bucket b holds bank indices [first, first + n_entries) as planar rows [n_entries, 2, cap] (zero beyond each
 * entry's length) in an allocation of its own, optionally with its spectral form (ss_rir_spectra_f32 of that bucket).
 * Buckets are ordered by `first` (bucket 0 starts at 0), ranges disjoint, at most 4; rir_len is ONE device array indexed by
 * the global bank index.  Unit descriptors are unchanged (they carry global indices).  Launches that promise
 * SS_FLAG_FIRST_BUCKET (and whose bucket 0 has cap <= kB) run the loop-free kernel. */
typedef struct ss_rir_bucket {
    const float* rir;     /* device, [n_entries, 2, cap] */
    const float* hspec;   /* device, [n_entries, 2, ceil(cap/kB), ss_spec_floats()] or NULL */
    int first;            /* global bank index of entry 0 of the bucket */
    int n_entries;
    int cap;              /* samples per (entry, ear) row, even */
    int reserved;
} ss_rir_bucket;
/* `buckets` is a HOST array of n_buckets descriptors.  The spectral kernels are used when every bucket carries hspec and
 * the launch is not cross-faded. */
int ss_fftconv_binaural_buckets_f32(const float* spec, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len,
                                    const int* unit_desc, float* out, int n_units, int n_valid, int out_len, int flags,
                                    void* stream);
int ss_audio_obs_buckets_f32(const float* spec, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len,
                             const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid,
                             int out_len, int pad_mode, int flags, void* stream);
/* Log-mel observation from a length-bucketed bank in ONE launch, no waveform buffer needed: outputs and mel arguments exactly
 * those of ss_audio_obs_logmel_f32 / ss_audio_obs_logmel_rows_f32 (logmel required; audiogoal and spectrogram may each be
 * NULL; any combination is one launch; a waveform buffer is written as ss_audio_obs_buckets_f32 writes it on the same kernel;
 * silent units and empty RIRs give log(mel_eps) in every band and exact zeros in the spectrogram).  Served: rows of one
 * partition block (257 <= out_len <= kB: k_conv / k_conv_spec <loop, MEL>) and rows of 2 or 3 blocks (kB < out_len <= 3 kB,
 * the deepest bucket at most 16 blocks: k_obs_blocks<.., MEL> while the grid fits the chip, k_obs_rows<.., BUCKETS, MEL>
 * beyond); spectral kernels when every bucket carries hspec, as above.  Launches that promise SS_FLAG_FIRST_BUCKET (or have one
 * bucket) are single-allocation launches on bucket 0 and equal ss_audio_obs_logmel_f32 / _spec_f32 / _rows_f32 / _rows_spec_f32
 * on its arrays bit for bit.  SS_EINVAL from the argument checks, before a device is touched: SS_FLAG_CROSSFADE, a bucket array
 * ss_audio_obs_buckets_f32 refuses, the mel limits of ss_audio_features_f32, a bad pad_mode, out_len < 257 or > 3 kB, n_valid
 * outside [0, out_len].  n_units == 0 returns 0. */
int ss_audio_obs_logmel_buckets_f32(const float* spec, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len,
                                    const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                    const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                    int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* ---- Spectral length buckets: a bucketed bank WITHOUT time-domain rows ------------------------------------------------------
 * The two dense forms of a bank - fp32 block spectra alone ("Spectral-only" binding of ss_ctx_set_rir_spectra) and the half form
 * ("Half-precision spectral bank") - for the length-bucketed store.  Bucket b holds bank indices [first, first + n_entries) in an
 * allocation of its own, in the per-bucket layout of the single-allocation forms:
 *   hspec   fp32: [n_entries, 2, ceil(cap/kB), ss_spec_floats()] floats, 16-byte aligned (ss_rir_spectra_f32 /
 *                 ss_bank_scatter_spectra_f32 of that bucket);
 *           half: the same count of fp16, 8-byte aligned (ss_rir_spectra16_f32 / ss_bank_scatter_spectra16_f32 of that bucket);
 *   hscale  half: [n_entries, 2, ceil(cap/kB)] floats, zero-initialised like the single-allocation bank's; fp32: NULL.
 * hscale NULL in every bucket = fp32, non-NULL in every bucket = half; a mixture is SS_EINVAL.  Block i of (entry r, ear ch) of
 * bucket b is block ((r - first_b) * 2 + ch) * ceil(cap_b/kB) + i of both arrays.  Ordering, count (<= 4), rir_len and the unit
 * descriptors as for ss_rir_bucket; a bucket has at most 16 blocks.  A half entry of bucket b costs 2 * h_blocks_b * (65 536 + 4)
 * + 4 bytes, an fp32 one 2 * h_blocks_b * 131 072 + 4 (ss_rir_bucket with both forms: three times the row bytes more).
 * Kernels: fp32 - the spectral kernels ss_*_buckets_f32 runs when every bucket carries hspec (they never read rows), results bit
 * for bit; half - k_conv_spec<.., HALF, HBK>, which resolves halves, scales and depth of a term's bucket from the wave-uniform
 * bank index.  Launches that promise SS_FLAG_FIRST_BUCKET (or have one bucket) are single-allocation launches on bucket 0 and
 * keep the loop-free kernels.
 *   ss_fftconv_binaural_spec_buckets_f32   every row length ss_fftconv_binaural_spec_f32 / _spec16_f32 serve (n_valid <= 3 kB);
 *   ss_audio_obs_spec_buckets_f32          fp32: the shapes ss_audio_obs_buckets_f32 serves from spectra; half: rows of one
 *                                          partition block, 257 <= out_len <= kB (rows of 2 or 3 blocks: the entries of their own
 *                                          below, ss_audio_obs_rows_spec16_buckets_f32);
 *   ss_audio_obs_logmel_spec_buckets_f32   ss_audio_obs_logmel_buckets_f32 on these buckets, same outputs, shapes and refusals:
 *                                          fp32 - one-block rows (k_conv_spec<loop, MEL>) and rows of 2 or 3 blocks (k_obs_blocks /
 *                                          k_obs_rows <true, .., BUCKETS, MEL>); half - one-block rows only
 *                                          (k_conv_spec<.., MEL, HALF, HBK>), out_len > kB is SS_EINVAL.
 * SS_EINVAL from the argument checks, before a device is touched: a NULL or misaligned hspec, mixed forms, more than 4 buckets,
 * `first` not ascending / overlapping / != 0 for bucket 0, an odd cap or cap < 2, a bucket of more than 16 blocks,
 * SS_FLAG_CROSSFADE, half with out_len > kB in the fused entries.  n_units == 0 returns 0. */
typedef struct ss_spec_bucket {
    const void*  hspec;   /* device; see above */
    const float* hscale;  /* device, or NULL (fp32) */
    int first;            /* global bank index of entry 0 of the bucket */
    int n_entries;
    int cap;              /* samples per (entry, ear) row the spectra cover, even */
    int reserved;
} ss_spec_bucket;
int ss_fftconv_binaural_spec_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                         const int* unit_desc, float* out, int n_units, int n_valid, int out_len, int flags,
                                         void* stream);
int ss_audio_obs_spec_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                  const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid,
                                  int out_len, int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_spec_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                         const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                         const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps,
                                         int n_units, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* ---- Half spectral length buckets, rows of 2 or 3 partition blocks (44.1 / 48 kHz) -------------------------------------------
 * The two fused entries above refuse half buckets with out_len > kB; these two serve exactly that: HALF ss_spec_bucket[] arrays
 * (hscale non-NULL in every bucket), kB < out_len <= 3 kB, 0 <= n_valid <= out_len, every bucket at most 16 blocks.  Arguments
 * as their single-allocation siblings ss_audio_obs_rows_spec16_f32 / ss_audio_obs_logmel_rows_spec16_f32 take them, with
 * (buckets, n_buckets) in place of (hspec16, hscale, h_blocks), and routed as those route: k_obs_blocks<true, MEL, HALF, HBK>
 * while rows x blocks fit the chip at one workgroup per CU and n_valid == out_len, k_obs_rows<true, false, BUCKETS, MEL, HALF>
 * beyond - both resolve halves, scales and depth of a term's bucket once per term from the wave-uniform bank index
 * (nbh = min(ceil(rir_len / kB), the bucket's blocks)); shapes the fp32 entry renders unfused (n_valid <= kB with a waveform
 * buffer) go to ss_fftconv_binaural_spec_buckets_f32 + the spectrogram kernel.
 *   ss_audio_obs_rows_spec16_buckets_f32          audiogoal may be NULL, spectrogram required;
 *   ss_audio_obs_logmel_rows_spec16_buckets_f32   logmel required (the mel limits of ss_audio_features_f32), audiogoal and
 *                                                 spectrogram optional, any combination in one launch.
 * Launches with one bucket or SS_FLAG_FIRST_BUCKET are single-allocation launches on bucket 0: bit for bit what the siblings
 * give on its arrays.  Values: those of the fp32 spectral buckets fed float(q) * hscale, to the rounding of the products' order.
 * SS_EINVAL before a device is touched: fp32 or mixed buckets, every refusal of ss_spec_bucket, SS_FLAG_CROSSFADE, out_len <= kB
 * or > 3 kB, n_valid outside [0, out_len], a bad pad_mode, a NULL required output.  n_units == 0 returns 0.  Capture and
 * replay: "Captured steps" (see ss_audio_obs_rows_spec16_f32). */
int ss_audio_obs_rows_spec16_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                         const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid,
                                         int out_len, int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_rows_spec16_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                                const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                                const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps,
                                                int n_units, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* ---- Half-precision time-domain rows in length buckets (EXTENSION, opt-in, LOSSY) ------------------------------------------------
 * The two capacity levers of a bank together: the half rows of "Half-precision time-domain rows" (same format, same quantiser, same
 * loss - a property of the per-row rule, independent of the bucket: 1.7-2.3e-4 of peak on the waveform, measured there) kept in the
 * length buckets of ss_rir_bucket.  Bucket b holds bank indices [first, first + n_entries) in two allocations of its own: rir16
 * [n_entries, 2, cap_b] halves and rscale [n_entries, 2] floats, both zero-initialised (ss_rir_rows16_f32 /
 * ss_bank_scatter_rows16_f32 of that bucket).  An entry of bucket b costs 4 * cap_b + 8 bytes.  Rows are NOT padded to whole
 * partition blocks: the halves behind a row's capacity are the next entry's, and the kernel takes a row's stride and its load bound
 * from the row's own bucket.  Ordering (`first` ascending, bucket 0 at index 0, disjoint ranges), count (1 to 4), rir_len (ONE device
 * array over global indices) and the unit descriptors as for ss_rir_bucket; `buckets` is a HOST array, copied where it is kept.
 * Each bucket must pass the checks of the single-allocation form: non-NULL 4-byte aligned halves, non-NULL scales, an even cap >= 2
 * of at most 16 partition blocks.
 * Kernel: k_conv<.., HALF, RBK> (the loop kernel), which resolves halves, scales, stride and capacity of a term's bucket from the
 * wave-uniform bank index with scalar compares; results equal those of ss_*_buckets_f32 fed float(q) * rscale.  Launches that promise
 * SS_FLAG_FIRST_BUCKET (or have one bucket) are single-allocation launches on bucket 0's arrays - with cap_0 <= kB the loop-free
 * half kernels - and equal ss_fftconv_binaural_rir16_f32 / ss_audio_obs_rir16_f32 on them bit for bit.
 *   ss_fftconv_binaural_rir16_buckets_f32   every shape ss_fftconv_binaural_rir16_f32 serves;
 *   ss_audio_obs_rir16_buckets_f32          the shapes of ss_audio_obs_rir16_f32: 257 <= out_len <= kB, at most 26 pooled blocks,
 *                                           `audiogoal` may be NULL.  Longer rows: the convolution entry + ss_spectrogram_f32 (what
 *                                           a context bound by ss_ctx_set_rir16_buckets does).
 *   ss_audio_obs_logmel_rir16_buckets_f32   ss_audio_obs_logmel_rir16_f32 on the buckets: one-block rows only (257 <= out_len <= kB;
 *                                           longer rows are SS_EINVAL), ONE launch for any combination of `audiogoal` and
 *                                           `spectrogram` (each may be NULL): k_conv<.., MEL, HALF, RBK>; bucket-0 launches run the
 *                                           single-allocation log-mel kernels on bucket 0's arrays (loop-free with cap_0 <= kB and
 *                                           SS_FLAG_NO_DISTRACTOR) and equal ss_audio_obs_logmel_rir16_f32 on them bit for bit.
 * OUT OF SCOPE, refused or not offered: bucketed half rows under the fused row kernels (k_obs_blocks / k_obs_rows keep reading one
 * allocation of half rows only - log-mel included), SS_FLAG_CROSSFADE, the wide form, k_conv_rows, the 512-thread core, the
 * in-call loaders, the TORCH_LIBRARY ops; no default selects the form.
 * SS_EINVAL before a device is touched: a NULL bucket array, n_buckets outside [1, 4], any bucket the single-allocation checks
 * refuse, `first` not ascending / overlapping / != 0 for bucket 0, negative n_entries, NULL rir_len, SS_FLAG_CROSSFADE, out_len
 * outside the entry's range, a bad pad_mode, a NULL required output.  n_units == 0 returns 0. */
typedef struct ss_rir16_bucket {
    const void*  rir16;   /* device, [n_entries, 2, cap] halves, planar, 4-byte aligned, zero-initialised */
    const float* rscale;  /* device, [n_entries, 2], zero-initialised */
    int first;            /* global bank index of entry 0 of the bucket */
    int n_entries;
    int cap;              /* samples per (entry, ear) row, even */
    int reserved;
} ss_rir16_bucket;
int ss_fftconv_binaural_rir16_buckets_f32(const float* spec, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len,
                                          const int* unit_desc, float* out, int n_units, int n_valid, int out_len, int flags,
                                          void* stream);
int ss_audio_obs_rir16_buckets_f32(const float* spec, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len,
                                   const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid,
                                   int out_len, int pad_mode, int flags, void* stream);
int ss_audio_obs_logmel_rir16_buckets_f32(const float* spec, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len,
                                          const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                          const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps,
                                          int n_units, int n_valid, int out_len, int pad_mode, int flags, void* stream);

/* EXTENSION, one pass for every STFT-derived feature (BASELINE.json configs[4] "GCC-PHAT + log-mel fused sensor"): each
 * (unit, ear, frame) of x [n_units, 2, len] is framed, windowed and transformed ONCE (both ears in one wave), and from that
 * one spectrum the kernel writes any subset of
 *   spectrogram [n_units, 65, T4, 2]            as ss_spectrogram_f32 (the reference's compute_spectrogram, nav.py:86-100)
 *   logmel      [n_units, n_mels, T, 2]         as ss_logmel_f32  (n_mels <= 64; larger banks: ss_logmel_f32)
 *   gccphat     [n_units, 2*max_lag+1, T]       as ss_gccphat_f32
 * (NULL = not wanted; at least one).  Same arguments and results as the three stand-alone entry points, which each re-read
 * the waveform and redo the STFT: any len >= 1, reflect padding as np.pad at every length (see ss_spectrogram_f32),
 * 1 <= n_mels <= 64, 1 <= max_lag <= 32, both eps > 0; SS_EINVAL outside. */
int ss_audio_features_f32(const float* x, int n_units, int len, int pad_mode, float* spectrogram, float* logmel,
                          const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps,
                          float* gccphat, int max_lag, float gcc_eps, void* stream);

/* ---- The loop-free case on the 512-thread FFT core (round 4; csrc/ss_fft_core32.hpp) ------------------------------------
 * Rows of ONE partition block from a time-domain bank of rir_cap <= kB, no distractor / cross-fade terms - SoundSpaces 1.0
 * with 1-s clips (simulator.py:629-632) - on a 512-thread / 32-values-per-thread transform (16384 = 32*32*16: two LDS
 * exchanges per transform instead of three, half the workgroup barriers).  Window spectra for it come from
 * ss_source_windows32_f32 (same descriptors and size as ss_source_windows_f32, that core's own register order: the two
 * formats are not interchangeable).  audiogoal or spectrogram may be NULL (not both).  Results equal ss_audio_obs_f32's to
 * fp32 rounding.  Measured A/B against the 1024-thread kernels: profiles/r4/NOTES.md section 1. */
int ss_source_windows32_f32(const float* src, const int* win_desc, float* spec_out, int n_windows, void* stream);
int ss_audio_obs32_f32(const float* spec32, const float* rir, const int* rir_len, const int* unit_desc, float* audiogoal,
                       float* spectrogram, int n_units, long long rir_unit_stride, int rir_chan_stride, int rir_elem_stride,
                       int rir_cap, int n_valid, int out_len, int pad_mode, void* stream);

/* av_wan Intensity sensor (ss_baselines/av_wan/avwan_sensors.py:91-100) on audiogoal [n_units, 2, len]:
 * onset = min over ears of the first sample > 0.1*max, out[n] = mean(x[:, onset:onset+num_frame]**2) over the samples that
 * exist (rows may be shorter than num_frame).  len >= 1, num_frame >= 1. */
int ss_intensity_f32(const float* audiogoal, float* out, int n_units, int len, int num_frame, void* stream);

/* EXTENSION (no counterpart in the reference; BASELINE.json north_star "log-mel"): log-mel spectrogram of
 * x [n_units, 2, len] -> out [n_units, n_mels, 1 + len/160, 2] (channel-last, no pooling):
 *   out = log( sum_k W[j][k] * |STFT(x)[k]|^2 + eps ), STFT framing exactly as ss_spectrogram_f32.
 * The filter bank is band-sparse: band j covers bins mel_start[j] .. mel_start[j] + max_len - 1 with weights
 * mel_w[j*max_len + i] (zero padded).  1 <= n_mels <= 128; eps > 0; any len >= 1 (reflect padding as np.pad at every length,
 * see ss_spectrogram_f32); max_len a multiple of 4, <= 64 (32 bands at 48 kHz; 20-band banks are wider); n_mels*max_len <= 4096;
 * mel_start[j] a multiple of 4 in [0, 256] (pad the band with leading zero weights; the kernel reads 16 bytes at a
 * time and sees zeros beyond bin 256); mel_w 16-byte aligned.  mel_start's range is the caller's responsibility. */
int ss_logmel_f32(const float* x, float* out, int n_units, int len, int pad_mode, const int* mel_start,
                  const float* mel_w, int n_mels, int max_len, float eps, void* stream);

/* EXTENSION (no counterpart in the reference; BASELINE.json configs[4] "GCC-PHAT"): generalised cross-correlation
 * with phase transform between the two ears, per STFT frame (framing exactly as ss_spectrogram_f32):
 *   G[k] = X_left[k] conj(X_right[k]);  g = irfft(G / (|G| + eps), 512);  out[n][i][t] = g[(i - max_lag) mod 512]
 * x [n_units, 2, len] -> out [n_units, 2*max_lag + 1, 1 + len/160].  1 <= max_lag <= 32 (0 and 33: SS_EINVAL), eps > 0,
 * any len >= 1 (reflect padding as np.pad at every length, see ss_spectrogram_f32). */
int ss_gccphat_f32(const float* x, float* out, int n_units, int len, int pad_mode, int max_lag, float eps,
                   void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Context API: the self-contained entry.  One call per vector step does what the reference does per env
 * in Python -- SoundSpacesSim._compute_audiogoal (soundspaces/simulator.py:608-666) /
 * ContinuousSoundSpacesSim._compute_audiogoal + _convolve_with_rir (soundspaces/continuous_simulator.py:413-456) and
 * SpectrogramSensor.compute_spectrogram (soundspaces/tasks/nav.py:86-100) -- for ALL envs: the caller hands over what a
 * simulator knows (which sound, which clip window, which RIR), the library plans the partitions, keeps the
 * source-window spectra it needs in a bounded cache, uploads the descriptors and launches.  A C caller therefore needs
 * neither ss_amd/planning.py nor the opaque spectrum slots of the entry points above.
 *
 * A context is bound to the HIP device that is current when it is created.  Calls must come from one host thread at a time;
 * consecutive calls may name different streams (the library orders the shared window-spectra pool between them: on a
 * stream change it records an event on the PREVIOUS call's stream, so a stream handed to ss_ctx_observe must stay alive
 * until a later call on another stream has returned, or the context is destroyed), and ss_ctx_set_overlap lets the library
 * alternate two internal streams itself.  hipStreamPerThread is not accepted for rows longer than one block (one handle,
 * a different stream per thread).  ss_ctx_plan is a planner-only / test entry: after it the next ss_ctx_observe synchronises
 * the device and starts from an empty window cache.
 * ---------------------------------------------------------------------------------------------------------------*/
typedef struct ss_ctx ss_ctx;

/* The units of one step, struct-of-arrays, HOST memory, n entries per column; optional columns may be NULL.
 * unit i:  out[c,t] = sum_k rir[c,k] * x[t0 + t - k], t < n_valid (rest of the 1-s row zero), x = clip `sound`,
 *   x[<0] = 0 and past the clip end 0 or -- contexts created with wrap_mode 1, units with wrap != 0 -- the clip again
 *   from its start (the reference wraps only in its steady branch, continuous_simulator.py:438-447).
 *   t0 per reference branch: 0 (1-s clip, simulator.py:629-632); _audio_index * sr (multi-second, :634-647);
 *   _current_sample_index (continuous_simulator.py:432).
 *   rir < 0: silent unit (simulator.py:610-612) -> exact zeros.
 *   dis_sound / dis_rir: distractor (whole clip through a second RIR, added; simulator.py:649-664), -1 = none.
 *   last_rir: the previous step's RIR for SS2.0 CROSSFADE (see SS_FLAG_CROSSFADE), -1 = none; last_wrap = the branch
 *   flag of THAT RIR (defaults to wrap).  A step has either distractors or cross-fades, not both. */
typedef struct ss_units {
    const int* sound;
    const int* t0;
    const int* rir;
    const int* dis_sound;            /* optional */
    const int* dis_rir;              /* optional */
    const int* last_rir;             /* optional */
    const unsigned char* wrap;       /* optional; NULL = 1 for every unit */
    const unsigned char* last_wrap;  /* optional; NULL = same as wrap */
} ss_units;

/* n_valid = samples computed per row: sampling_rate (SoundSpacesSim) or int(sampling_rate * STEP_TIME) (Continuous);
 * rows are sampling_rate long.  wrap_mode: 0 = SoundSpaces 1.0, 1 = SoundSpaces 2.0 semantics (see ss_units).
 * max_window_sets = initial capacity of the window-spectra cache in (sound, t0) keys (128 KiB of HBM per stored
 * window; <= 0: 256); the cache is LRU and only grows when one step itself needs more keys than it holds. */
int ss_ctx_create(ss_ctx** ctx, int sampling_rate, int n_valid, int pad_mode, int wrap_mode, int max_window_sets);
int ss_ctx_destroy(ss_ctx* ctx);
/* Register a mono clip, float32, already at the simulator rate (the reference's _source_sound_dict,
 * simulator.py:595-600).  `clip` is host memory (on_device = 0) or device memory.  Returns the sound id >= 0. */
int ss_ctx_add_source(ss_ctx* ctx, const float* clip, int len, int on_device);
int ss_ctx_add_source_len(ss_ctx* ctx, int len);   /* planner-only registration (no device memory; for ss_ctx_plan) */
/* RIR bank in device memory, addressing as for ss_fftconv_binaural_f32; the pointers are borrowed. */
int ss_ctx_set_rir_bank(ss_ctx* ctx, const float* rir, const int* rir_len, long long rir_unit_stride,
                        int rir_chan_stride, int rir_elem_stride, int rir_cap);
/* Optional spectral form (ss_rir_spectra_f32) of the bank given to ss_ctx_set_rir_bank: steps without a cross-fade then
 * run the *_spec_* kernels.  hspec = NULL: back to the time-domain kernels.  Borrowed pointer.
 * SPECTRAL-ONLY binding (a bank that keeps no time-domain rows, filled by ss_bank_scatter_spectra_f32):
 *   ss_ctx_set_rir_bank(ctx, NULL, rir_len, 0, 0, 1, rir_cap);  ss_ctx_set_rir_spectra(ctx, hspec, ceil(rir_cap / kB));
 * Steps then always read the spectra; a step whose route reads time-domain rows (a cross-fade) is refused with SS_EINVAL
 * before any upload or launch.  The in-call loaders (ss_miss_loader with bank = NULL, stage_desc not needed) write the
 * new rows' spectra and lengths with one k_stage_spectra launch. */
int ss_ctx_set_rir_spectra(ss_ctx* ctx, const float* hspec, int h_blocks);
/* The same binding for a HALF bank ("Half-precision spectral bank" above): spectral-only, so
 *   ss_ctx_set_rir_bank(ctx, NULL, rir_len, 0, 0, 1, rir_cap);  ss_ctx_set_rir_spectra16(ctx, hspec16, hscale, ceil(rir_cap / kB));
 * Steps then take the three *_spec16_* entries (ss_ctx_observe_features' one-launch log-mel route and the unit-count policies as
 * they stand).  SS_EINVAL, nothing changed: a context whose rows exceed kB (sampling_rate > kB), a bank that keeps time-domain
 * rows or length buckets, fp32 spectra already bound (and ss_ctx_set_rir_spectra while a half bank is bound): one form at a time.
 * A cross-faded step is refused like on every spectral-only bank.  hspec16 = NULL unbinds.  The in-call loaders
 * (ss_ctx_observe_requests_load, ss_ctx_load_rir_files) serve such a context through ss_bank_scatter_spectra16_f32; the
 * ss_miss_loader of a spectral-only store is used as it is (bank = NULL). */
int ss_ctx_set_rir_spectra16(ss_ctx* ctx, const void* hspec16, const float* hscale, int h_blocks);
/* ... and for contexts whose rows have 2 or 3 partition blocks (kB < sampling_rate <= 3 kB: 44.1 / 48 kHz), which the call above
 * keeps refusing: the same preconditions otherwise (spectral-only bank, no buckets, rir_len set, no fp32 spectra bound,
 * h_blocks == ceil(rir_cap / kB) <= 16), SS_EINVAL on a context of one-block rows.  Spectrogram steps (with or without a
 * waveform buffer) then take ss_audio_obs_rows_spec16_f32, log-mel steps inside ss_ctx_set_logmel_rows_policy's range
 * ss_audio_obs_logmel_rows_spec16_f32 (outside it: the context's waveform scratch, as always), waveform-only steps
 * ss_fftconv_binaural_spec16_f32.  Cross-faded steps are SS_EINVAL and leave no keys behind.  hspec16 = NULL unbinds.  The
 * in-call loaders serve the binding through ss_bank_scatter_spectra16_f32. */
int ss_ctx_set_rir_spectra16_rows(ss_ctx* ctx, const void* hspec16, const float* hscale, int h_blocks);
/* Half-precision time-domain rows as the context's bank ("Half-precision time-domain rows" above).  Replaces ANY earlier binding
 * and is replaced by every other bank call; while it is bound ss_ctx_set_rir_spectra / _spectra16 / _spectra16_rows with a bank are
 * SS_EINVAL.  rir16 = NULL unbinds.  Steps of one-block rows (257 <= sampling_rate <= kB) take the fused half kernels, every longer
 * row (44.1 / 48 kHz) the half convolution into the caller's waveform buffer - or the context's hand-over buffer - and the
 * spectrogram kernel over it; log-mel steps render into the context's waveform scratch unless ss_ctx_set_logmel_rir16_policy
 * admits them to the one-launch form (one-block rows on this binding).  A cross-faded step is SS_EINVAL and
 * leaves no keys behind.  The in-call loaders (ss_ctx_load_rir_files, ss_ctx_observe_requests_load) serve this binding when the
 * ss_miss_loader lends no rows (bank = NULL), a pinned block for the rows' maxima (stage_max != NULL) and cap == rir_cap: the files'
 * maxima are taken by the reader, ONE launch (k_scatter_rows16_max) writes halves, scales and lengths of the new entries, and the
 * books are kept exactly as for a bank of fp32 rows (free stack, LRU eviction, host_len, clipped, the reports, the order behind
 * steps in flight in overlap mode).  Without stage_max, or with another cap, the answers are those of a form that is not served:
 * ss_ctx_load_rir_files returns 1, ss_ctx_observe_requests_load reports the misses (the caller scatters with
 * ss_bank_scatter_rows16_f32 and calls again); nothing is changed.  The pose
 * memo, the overlap mode and the column / request entries run on it unchanged.  SS_EINVAL, nothing changed: the bank refusals of
 * the stateless entries, rir_len == NULL. */
int ss_ctx_set_rir_bank16(ss_ctx* ctx, const void* rir16, const float* rscale, const int* rir_len, int rir_cap);
/* The same binding, opted in to the fused row kernels (EXTENSION): ss_ctx_set_rir_bank16 in every respect - replace and unbind
 * rules, refusals, loaders, pose memo, overlap mode, column / request entries - except that steps of rows of 2 or 3 partition
 * blocks (44.1 / 48 kHz) take ONE launch (k_obs_blocks / k_obs_rows<.., ROWS16>, what ss_audio_obs_rows_rir16_f32 runs) wherever the
 * fp32 time-domain bank would: not with a waveform buffer and one rendered block (n_valid <= kB), not past 3 kB samples - those keep
 * the two launches.  A spectrogram-only step then needs no hand-over buffer.  Log-mel steps inside
 * ss_ctx_set_logmel_rir16_policy's range (empty by default) take ss_audio_obs_logmel_rir16_f32 / _rows_rir16_f32; the others keep
 * the waveform scratch: with a spectrogram asked as well and n_valid > kB, the row
 * kernel writes the scratch and the spectrogram and the feature kernel runs over the scratch.  One-block rates: the same routes
 * as ss_ctx_set_rir_bank16.  A later ss_ctx_set_rir_bank16 on the context clears the opt-in. */
int ss_ctx_set_rir_bank16_rows(ss_ctx* ctx, const void* rir16, const float* rscale, const int* rir_len, int rir_cap);
/* The bank as length buckets (see ss_rir_bucket; replaces the two calls above for such banks; the descriptor array is copied,
 * the device pointers are borrowed).  Call again whenever a bucket is (re)allocated. */
int ss_ctx_set_rir_buckets(ss_ctx* ctx, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len);
/* The bank as spectral length buckets (see ss_spec_bucket), either form.  Replaces ANY earlier binding - rows, spectra of either
 * form, ss_rir_bucket buckets - and is replaced by ss_ctx_set_rir_bank / ss_ctx_set_rir_buckets; while it is bound,
 * ss_ctx_set_rir_spectra / _spectra16 / _spectra16_rows with a bank are SS_EINVAL: one form at a time.  Planning depth is the
 * longest bucket's blocks, as for ss_ctx_set_rir_buckets; steps whose units all sit in bucket 0 keep the loop-free kernels.
 * SS_EINVAL, nothing changed: the refusals of ss_spec_bucket, rir_len == NULL, half buckets on a context whose rows exceed kB.
 * A cross-faded step is SS_EINVAL and leaves no keys behind, as on every spectral-only bank; log-mel steps render into the
 * context's waveform scratch and run the feature kernel over it, as on ss_ctx_set_rir_buckets contexts, unless
 * ss_ctx_set_logmel_buckets_policy admits them to the one-launch route.  The in-call loaders are
 * not extended and load nothing on such a context: ss_ctx_load_rir_files returns 1 ("not served", nothing changed);
 * ss_ctx_observe_requests_load returns 0 with the unresolved requests reported in miss_out / n_miss and no launch made, as
 * ss_ctx_observe_requests reports them (a step without misses is rendered).  Call again whenever a bucket is (re)allocated. */
int ss_ctx_set_rir_spec_buckets(ss_ctx* ctx, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len);
/* HALF spectral length buckets on a context whose rows are 2 or 3 partition blocks (kB < sampling_rate <= 3 kB: 44.1 / 48 kHz).
 * Preconditions, replacement rules and the loaders' "not served" as ss_ctx_set_rir_spec_buckets; on top, SS_EINVAL (nothing
 * changed) for fp32 buckets and on a context of one-block rows.  Spectrogram steps take ss_audio_obs_rows_spec16_buckets_f32,
 * log-mel steps inside ss_ctx_set_logmel_buckets_policy's range ss_audio_obs_logmel_rows_spec16_buckets_f32 (outside it: the
 * context's waveform scratch, as always), waveform-only steps ss_fftconv_binaural_spec_buckets_f32.  Cross-faded steps are
 * SS_EINVAL and leave no keys behind. */
int ss_ctx_set_rir_spec_buckets_rows(ss_ctx* ctx, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len);
/* Half-precision time-domain rows in length buckets as the context's bank (see ss_rir16_bucket).  Replaces ANY earlier binding and
 * is replaced by every other bank call; buckets = NULL unbinds; while it is bound ss_ctx_set_rir_spectra / _spectra16 /
 * _spectra16_rows with a bank are SS_EINVAL.  Planning depth is the deepest bucket's blocks, as for ss_ctx_set_rir_buckets; steps
 * whose units all sit in bucket 0 carry SS_FLAG_FIRST_BUCKET and keep the loop-free half kernels.  Routes as ss_ctx_set_rir_bank16:
 * one-block rows take the fused launch, longer rows (44.1 / 48 kHz) the bucketed half convolution into the caller's waveform buffer
 * - or the context's hand-over buffer - and the spectrogram kernel over it (never the fused row kernels), log-mel steps the waveform
 * scratch - or, one-block rows inside ss_ctx_set_logmel_rir16_policy's range, ss_audio_obs_logmel_rir16_buckets_f32.  A cross-faded step is SS_EINVAL and leaves no keys behind.  The in-call loaders do not serve this form:
 * ss_ctx_load_rir_files returns 1, ss_ctx_observe_requests_load reports the misses and launches nothing.  The pose memo, the overlap
 * mode and the column / request entries run on it unchanged.  SS_EINVAL, nothing changed: the refusals of ss_rir16_bucket,
 * rir_len == NULL.  Call again whenever a bucket is (re)allocated. */
int ss_ctx_set_rir16_buckets(ss_ctx* ctx, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len);
/* One step.  audiogoal [n,2,sr] and spectrogram [n,65,T4,2] are device buffers; either may be NULL (not both).
 * Asynchronous on `stream`; the host arrays of `units` may be reused as soon as the call returns. */
int ss_ctx_observe(ss_ctx* ctx, const ss_units* units, int n, float* audiogoal, float* spectrogram, void* stream);
/* One step plus its STFT-derived extension features (BASELINE.json configs[4]: savi, "GCC-PHAT + log-mel fused sensor"): as
 * ss_ctx_observe, then ss_audio_features_f32 over the step's waveform on the SAME stream (in overlap mode: the same internal
 * lane), so the features need no join of their own.  logmel / gccphat of `f` may each be NULL (not both).  With an audiogoal
 * buffer and a spectrogram asked for as well, the spectrogram is pooled by the feature kernel (which holds every frame's
 * spectrum of both ears anyway) and the convolution launch runs without its fused STFT phase: 96.5 instead of 108 us per
 * 256-env savi step.
 * audiogoal == NULL is accepted for log-mel without GCC-PHAT (f->logmel != NULL, f->gccphat == NULL; GCC-PHAT reads both ears'
 * waveform and stays SS_EINVAL without a buffer); spectrogram may then be NULL too.  Such a step takes
 *   - ONE fused launch (ss_audio_obs_logmel_f32 / _spec_f32; no waveform anywhere) when its rows are one partition block
 *     (257 <= sr <= kB: 16 kHz), the step has no cross-fade, the bank is a single allocation of either form (also the
 *     spectral-only binding) and its unit count lies inside ss_ctx_set_logmel_policy's range;
 *   - ONE fused launch as well (ss_audio_obs_logmel_rows_f32 / _spec_f32) when its rows are 2 or 3 partition blocks (44.1 /
 *     48 kHz), under the same conditions, and its unit count lies inside ss_ctx_set_logmel_rows_policy's range - which is empty
 *     by default: the fused values equal the next route's to rounding (1e-4 of the largest value), not bit for bit;
 *   - ONE fused launch (ss_audio_obs_logmel_ss2_f32) when it is a SoundSpaces 2.0 step - a cross-faded step of one-block rows,
 *     or a step that renders only block 0 of a 44.1 / 48 kHz row, cross-faded or not - on the time-domain rows of a
 *     single-allocation bank (not the spectral-only binding) and its unit count lies inside ss_ctx_set_logmel_ss2_policy's
 *     range, which is empty by default for the same reason;
 *   - ONE fused launch (ss_audio_obs_logmel_buckets_f32 / _spec_buckets_f32) on a context bound by ss_ctx_set_rir_buckets or
 *     ss_ctx_set_rir_spec_buckets, when the step has no cross-fade, its rows are one partition block (every bank form) or 2 or
 *     3 blocks (the fp32 forms) and its unit count lies inside ss_ctx_set_logmel_buckets_policy's range, which is empty by
 *     default for the same reason; the three ranges above never apply to such a context;
 *   - ONE fused launch (ss_audio_obs_logmel_rir16_f32 / _rows_rir16_f32 / _rir16_buckets_f32) on a context bound by
 *     ss_ctx_set_rir_bank16, ss_ctx_set_rir_bank16_rows or ss_ctx_set_rir16_buckets, when the step has no cross-fade, its rows are
 *     one partition block (all three bindings) or 2 or 3 blocks (ss_ctx_set_rir_bank16_rows only) and its unit count lies inside
 *     ss_ctx_set_logmel_rir16_policy's range, which is empty by default for the same reason; the four ranges above never apply
 *     to such a context;
 *   - otherwise (44.1 / 48 kHz rows, cross-faded steps and bucketed banks by default, unit counts outside the range) the route ss_ctx_observe
 *     takes with an audiogoal buffer, into a waveform scratch the CONTEXT owns ([n, 2, sr] floats per overlap lane, grown on
 *     demand, freed with the context and by ss_release_scratch; a growth needed while the stream is being captured is refused
 *     with SS_EINVAL: warm the stream up first), then ss_audio_features_f32 over it: bit for bit ss_ctx_observe +
 *     ss_audio_features_f32.
 * Calls that pass an audiogoal buffer take exactly the route described first. */
typedef struct ss_features {
    float* logmel;            /* [n, n_mels, 1 + sr/160, 2] or NULL */
    const int* mel_start;     /* device, [n_mels]          (ss_logmel_f32's band-sparse filter bank) */
    const float* mel_w;       /* device, [n_mels, max_len] */
    int n_mels, max_len;
    float mel_eps;
    float* gccphat;           /* [n, 2*max_lag+1, 1 + sr/160] or NULL */
    int max_lag;
    float gcc_eps;
} ss_features;
int ss_ctx_observe_features(ss_ctx* ctx, const ss_units* units, int n, float* audiogoal, float* spectrogram,
                            const ss_features* f, void* stream);
/* Which log-mel steps without a waveform buffer take the fused launch: those of min_units <= n <= max_units units (and a shape
 * it serves, see above).  Default: the range in which the fused launch measured faster than the two launches it replaces
 * (profiles/r7/kbench_obs_logmel.txt).  (1, INT_MAX): whenever the shape allows; max_units < min_units: never. */
int ss_ctx_set_logmel_policy(ss_ctx* ctx, int min_units, int max_units);
/* The same for rows of 2 or 3 partition blocks (44.1 / 48 kHz).  ss_ctx_set_logmel_policy keeps its meaning (one-block rows
 * only).  Default: never (max_units < min_units) - see above; profiles/r7/NOTES.md names the range the measurements support. */
int ss_ctx_set_logmel_rows_policy(ss_ctx* ctx, int min_units, int max_units);
/* The same for SoundSpaces 2.0 steps (ss_audio_obs_logmel_ss2_f32's shapes); the two setters above keep their meaning.  Default:
 * never (max_units < min_units) - the fused values equal the scratch route's to rounding only.  Measured faster than the
 * scratch route of the same context at every point of 1 .. 256 units (16 kHz cross-faded, 44.1 kHz cross-faded and plain; RIRs
 * of 9000 taps: 19-58 %, of 4 s: 5-33 %; profiles/r7/kbench_obs_logmel_ss2.txt), so (1, INT_MAX) is the range a caller who
 * accepts rounding-level differences would pass. */
int ss_ctx_set_logmel_ss2_policy(ss_ctx* ctx, int min_units, int max_units);
/* The same for contexts bound by ss_ctx_set_rir_buckets / ss_ctx_set_rir_spec_buckets (ss_audio_obs_logmel_buckets_f32 /
 * _spec_buckets_f32 and their shapes); the three setters above keep their meaning and never apply to such a context.  The pool,
 * the planner's SS_FLAG_FIRST_BUCKET and the step's flags pass through unchanged; cross-faded steps keep the scratch route.
 * Default: never (max_units < min_units) - the fused values equal the scratch route's to rounding only.  Measured against the
 * scratch route of the same context on a mixed-bucket step (profiles/r7/kbench_obs_logmel_buckets.txt): 16 kHz, every bank form,
 * 1 .. 128 units: 9-41 % faster, so (1, INT_MAX) is the range a caller would pass there; 44.1 kHz: faster up to 42 units and
 * whenever the spectrogram is asked for as well (8-29 %), but log-mel alone at 43 units costs 1.7 x the scratch route (the row
 * kernel takes over from the one-workgroup-per-block kernel) and 128 units are a tie: (1, 42) there. */
int ss_ctx_set_logmel_buckets_policy(ss_ctx* ctx, int min_units, int max_units);
/* The same for contexts bound to half-precision time-domain rows (ss_ctx_set_rir_bank16, ss_ctx_set_rir_bank16_rows,
 * ss_ctx_set_rir16_buckets: ss_audio_obs_logmel_rir16_f32 / _rows_rir16_f32 / _rir16_buckets_f32 and their shapes); the four
 * setters above keep their meaning and never apply to such a context, and this one applies to no other.  Rebinding a bank keeps
 * the range.  Default: never (max_units < min_units) - the fused values equal the scratch route's to rounding only.  Measured
 * against the scratch route of the same bank, ONE pass (profiles/r12/kbench_obs_logmel_rir16.txt): 16 kHz, one allocation and buckets,
 * 1 .. 512 units: 16-45 % faster, so (1, INT_MAX) is the range a caller would pass there; 44.1 kHz: 15-34 % faster up to 42 units and
 * whenever the spectrogram is asked for as well, but log-mel alone at 43 units is 20 % slower (the row kernel takes over from the
 * one-workgroup-per-block kernel): (1, 42) there. */
int ss_ctx_set_logmel_rir16_policy(ss_ctx* ctx, int min_units, int max_units);
/* Bytes of waveform scratch the context currently holds over all overlap lanes (the scratch route above): 0 after creation and
 * after ss_release_scratch. */
size_t ss_ctx_wave_scratch_bytes(const ss_ctx* ctx);
/* Overlap mode.  ss_ctx_set_overlap(ctx, n), n = 2 .. 4: consecutive ss_ctx_observe calls run on n internal streams in turn
 * (2: the head of step k+1 under the tail of step k; 3 - 4: for steps of few rows, where several launches fit the chip side by
 * side - fused rows are then split over fewer workgroups, ConvParams::parts_log2 - and the caller has that many to issue), each
 * ordered behind what the CALLER's stream holds at the time of the call (the consumers of the output rows it overwrites,
 * uploads of the RIR rows it reads), so the head of step k+1 (descriptor and row loads: HBM latency, nothing to compute)
 * overlaps the tail of step k (STFT: no memory traffic) - what the reference's serial per-env loop
 * (ss_baselines/common/sync_vector_env.py:397-410) cannot do.  Results become visible to a stream through
 * ss_ctx_join(ctx, stream) (the stream waits for every step issued so far); a caller that needs step k before it issues
 * step k+1 joins every step and gets the single-stream behaviour (joins from several streams each wait).  n_streams = 1
 * switches back (synchronises the device).
 * Steps must write disjoint output rows while they are in flight (rollout rows are), and a caller that REWRITES bank rows
 * (eviction: a new pose's RIR over an old entry) while steps are in flight joins first on the stream that carries the
 * rewrite - a step still running on a lane may read the old entry.  The library's own loaders (ss_ctx_observe_requests_load,
 * ss_ctx_load_rir_files) order their scatter behind every step issued so far themselves.
 * Threading: the ordering behind the caller's stream is elided when that stream is IDLE at the time of the call (one
 * hipStreamQuery instead of an event record + a stream wait).  That test is only sound for a single-threaded user of `stream`:
 * a second host thread that enqueues work on the same stream between the query and the lane's launch is NOT ordered in front
 * of the step.  Callers that share the stream between threads must serialise ss_ctx_observe with those enqueues (the
 * reference has one env loop per process: ss_baselines/common/sync_vector_env.py:397-410).  A stream that is being captured
 * into a graph is never queried (hipStreamIsCapturing first); the step is then always fenced. */
int ss_ctx_set_overlap(ss_ctx* ctx, int n_streams);
int ss_ctx_join(ss_ctx* ctx, void* stream);
/* A context that holds BOTH bank forms (ss_ctx_set_rir_bank + ss_ctx_set_rir_spectra) renders from the spectral one.  For
 * rows of one block (16 kHz) that pays for SMALL steps only - no forward FFT on a chip that is mostly idle: 12.9-15.6 us
 * against 17.1-19.0 us per step of 1-32 envs, the reference's 5-10 envs per GPU (ss_baselines/av_nav/config/audionav/
 * {replica,mp3d}/train_telephone/audiogoal_depth_ddppo.yaml:3) - while at 128 envs the forward FFT hides under the rows' loads
 * and the spectral rows are twice the bytes.  max_units > 0: steps of more than max_units units of one-block rows take the
 * time-domain rows - unless the step has distractor terms (two forward transforms per row do not hide under one row's load:
 * savi's 256-env step is 87.9 against 96.3 us); rows of several blocks (44.1 / 48 kHz) are not affected.  0 (default): the
 * spectral form whenever set. */
int ss_ctx_set_spectral_policy(ss_ctx* ctx, int max_units);
/* Small steps are rendered by several workgroups per row while CUs would idle (ConvParams::parts_log2).  A caller that keeps
 * SEVERAL launch sources busy at once - e.g. two env groups stepped alternately, each with a context of its own on its own
 * stream (the double-buffered sampler of bench.py's `dependent.two_groups`; ss_baselines/common/sync_vector_env.py has one
 * group) - says so here: every launch of this context then splits its rows over 1 / n_sources of the chip, so that the
 * sources' launches run side by side instead of queueing behind each other.  0 (default): the context's own lane count. */
int ss_ctx_set_chip_share(ss_ctx* ctx, int n_sources);
/* One step straight from the simulators' state, struct-of-arrays (ss_amd/vector.py::VectorSimState: the int64 columns a
 * vector env keeps per env; HOST memory, n entries each).  Does, for all envs at once, what SoundSpacesSim does per env:
 *   silent = step_count > duration (simulator.py:610) or sound < 0;   t0 = clip is 1 s ? 0 : audio_index * sr (:629-634);
 *   audio_index = (audio_index + 1) % (clip_len / sr) for multi-second clips that are not silent (:635; written back);
 *   azimuth = -rot mod 360 (:573);   RIR slot = index[scene][recv][src] + azimuth / (360 / azimuths)  (the pair's azimuths
 *   sit in adjacent bank rows; table entry -1 = pair not resident);   distractor likewise from dis_sound / dis_src.
 * If some non-silent env's pair is not resident nothing is launched and nothing advanced: their env indices go to
 * miss_out (capacity n), *n_miss > 0 and the call returns 0 - load the pairs, fix the table, call again. */
typedef struct ss_sim_columns {
    const long long* sound;          /* sound id per env, -1 = unknown                     */
    long long* audio_index;          /* in / out                                           */
    const long long* step_count;
    const long long* duration;
    const long long* recv;
    const long long* src;
    const long long* rot;            /* _rotation_angle, degrees                           */
    const long long* scene;          /* scene id = index into index_off / index_dim        */
    const long long* dis_sound;      /* optional (HAS_DISTRACTOR_SOUND): both or neither   */
    const long long* dis_src;
    const int* index_flat;           /* concatenated [dim x dim] tables, first slot or -1  */
    const long long* index_off;      /* [n_scenes] offset of a scene's table in index_flat */
    const long long* index_dim;      /* [n_scenes] nodes per scene                         */
    int n_scenes;
    int azimuths;                    /* bank rows per (receiver, source) pair, e.g. 4      */
} ss_sim_columns;
int ss_ctx_observe_sims(ss_ctx* ctx, const ss_sim_columns* cols, int n, float* audiogoal, float* spectrogram,
                        int* miss_out, int* n_miss, void* stream);
/* The state -> unit columns step of ss_ctx_observe_sims alone (host only, needs no GPU; advances audio_index the same
 * way): units_out int32 [5, n] = sound, t0, rir, dis_sound, dis_rir. */
int ss_ctx_sims_units(ss_ctx* ctx, const ss_sim_columns* cols, int n, int* units_out, int* miss_out, int* n_miss);
/* One step from the packed REQUEST RECORDS of a multi-process vector env (ss_amd/deferred.py: every worker-side sensor
 * returns an AudioRequest whose `rec` is SS_REQ_WORDS int64 words; the trainer concatenates the N records of the step).  Does
 * in C++ what DeferredResolver._columns does in numpy: names travel as CRC-32 keys, ids and resident RIR files are found by
 * binary search in the caller's SORTED tables; reference: what _compute_audiogoal reads per env, simulator.py:608-666.
 *   words: [0] silent  [1] sound key  [2] t0  [3] RIR table key (= directory/azimuth)  [4] receiver  [5] source
 *          [6] distractor sound key or -1  [7] distractor source  [8] env  [9] reserved
 * A request that names an unknown sound / table, a pair that is not resident, or a row flagged stale is a MISS: their
 * indices go to miss_out (capacity n), *n_miss > 0, nothing is launched and the call returns 0 - register / load, call again. */
#define SS_REQ_WORDS 10
typedef struct ss_request_tables {
    const long long* sound_keys;   /* sorted */
    const long long* sound_ids;
    const long long* table_keys;   /* sorted */
    const long long* table_ids;
    const long long* pair_keys;    /* sorted: table id << 40 | receiver << 20 | source */
    const long long* pair_slots;   /* bank slot of the pair's RIR */
    const unsigned char* stale;    /* optional, [n_slots]: != 0 = the row must be reloaded before it is used */
    int n_sounds, n_tables, n_pairs, n_slots;
    /* optional: the caller's LRU clock.  last_used[slot] = tick is written for every bank slot (< n_slots) a request of the
     * step resolves to, so that a store evicting by recency still knows which rows the C path used (the lookups never pass
     * through the store).  NULL: nothing is written. */
    long long* last_used;
    long long tick;
} ss_request_tables;
int ss_ctx_observe_requests(ss_ctx* ctx, const long long* recs, int n, const ss_request_tables* tables, float* audiogoal,
                            float* spectrogram, int* miss_out, int* n_miss, void* stream);
/* Round 6: the same call with the miss path INSIDE it.  The reference reads a pose's RIR file on every cache-missing step
 * (wavfile.read at soundspaces/simulator.py:615-618); with ss_ctx_observe_requests a step that meets a pose whose file is not
 * resident costs three C calls and the store's Python bookkeeping between them (report -> ss_wav_read_rirs_f32 + scatter -> call
 * again).  Here the caller lends the library what that bookkeeping needs - the RIR directories, the sorted resident-pair arrays
 * with spare capacity, a stack of free bank entries, the bank and its length tables, a pinned staging block - and a step whose
 * only misses are poses that are not resident is served in ONE call: file names built, files read by the library's reader
 * straight into the staging block, one scatter launch into the free entries, the pair arrays extended in place, the step
 * launched.  What was loaded is reported (loaded_key / loaded_slot / loaded_frames, n_loaded) so that the caller's own tables
 * (key -> entry dictionaries, LRU order) follow; n_free and *n_pairs are updated.  Anything the fast path does not cover - an
 * unknown sound or directory, a stale row, no entry to be had (stack empty and no eviction arrays lent, or every occupied entry
 * in use by this very step), a file that is not a plain
 * float32 stereo wav / is missing / does not fit the rows, a launch that reads the spectral rows without `stage_desc` - changes NOTHING and is
 * reported exactly as ss_ctx_observe_requests reports it (miss_out, *n_miss > 0).  Arrays are HOST memory unless said
 * otherwise; `stage`, `stage_slot`, `stage_len` must be pinned (the scatter kernel reads them over the host link) and stay
 * untouched by the caller until the stream has run the launch (the library waits for its own previous use of them). */
typedef struct ss_miss_loader {
    const char* const* table_dirs;   /* [n_table_dirs]: directory of table id t ("<BINAURAL_RIR_DIR>/<scene>/<azimuth>")      */
    int n_table_dirs;
    long long* pair_keys;            /* the arrays ss_request_tables.pair_keys / pair_slots point at, writable, ...            */
    long long* pair_slots;
    int pair_cap;                    /* ... with room for pair_cap entries; ss_request_tables.n_pairs is updated                */
    int* free_slots;                 /* stack of free bank entries: the call pops free_slots[n_free - 1], ...                   */
    int n_free;                      /* in: entries on the stack; out: entries left                                             */
    float* bank;                     /* DEVICE: planar time-domain bank [entries][2][cap]; NULL on a spectral-only context       */
    long long bank_unit_stride;      /* floats between entries                                                                   */
    int bank_chan_stride, cap;
    int* dev_len;                    /* DEVICE: rir_len table of the bank                                                        */
    int* host_len;                   /* host mirror of it                                                                        */
    unsigned char* clipped;          /* [entries]: 1 = the stored row is shorter than its file (keep < frames)                  */
    unsigned char* spec_stale;       /* optional [entries]: 1 = the row's block spectra must be rebuilt before a spectral launch */
    int keep;                        /* frames kept per file (1-s clips only ever hear h[0:sr]) or -1 = whole files              */
    float* stage;                    /* PINNED: stage_rows rows of 2 * cap floats (wav layout)                                   */
    int* stage_slot;                 /* PINNED [stage_rows]                                                                      */
    int* stage_len;                  /* PINNED [stage_rows]                                                                      */
    int* stage_desc;                 /* optional, PINNED [stage_rows * 2 * ceil(cap / kB) * 5]: window descriptors of the new rows'
                                      * block spectra - with it, steps that read the SPECTRAL rows (ss_ctx_set_rir_spectra) are
                                      * served too: the new rows are transformed right behind the scatter                        */
    int stage_rows, threads;
    /* optional: eviction inside the call.  When the step needs more entries than the stack holds, the least recently used
     * occupied entries are reused - recency = ss_request_tables.last_used (entries stamped with the step's own tick are never
     * taken), ties by use_seq, oldest first: the policy of RirStore._take_slots.  Their pairs leave pair_keys / pair_slots in
     * the call; evicted_slot names them so that the caller drops its own records of the keys they held.  NULL: no eviction. */
    const unsigned char* used;       /* [n_slots of ss_request_tables]: 1 = the entry is occupied                                */
    const long long* use_seq;        /* [n_slots]: order of last use through the caller's own lookups                            */
    int* evicted_slot;               /* report, capacity evict_cap                                                               */
    int n_evicted, evict_cap;
    long long* loaded_key;           /* report, capacity loaded_cap: pair key, ...                                               */
    int* loaded_slot;                /* ... the entry it went to, ...                                                            */
    int* loaded_frames;              /* ... frames in its file (kept = min(frames, keep))                                        */
    int n_loaded, loaded_cap;
    float* stage_max;                /* optional, PINNED [stage_rows][2]: maxima of |v| per staged row and ear, written by the reader.
                                      * With it (and bank = NULL, cap = the bound rir_cap) a context bound by ss_ctx_set_rir_bank16 /
                                      * _rows is served: halves + scales through k_scatter_rows16_max.  NULL: that form is not served  */
} ss_miss_loader;
int ss_ctx_observe_requests_load(ss_ctx* ctx, const long long* recs, int n, ss_request_tables* tables, ss_miss_loader* loader,
                                 float* audiogoal, float* spectrogram, int* miss_out, int* n_miss, void* stream);
/* The loader alone, for callers that name FILES (the eager call of an agent that has moved: simulator.py:615-618 reads the pose's
 * file on every cache-missing step): k wav files -> k bank entries of the lent store (free stack first, then the least recently
 * used occupied entries whose last_used is below `tick`; last_used / n_slots as in ss_request_tables, NULL = no eviction), one
 * scatter launch on `stream`, block spectra of the new rows when the context holds the spectral form; report in loaded_slot /
 * loaded_frames / evicted_slot.  pair_keys / pair_slots / table_dirs / loaded_key are not used.  Returns 0 = loaded, 1 = not for
 * this path (nothing changed: unusual file, no entry to be had, rows too short, the bank is not the context's), < 0 = error. */
int ss_ctx_load_rir_files(ss_ctx* ctx, ss_miss_loader* loader, const char* const* paths, int k, long long* last_used,
                          long long tick, int n_slots, void* stream);
/* The records -> unit columns step alone (host only, needs no GPU): units_out int32 [5, n] = sound, t0, rir, dis_sound, dis_rir. */
int ss_ctx_requests_units(ss_ctx* ctx, const long long* recs, int n, const ss_request_tables* tables, int* units_out,
                          int* miss_out, int* n_miss);
/* The planner alone (host only, needs no GPU): unit_desc_out int32 [n,8] as ss_fftconv_binaural_f32 takes them,
 * *flags_out the SS_FLAG_* of the launch, *n_new_windows_out the source windows whose spectra would be computed,
 * new_windows_out (optional, int32 [cap,5]) = {src_offset, src_len, start, wrap, pool slot} of those windows. */
int ss_ctx_plan(ss_ctx* ctx, const ss_units* units, int n, int* unit_desc_out, int* flags_out, int* n_new_windows_out,
                int* new_windows_out, int new_windows_cap);
/* out8 = {cache hits, misses, evictions, grows, capacity (keys), keys resident, pool slots per key, steps planned} */
int ss_ctx_stats(ss_ctx* ctx, long long* out8);
/* The descriptor ring's release bookkeeping, four counters that only grow: out4 = {ring events recorded, host waits for a ring
 * event, pace events recorded, host waits for a pace event}.  A ring group records an event only when the device was given one of
 * its slots to read (descriptors read in place or uploaded, a window upload): steps whose launch carries its units in the kernel
 * arguments and that upload no window add to neither of the first two.  Such steps are paced instead: one event per 16 of them,
 * waited for 16 steps later, so a caller that never synchronises stays at most two ring lengths ahead of the device.
 * (A getter of its own: ss_ctx_stats keeps its eight words.) */
int ss_ctx_ring_stats(ss_ctx* ctx, long long* out4);

/* ---- Pose memo on the column path ----------------------------------------------------------------------------------
 * The reference memoises observations per pose (soundspaces/simulator.py:678-701): the key is (source, receiver, azimuth)
 * and ignores _audio_index; _audio_index advances inside a miss only (:634-635); the caches are dropped on a scene or sound
 * change (:395-397).  For multi-second sounds this changes what the agent hears: an agent that stands still or comes back
 * to a pose gets the observation FIRST rendered there again.  The entries below reproduce it inside the step's call.
 *
 * ss_memo_rows_f32 (k_memo_rows, stateless): one launch moves rows between up to 4 (output, pool) array pairs.  moves =
 * {row, slot} per move: the first n_store moves STORE row `row` of every io[a].out into row `slot` of io[a].pool, the
 * following n_fetch moves FETCH pool row `slot` into output row `row`.  Rows are contiguous, row i at base + i * row_floats.
 * `moves` may be device memory or pinned host memory (the kernel reads it in place; pageable host memory is refused).
 * PRECONDITION: rows are distinct and slots are distinct over the WHOLE list - one launch then needs no ordering between
 * its moves (a list that breaks it has an unspecified result in the rows named twice).  Access width per pair from what
 * both bases and row_floats allow: 16 bytes, else 8, else 4.  Rows and slots that are not named, and bytes behind a row's
 * end, are never touched.  n_store + n_fetch == 0 returns 0 without a launch.  SS_EINVAL before a device is touched: n_io
 * outside 1..4, negative counts, and with moves pending a NULL io / out / pool / moves, row_floats < 1, a base that is not
 * 4-byte aligned.  Asynchronous on `stream`. */
typedef struct ss_memo_io { float* out; float* pool; int row_floats; int reserved; } ss_memo_io;
int ss_memo_rows_f32(const ss_memo_io* io, int n_io, const int* moves, int n_store, int n_fetch, void* stream);
/* The memo of a context (host state; csrc/ss_memo.hpp): per env a tag (scene, sound) and a map pose key -> pool row, one
 * free list over the caller's pool rows.  n_envs >= 1 switches it on for steps of exactly n_envs envs (again: reset with a
 * new size); 0 switches it off and frees the state.  _reset forgets every pose and the counters (the pools' contents become
 * meaningless); _stats: out4 = {hits, misses, pool rows in use, maps dropped by a scene / sound change}.  _reset and _stats
 * are SS_EINVAL while the memo is off. */
int ss_ctx_memo_enable(ss_ctx* ctx, int n_envs);
int ss_ctx_memo_reset(ss_ctx* ctx);
int ss_ctx_memo_stats(ss_ctx* ctx, long long* out4);
/* The device-side pools, owned by the caller: `rows` rows each, a row the size of one env's output row ([65,T4,2] /
 * [2,sr] floats).  An array is given exactly when its output is.  The caller may replace them by LARGER ones (contents
 * kept, ordered against the step streams by the caller: in overlap mode ss_ctx_join first); rows never shrinks below the
 * value rows were last handed out of (SS_EINVAL; ss_ctx_memo_reset starts over). */
typedef struct ss_memo_pool { float* spectrogram; float* audiogoal; int rows; int reserved; } ss_memo_pool;
/* ss_ctx_observe_sims with the memo inside: plan, render, move - in that order.
 *   plan:   an env whose (scene, sound) changed drops its map first (its rows are free again and may serve this very step);
 *           an env whose pose key (src << 40 | recv << 20 | azimuth) is present is a HIT and is HELD: a silent unit, no RIR
 *           looked up (never an RIR miss), audio_index not advanced; every other env is a MISS: rendered as
 *           ss_ctx_observe_sims renders it and given a free pool row - silent envs too (the reference caches its zeros
 *           under the pose as well);
 *   render: as ss_ctx_observe, held envs as silent units;
 *   move:   k_memo_rows on the same stream right behind the step's launches (overlap mode: on the step's lane, behind the
 *           other lanes' latest moves by stream waits - no join is needed for it and none is issued; results are visible to
 *           a stream after ss_ctx_join as for every step).  The move list travels in the kernel arguments: no copy, no host
 *           wait, nothing of the descriptor ring is read.
 * TRANSACTIONAL: a non-resident pair of an env that is neither held nor silent (*n_miss > 0, indices in miss_out, capacity n)
 * or too few free pool rows (*need_rows = rows the pools need in total, > pool->rows) launches nothing and commits nothing -
 * no audio_index change, no memo entry, no move - and returns 0; both may be reported by one call.  Otherwise
 * *need_rows = 0.  A step that fails with an error commits nothing either.
 * SS_EINVAL: the memo is off; n != n_envs; cols->dis_sound / dis_src != NULL (the reference bypasses its caches with a
 * distractor, :679-681 - use ss_ctx_observe_sims there); pool == NULL or pool->rows < 0 or below the rows already handed
 * out; an output without its pool array or a pool array without its output; a set of outputs other than the one the memo's
 * rows were first stored with; everything ss_ctx_observe_sims refuses.
 * Pool row numbering is the library's own. */
int ss_ctx_observe_sims_memo(ss_ctx* ctx, const ss_sim_columns* cols, int n, float* audiogoal, float* spectrogram,
                             const ss_memo_pool* pool, int* miss_out, int* n_miss, int* need_rows, void* stream);
/* The host half alone (needs no GPU; commits exactly as the full call would, the set of outputs apart): units_out int32
 * [5, n] as ss_ctx_sims_units (held envs silent), hold_out [n] 1 = held, moves_out int32 [n][2] = {env, pool row}: the
 * step's *n_store misses first, then its *n_fetch hits (both 0 when the step was not committed). */
int ss_ctx_sims_memo_plan(ss_ctx* ctx, const ss_sim_columns* cols, int n, int pool_rows, int* units_out,
                          unsigned char* hold_out, int* moves_out, int* n_store, int* n_fetch, int* miss_out, int* n_miss,
                          int* need_rows);

/* ---- RIR files -> staging rows (the step BEFORE the path: SURVEY 8(f)2) ---------------------------------------------
 * Replaces the reference's per-miss `scipy.io.wavfile.read(binaural_rir_file)` (soundspaces/simulator.py:615-618, float32
 * stereo files under <binaural_rir_dir>/<azimuth>/<recv>_<src>.wav) for bulk loads and the per-step pose misses of the
 * vector modes: n files are parsed (RIFF header, "fmt " / "data" chunks) and their first `keep` frames (keep < 0: all) are
 * read() straight into row i of `dst` on up to n_threads plain threads - HOST pointers here, typically a pinned staging
 * block that one H2D copy then moves.  Row i starts at dst + i * row_stride floats (row_stride >= 2 * cap) and is
 * wav-interleaved [cap][2] (planar = 0: the file's own layout, no transpose; the kernels read such rows with
 * rir_elem_stride = 2) or planar [2][cap] (planar = 1); rows are zero beyond the frames kept.
 * status_out[i]: 0 loaded; 1 not a plain little-endian float32 stereo RIFF/WAVE file (integer PCM, RIFX, malformed ...):
 * NOT interpreted here - route that file through the Python reader, which keeps scipy's semantics (ValueError -> zero RIR,
 * :619-621); 2 no frames (-> zero RIR, :622-624); 3 cannot be opened; 4 more frames to keep than `cap` (nothing read:
 * grow the rows and retry).  kept_out[i] = frames stored, frames_out[i] = frames in the file.  Rows with a non-zero
 * status are zero-filled.  Returns 0 / SS_EINVAL. */
int ss_wav_read_rirs_f32(const char* const* paths, int n, float* dst, long long row_stride, int cap, int keep, int planar,
                         int* kept_out, int* frames_out, int* status_out, int n_threads);
/* The same read in wav layout (planar = 0) with the rows' maxima: max_out [n][2] (host memory) receives, per row and ear, the
 * maximum of |v| over the frames KEPT - taken with fmax in one pass on the reader's thread, right behind the row's read(); frames
 * of the file behind `keep` do not count; 0, 0 for every non-zero status.  What ss_bank_scatter_rows16_max_f32 takes as row_max.
 * Rows, kept_out, frames_out and status_out are those of ss_wav_read_rirs_f32.  Returns 0 / SS_EINVAL (also max_out == NULL). */
int ss_wav_read_rirs_max_f32(const char* const* paths, int n, float* dst, long long row_stride, int cap, int keep,
                             int* kept_out, int* frames_out, int* status_out, int n_threads, float* max_out);
/* The miss path's last hop: n staged rows in wav layout - row i = frames j < lens[i] as (L, R) pairs at
 * staged[i*staged_row_stride + 2*j + c] - into the planar bank rows bank[slots[i]*unit_stride + c*chan_stride + j], zeros
 * behind each row's length up to `cap`, and lens[i] into bank_len[slots[i]] (bank_len may be NULL).  `staged`, `slots`
 * and `lens` may be PINNED HOST memory (the kernel pulls the samples over the host link: one launch, no staging copy) or
 * device memory (pageable host memory is refused: SS_EINVAL); bank / bank_len are device memory.  Asynchronous on `stream`: the caller keeps the staged block alive and
 * unchanged until the launch has run.  Replaces the reference's per-file host path simulator.py:615-624 -> numpy -> (no
 * device at all there) for what follows ss_wav_read_rirs_f32 / ss_rows_gather_f32.  Returns 0 / SS_EINVAL / -hipError_t. */
int ss_bank_scatter_rows_f32(const float* staged, long long staged_row_stride, const int* slots, const int* lens, int n,
                             float* bank, long long unit_stride, int chan_stride, int cap, int* bank_len, void* stream);
/* The same hop for a SPECTRAL-ONLY bank (no time-domain rows, see ss_ctx_set_rir_spectra): n staged rows -> the block spectra
 * H'_b = 2 rFFT(block b) of both ears in entry slots[i] of hspec [entries][2][h_blocks][ss_spec_floats()] - item order and
 * scale exactly those of ss_rir_spectra_f32, whose output over the scattered planar rows they equal bit for bit - and lens[i]
 * into bank_len[slots[i]] (bank_len may be NULL), ONE launch (k_stage_spectra: one workgroup per row and block).  Row i
 * starts at staged + i * staged_row_stride floats: wav layout [frames][2] (planar = 0; staged_row_stride even) or planar
 * [2][staged_row_stride / 2] (planar = 1; staged_row_stride a multiple of 4); `staged` 8-byte aligned.  A row holds
 * cap = min(staged_row_stride / 2, h_blocks * kB) frames; lens[i] is clamped to [0, cap] and frames at or beyond it are
 * not read (zero).  `staged`, `slots`, `lens`: pinned host or device memory as for ss_bank_scatter_rows_f32 (pageable host
 * memory is refused: SS_EINVAL); hspec / bank_len are device memory.  Asynchronous on `stream`.
 * Returns 0 / SS_EINVAL / -hipError_t. */
int ss_bank_scatter_spectra_f32(const float* staged, long long staged_row_stride, int planar, const int* slots, const int* lens,
                                int n, float* hspec, int h_blocks, int* bank_len, void* stream);
/* ... into a HALF bank (fp16 spectra + scales, "Half-precision spectral bank"): same staging rules, same lengths table. */
int ss_bank_scatter_spectra16_f32(const float* staged, long long staged_row_stride, int planar, const int* slots, const int* lens,
                                  int n, void* hspec16, float* hscale, int h_blocks, int* bank_len, void* stream);
/* ... and into a bank of HALF-PRECISION TIME-DOMAIN ROWS ("Half-precision time-domain rows"): the contract of
 * ss_bank_scatter_rows_f32 - wav-layout rows in pinned host or device memory (pageable: SS_EINVAL), 8-byte aligned, an even
 * staged_row_stride >= 2 cap - into halves + scale of both ears in entry slots[i], +0 halves behind the row's length up to `cap`,
 * lens[i] (clamped to [0, cap]) into bank_len[slots[i]] (may be NULL).  Bit-identical to ss_rir_rows16_f32 over the rows
 * ss_bank_scatter_rows_f32 would have written.  One launch; a row is read twice (maxima, then quantisation), never staged. */
int ss_bank_scatter_rows16_f32(const float* staged, long long staged_row_stride, const int* slots, const int* lens, int n,
                               void* rir16, float* rscale, int cap, int* bank_len, void* stream);
/* The same hop in ONE pass over each row, for callers that know the rows' maxima (ss_wav_read_rirs_max_f32 takes them while it
 * reads): row_max is [n][2] fp32 in pinned host or device memory (pageable: SS_EINVAL), row_max[i][c] = the maximum of |v| over
 * ear c of the frames j < clamp(lens[i], 0, cap), 0 for an empty row.  k_scatter_rows16_max: a row is spread over ceil(cap / 512)
 * workgroups and every kept frame is read once, frames at or behind the length never.  Same bits as ss_bank_scatter_rows16_f32 on
 * the same samples: halves, scales, lengths.  A row_max that is not the rows' maxima gives unspecified values in the entries
 * named and touches nothing else.  The refusals of ss_bank_scatter_rows16_f32, and row_max == NULL or not 4-byte aligned;
 * n == 0 returns 0 without a launch. */
int ss_bank_scatter_rows16_max_f32(const float* staged, long long staged_row_stride, const int* slots, const int* lens,
                                   const float* row_max, int n, void* rir16, float* rscale, int cap, int* bank_len, void* stream);
/* n HOST arrays -> n rows of a (pinned) staging block: row i = src[i][0 .. n_floats[i]) followed by zeros up to row_floats,
 * rows row_stride floats apart, on up to n_threads plain threads.  The live RIRs of a SoundSpaces 2.0 step (one new RIR per
 * env and step from the ray tracer, soundspaces/continuous_simulator.py:419) travel to the bank this way: one block, one
 * H2D copy.  Returns 0 / SS_EINVAL. */
int ss_rows_gather_f32(const float* const* src, const int* n_floats, int n, float* dst, long long row_stride, int row_floats,
                       int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* SS_HIP_H */
