// ss_route.hpp — which launch serves a step: the shape rules of the observation kernels and the one decision built from them.
//
// Pure host C++, no HIP runtime and no environment: tests/route_host.cpp compiles this header on its own and prints the
// route of every case of a fixed grid (tests/golden/route_table.txt pins it).  ss_hip.hip is the only other reader: the
// stateless C entries walk obs_chain() for the bank form they were given, the context API asks route_step() once per
// step.  The A/B switches of -DSS_AB builds are read over there and arrive here as plain values (Switches).
#pragma once

#include "../../include/ss_hip.h"
#include "ss_consts.hpp"

namespace ssroute {

using ssk::kB;

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }   // a >= 0, b > 0
inline int n_frames_of(int len) { return 1 + len / ssk::kHop; }
inline int t4_of(int len) { return (n_frames_of(len) + ssk::kPool - 1) / ssk::kPool; }

struct Switches {
    bool no_wide = false;             // SS_HIP_NO_WIDE (A/B builds only: -DSS_AB)
};

// Rows longer than one block of which only block 0 is rendered (SS2.0 steps at 44.1 kHz: 0.25 s of a 1-s row) and whose live
// pooled blocks all lie inside that block: the fused LOOP kernel serves them in one launch (k_conv<..., WIDE>: block spectra
// accumulated in registers, the spectrogram's dead columns written as zeros) - with or without a waveform buffer.
inline bool wide_one_block_ok(int out_len, int n_valid, int flags, bool spectral, const Switches& sw) {
    if (sw.no_wide || spectral || out_len <= kB || n_valid < 0 || n_valid > kB) return false;
    if ((flags & SS_FLAG_CROSSFADE) &&
        (static_cast<int>(0.05 * out_len) < 1 || static_cast<int>(0.05 * out_len) > 2 * ssk::kPrevPairs - 2)) return false;
    return ssk::live_blocks(n_valid, out_len, t4_of(out_len)) <= 26;
}

// should k_obs_rows serve this shape?  (rows of 2 or 3 blocks, stash mask of 32 bits.)  Rows with ONE rendered block
// (n_valid <= kB: SS2.0 steps at 44.1 kHz) and cross-faded rows: only when the caller has no waveform buffer.  With one,
// the loop kernel (block spectra accumulated in registers: every one is used once, the rows kernel's stash is pure overhead
// there) + k_spectrogram (told where the zeros of a short step begin) is faster - per 128 units at 44.1 kHz: plain steps
// 61.6 vs 72.5 us (66.3 without the waveform written), cross-faded 92.7 vs 117.8 us (profiles/r3/NOTES.md section 8)
inline bool obs_rows_ok(int out_len, int n_valid, int nbh_max, int flags, bool spectral = false, bool have_waveform_buffer = false) {
    if (have_waveform_buffer && ((flags & SS_FLAG_CROSSFADE) || n_valid <= kB)) return false;
    if ((flags & SS_FLAG_CROSSFADE) &&
        (spectral || static_cast<int>(0.05 * out_len) < 1 || static_cast<int>(0.05 * out_len) > 2 * ssk::kPrevPairs - 2)) return false;
    return out_len > kB && out_len <= 3 * kB && n_valid <= out_len && nbh_max >= 1 && nbh_max <= 16;
}

// rows the log-mel form serves: one partition block, long enough for the reflect padding, no cross-fade
inline bool obs_logmel_shape_ok(int out_len, int flags) {
    return out_len >= ssk::kNfft / 2 + 1 && out_len <= kB && !(flags & SS_FLAG_CROSSFADE);
}

// SoundSpaces 2.0 steps the log-mel form serves (time-domain bank): (A) cross-faded one-block rows - fade_len = int(0.05 out_len)
// lies inside [1, 2 kPrevPairs - 2] for every such length - and (B) rows of 2 or 3 blocks of which only block 0 is rendered
// (wide_one_block_ok: its own cross-fade limits).  0: neither, 1: (A), 2: (B).
inline int obs_logmel_ss2_shape(int out_len, int n_valid, int flags, const Switches& sw) {
    if (n_valid < 0 || n_valid > out_len) return 0;
    if (out_len >= ssk::kNfft / 2 + 1 && out_len <= kB) return (flags & SS_FLAG_CROSSFADE) ? 1 : 0;
    return out_len <= 3 * kB && wide_one_block_ok(out_len, n_valid, flags, false, sw) ? 2 : 0;
}

// rows the log-mel form of k_obs_rows / k_obs_blocks serves: 2 or 3 partition blocks (44.1 / 48 kHz), plain steps, at most 16
// RIR blocks (obs_rows_ok without a cross-fade; a waveform buffer changes nothing here: the caller chose the entry)
inline bool obs_logmel_rows_shape_ok(int out_len, int n_valid, int nbh_max, int flags) {
    return !(flags & SS_FLAG_CROSSFADE) && n_valid >= 0 && obs_rows_ok(out_len, n_valid, nbh_max, flags);
}

// rows the log-mel entries of the length-bucketed banks serve (ss_audio_obs_logmel_buckets_f32 / _spec_buckets_f32): one partition
// block on every bank form; 2 or 3 blocks on the fp32 forms - and on half spectral buckets bound for such rows (half_rows:
// ss_ctx_set_rir_spec_buckets_rows) - with the deepest bucket's blocks inside the row kernels' limit
inline bool obs_logmel_buckets_shape_ok(int out_len, int n_valid, int nbh_max, int flags, bool half, bool half_rows = false) {
    if (n_valid < 0 || n_valid > out_len) return false;
    if (obs_logmel_shape_ok(out_len, flags)) return true;
    return (!half || half_rows) && obs_logmel_rows_shape_ok(out_len, n_valid, nbh_max, flags);
}

// One value per distinct launch body (not per C entry: every bank form has the same bodies).
enum class Launch {
    kNone,          // nothing is launched (a refused step)
    kConv,          // the waveform alone: the unfused convolution
    kObs,           // waveform and / or spectrogram: the chain below
    kMelOneBlock,   // log-mel forms, no waveform buffer: one-block rows (obs_logmel_shape_ok)
    kMelSs2,        // ... SoundSpaces 2.0 steps from time-domain rows (obs_logmel_ss2_shape)
    kMelRows,       // ... rows of 2 or 3 blocks (obs_logmel_rows_shape_ok)
};

// The chain every observation (Launch::kObs) walks: fused one-block, then wide, then rows, then two launches with the waveform
// handed over through memory (which needs a buffer).
enum class Chain {
    kFused,         // one-block rows in one launch (the waveform stays in LDS)
    kWide,          // block 0 of a longer row: the fused loop kernel (wide_one_block_ok)
    kRows,          // rows of 2 or 3 blocks: k_obs_blocks / k_obs_rows (obs_rows_ok)
    kTwo,           // the unfused convolution into a waveform buffer, then k_spectrogram over it
};
inline Chain obs_chain(int out_len, int n_valid, int nbh_max, int flags, bool spectral, bool have_waveform_buffer,
                       const Switches& sw) {
    if (out_len <= kB && t4_of(out_len) <= 26) return Chain::kFused;
    if (wide_one_block_ok(out_len, n_valid, flags, spectral, sw)) return Chain::kWide;
    if (obs_rows_ok(out_len, n_valid, nbh_max, flags, spectral, have_waveform_buffer)) return Chain::kRows;
    return Chain::kTwo;                                                               // cross-faded / very long rows
}

// What is bound to a context (ss_ctx_set_rir_bank / _spectra / _spectra16 / _spectra16_rows / _buckets / _spec_buckets / _spec_buckets_rows)
struct Bank {
    bool rows = false;                // time-domain rows (of a length-bucketed bank: bucket 0's)
    bool spectra = false;             // block spectra of a single-allocation bank, fp32 or ...
    bool half = false;                // ... fp16 + one scale per block
    bool buckets = false;             // length buckets that keep rows (ss_rir_bucket[]) ...
    bool buckets_spectra = false;     // ... every one of which carries its fp32 spectra as well
    bool spec_buckets = false;        // length buckets without rows (ss_spec_bucket[]), fp32 or ...
    bool spec_buckets_half = false;   // ... half
    int rir_cap = 0;                  // samples per row (length buckets: the deepest bucket's blocks * kB)
    int h_blocks = 0;                 // blocks of `spectra`
    bool spec_buckets_half_rows = false;      // half `spec_buckets` bound for rows of 2 or 3 blocks (ss_ctx_set_rir_spec_buckets_rows)
    bool rows16 = false;              // half-precision time-domain rows (ss_ctx_set_rir_bank16): nothing else is bound then
    bool rows16_rows = false;         // ... bound for the fused row kernels as well (ss_ctx_set_rir_bank16_rows; only with rows16)
    bool rows16_buckets = false;      // half-precision time-domain rows in length buckets (ss_ctx_set_rir16_buckets): nothing else is bound then
};

struct Policies {
    int spectral_max_units = 0;       // ss_ctx_set_spectral_policy: one-block rows take the spectral bank only for steps of <= this many units (0: always)
    // ss_ctx_set_logmel_policy: log-mel steps without a waveform buffer take the fused launch for min <= units <= max
    int mel_fused_min = 1, mel_fused_max = 0x7fffffff;
    // ss_ctx_set_logmel_rows_policy: the same for rows of 2 or 3 blocks (44.1 / 48 kHz); default: never
    int mel_rows_min = 1, mel_rows_max = 0;
    int mel_ss2_min = 1, mel_ss2_max = 0;       // ss_ctx_set_logmel_ss2_policy: never, by default
    int mel_bk_min = 1, mel_bk_max = 0;         // ss_ctx_set_logmel_buckets_policy (length-bucketed banks): never, by default
    // ss_ctx_set_logmel_rir16_policy (half-precision time-domain rows, one allocation or length buckets): never, by default
    int mel_r16_min = 1, mel_r16_max = 0;
};

struct Wants {
    bool waveform = false;            // the caller gave a waveform buffer
    bool spectrogram = false;
    bool mel = false;                 // a log-mel step without a waveform buffer (ss_ctx_observe_features)
};

struct Route {
    Launch launch = Launch::kNone;
    Chain chain = Chain::kFused;      // (Launch::kObs: where the chain ends)
    bool spectral = false;            // the launch reads block spectra (else the time-domain rows)
    bool refused = false;             // a spectral-only bank cannot serve a cross-faded step
    bool wave_scratch = false;        // a log-mel step no log-mel form serves: renders into the context's waveform scratch
    bool handover = false;            // two launches without a caller's waveform: the context's hand-over buffer
};

// The route of one step of a context: `flags` are the planner's, n the step's units.
inline Route route_step(const Bank& b, int out_len, int n_valid, const Policies& pol, int n, int flags, const Wants& w,
                        const Switches& sw = Switches()) {
    Route r;
    const bool xfade = (flags & SS_FLAG_CROSSFADE) != 0;
    const bool bucketed = b.buckets || b.spec_buckets;
    // half-precision time-domain rows: the fused half kernels for one-block rows, every longer row the half convolution into the
    // caller's waveform buffer or the context's hand-over buffer and k_spectrogram over it (no wide kernel reads halves);
    // no cross-fade (refused as on the spectral-only banks).
    // Log-mel steps without a waveform buffer, inside the units range of ss_ctx_set_logmel_rir16_policy (default never; the four
    // other log-mel policies never apply here): the log-mel form of the half kernels - one-block rows on both bindings
    // (k_conv<.., MEL, HALF>), rows of 2 or 3 blocks only on a bank bound by ss_ctx_set_rir_bank16_rows (k_obs_blocks /
    // k_obs_rows<.., MEL, .., ROWS16>).  Every other log-mel step renders into the waveform scratch.
    // Bound by ss_ctx_set_rir_bank16_rows (rows16_rows), rows of 2 or 3 blocks take k_obs_blocks / k_obs_rows<.., ROWS16> wherever
    // obs_rows_ok hands the shape to them - a log-mel step's scratch counts as its waveform buffer - and need no hand-over
    // buffer there.
    // Half rows in length buckets (rows16_buckets; rir_cap = the deepest bucket's blocks * kB): exactly as rows16, and never the
    // row kernels - they do not read bucketed half rows.
    if (b.rows16 || b.rows16_buckets) {
        if (xfade) {
            r.refused = true;
            return r;
        }
        if (w.mel && !w.waveform && n >= pol.mel_r16_min && n <= pol.mel_r16_max) {
            if (obs_logmel_shape_ok(out_len, flags)) r.launch = Launch::kMelOneBlock;
            else if (b.rows16 && b.rows16_rows && obs_logmel_rows_shape_ok(out_len, n_valid, ceil_div(b.rir_cap, kB), flags))
                r.launch = Launch::kMelRows;
            if (r.launch != Launch::kNone) return r;
        }
        r.wave_scratch = w.mel;
        if (!w.spectrogram) {
            r.launch = Launch::kConv;
            return r;
        }
        r.launch = Launch::kObs;
        const bool have_wave = w.waveform || r.wave_scratch;
        r.chain = out_len <= kB && t4_of(out_len) <= 26 ? Chain::kFused : Chain::kTwo;
        if (r.chain == Chain::kTwo && b.rows16 && b.rows16_rows && obs_rows_ok(out_len, n_valid, ceil_div(b.rir_cap, kB), flags, false, have_wave))
            r.chain = Chain::kRows;
        r.handover = r.chain == Chain::kTwo && !have_wave;
        return r;
    }
    // a spectral-only bank (spectra bound, no rows: ss_ctx_set_rir_bank(ctx, NULL, ...) + ss_ctx_set_rir_spectra) cannot serve a
    // step whose route reads the time-domain rows (a cross-fade)
    // (spectral length buckets, ss_ctx_set_rir_spec_buckets, are such a bank)
    if (!b.rows && !b.buckets && ((!b.spectra && !b.spec_buckets) || xfade)) {
        r.refused = true;
        return r;
    }
    // cross-faded steps take the time-domain rows; so do LARGE steps of one-block rows when the caller keeps both forms and said
    // so (ss_ctx_set_spectral_policy): there the forward FFT hides under the row's load and the spectral rows are twice the bytes
    // (... unless its units carry a second term - a distractor, simulator.py:649-664: two forward transforms per row do not hide
    // under one row's load; savi's 256-env step: 87.9 against 96.3 us)
    // (length buckets that keep rows: spectral when every bucket carries its spectra)
    r.spectral = b.buckets ? b.buckets_spectra && !xfade
                           : (b.spectra || b.spec_buckets) && !xfade &&
                                 !(pol.spectral_max_units > 0 && b.rows && out_len <= kB && n > pol.spectral_max_units &&
                                   (flags & SS_FLAG_NO_DISTRACTOR));
    const int nbh_cap = b.rir_cap > 0 ? ceil_div(b.rir_cap, kB) : 1;
    const int nbh_bank = r.spectral && !bucketed ? b.h_blocks : nbh_cap;
    // log-mel without a waveform buffer - inside the units range the measured policy of the bank form gives (single allocation:
    // ss_ctx_set_logmel_policy for one-block rows, default always; _rows_policy and _ss2_policy, default never: the scratch
    // route is bit-equal to observe-then-features, the fused arithmetic only to rounding; length buckets: _buckets_policy,
    // default never, and the three others never apply) - the log-mel form of the kernels where one serves the shape
    auto within = [n](int lo, int hi) { return n >= lo && n <= hi; };
    if (w.mel && !bucketed) {
        if (obs_logmel_shape_ok(out_len, flags) && within(pol.mel_fused_min, pol.mel_fused_max)) r.launch = Launch::kMelOneBlock;
        // (a half bank: only the one bound by ss_ctx_set_rir_spectra16_rows has rows this long)
        else if ((!b.half || out_len > kB) && (r.spectral || (b.rows && b.rir_cap > 0)) &&
                 obs_logmel_rows_shape_ok(out_len, n_valid, nbh_bank, flags) && within(pol.mel_rows_min, pol.mel_rows_max))
            r.launch = Launch::kMelRows;
        else if (b.rows && !r.spectral && obs_logmel_ss2_shape(out_len, n_valid, flags, sw) != 0 &&
                 within(pol.mel_ss2_min, pol.mel_ss2_max))
            r.launch = Launch::kMelSs2;
    } else if (w.mel && obs_logmel_buckets_shape_ok(out_len, n_valid, nbh_cap, flags, b.spec_buckets_half, b.spec_buckets_half_rows) &&
               within(pol.mel_bk_min, pol.mel_bk_max)) {
        r.launch = out_len <= kB ? Launch::kMelOneBlock : Launch::kMelRows;
    }
    if (r.launch != Launch::kNone) return r;
    // everything else renders a waveform: into the caller's buffer, else (log-mel steps) into the context's waveform scratch,
    // which the feature kernel then reads
    r.wave_scratch = w.mel;
    if (!w.spectrogram) {
        r.launch = Launch::kConv;
        return r;
    }
    // the rows the time-domain entry counts (rir_cap = 0: none, which k_obs_rows does not serve)
    const int nbh = r.spectral && !bucketed ? b.h_blocks : bucketed ? nbh_cap : ceil_div(b.rir_cap, kB);
    // Cross-faded / very long rows hand over through memory.  A step without a waveform buffer gets the context's own when the
    // chain, walked as WITH a buffer, ends in two launches: given one, cross-faded rows and rows of one rendered block are
    // faster there than in k_obs_rows (obs_rows_ok).
    // (Length buckets that keep rows: asked as of time-domain rows, whatever spectra the buckets carry - a step on block 0 of a
    // longer row then stays with k_obs_rows, or, past its 16 RIR blocks, is left without a buffer and refused by the launch.)
    const bool have_wave = w.waveform || r.wave_scratch;
    r.handover = !have_wave && obs_chain(out_len, n_valid, nbh_bank, flags, r.spectral && !b.buckets, true, sw) == Chain::kTwo;
    r.launch = Launch::kObs;
    r.chain = obs_chain(out_len, n_valid, nbh, flags, r.spectral, have_wave || r.handover, sw);
    return r;
}

}  // namespace ssroute
