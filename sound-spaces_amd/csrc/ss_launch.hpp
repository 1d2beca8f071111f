// ss_launch.hpp — how a launch is shaped: output blocks, parts, grids, kernel variant, stash and hand-off sizes, and the shape
// fields of ConvParams.  Three layers: ss_route.hpp decides WHICH launch serves a step; this header decides its geometry;
// ss_dispatch.hpp decides which kernel instantiation runs it.  ss_hip.hip acquires the resources at the sizes given here in between.
//
// Pure host C++, no HIP runtime, no environment, no statics, no pointers to device memory: tests/launch_host.cpp compiles this
// header on its own and prints the plan of every case of a fixed grid (tests/golden/launch_table.txt and launch_mel_table.txt pin
// it), and the host simulator (tests/hostsim/hostsim.cpp and the drivers around it) shapes its launches with the same functions
// and dispatches them through ss_dispatch.hpp - so the CPU tests of the kernels run the library's own geometry and kernel choice.  The A/B switches of -DSS_AB builds are read in ss_hip.hip and arrive here as
// plain values (Switches).
#pragma once

#include <cstddef>
#include <type_traits>

#include "ss_consts.hpp"
#include "ss_route.hpp"

namespace sslaunch {

using ssk::kB;
using ssroute::ceil_div;
using ssroute::n_frames_of;
using ssroute::t4_of;

struct Switches {
    int parts_log2 = -1;              // SS_HIP_PARTS_LOG2: >= 0 forces the parts of every launch (A/B builds only: -DSS_AB)
    bool no_row_kernel = false;       // SS_HIP_NO_ROW_KERNEL
    bool no_obs_blocks = false;       // SS_HIP_NO_OBS_BLOCKS
};

// output blocks of a row of which n_valid samples are rendered (a silent step still launches one)
inline int nb_y_of(int n_valid) { return n_valid == 0 ? 1 : (n_valid + kB - 1) / kB; }

// Small steps (fewer rows than CUs): a fused one-block row is rendered by 2^k workgroups on as many CUs, each running the
// row's convolution and its share of the pooled STFT blocks (ConvParams::parts_log2) - as long as the grid still fits the
// chip in one round of one workgroup per CU.  26 pooled blocks: k <= 3 (shares of 13 / 7 / 4 blocks).
inline int parts_log2_for(int n_rows, int n_cus, int share, int forced) {
    if (forced >= 0) return forced < 3 ? forced : 3;
    const int cus = n_cus / (share > 1 ? share : 1);       // overlap mode: the lanes share the chip
    int k = 0;
    while (k < 3 && (n_rows << (k + 1)) <= cus) ++k;
    return k;
}

// ---- the convolution launches (k_conv, k_conv_spec and their half forms; fused with the STFT or not) -------------------------
enum class Form {                     // the bank form the launch reads
    kRows,                            // fp32 time-domain rows (length buckets that keep rows included)
    kRows16,                          // half-precision time-domain rows + one scale per (entry, ear); n_buckets > 1: in length buckets
    kSpec,                            // fp32 block spectra
    kSpec16,                          // fp16 block spectra + one scale per block, one allocation
    kSpec16Buckets,                   // ... in length buckets
};
enum class Variant {
    kSimple,                          // the loop-free kernel: one term, one block, bucket 0
    kLoop,                            // the loop kernel
    kXfade,                           // the loop kernel with the cross-fade
    kWide,                            // block 0 of a longer row (ssroute::wide_one_block_ok)
    kWideXfade,
    kPersistRows,                     // more rows than CUs: persistent workgroups (k_conv_rows / k_conv_spec_rows)
};
struct ConvPlan {
    int rc = 0;                       // SS_EINVAL: the launch is refused and nothing else of the plan is set
    Variant variant = Variant::kLoop;
    bool tab_ok = false;              // kSimple: the unit table may be tried (the host knows the descriptors: fill_unit_tab)
    bool bucket0 = true;              // the launch addresses bucket 0 only (kSpec16Buckets, bucketed kRows16: the single-allocation half kernels)
    int grid_x = 1, grid_y = 1;
    int parts_log2 = 0;
    int nb_y = 1;
};

// planar: the rows can be read as pairs (elem stride 1, even cap and strides, 8-byte base); hspec_aligned: 16-byte base of the
// spectra.  The caller computes both from its pointers.  n_cus = 0 (spectral forms): no parts, no persistent kernel.
inline ConvPlan plan_conv(Form form, bool fuse, bool wide, int flags, int rir_cap, int h_blocks, int n_buckets, int fade_len,
                          bool planar, bool hspec_aligned, int n_units, int nb_y, int n_cus, int share, const Switches& sw) {
    ConvPlan pl;
    const bool time = form == Form::kRows || form == Form::kRows16;
    const bool xfade = (flags & SS_FLAG_CROSSFADE) != 0;
    pl.rc = SS_EINVAL;
    if (nb_y < 1 || nb_y > 3 || (fuse && nb_y != 1) || (form != Form::kRows && xfade)) return pl;
    if (xfade && (fade_len < 1 || fade_len > 2 * ssk::kPrevPairs - 2)) return pl;
    pl.rc = 0;
    pl.nb_y = nb_y;
    wide = wide && fuse && form == Form::kRows;
    pl.parts_log2 = fuse && (time ? !wide : n_cus > 0) ? parts_log2_for(2 * n_units, n_cus, share, sw.parts_log2) : 0;
    if (wide) {
        pl.variant = xfade ? Variant::kWideXfade : Variant::kWide;
        pl.grid_x = 2 * n_units;
        return pl;
    }
    // the loop-free kernels address bucket 0 only: a bucketed bank qualifies when the caller promises that every index
    // of the launch lies there (SS_FLAG_FIRST_BUCKET; the context's planner works it out per step)
    pl.bucket0 = n_buckets == 1 || (flags & SS_FLAG_FIRST_BUCKET);
    const bool simple = (flags & SS_FLAG_NO_DISTRACTOR) && !xfade && nb_y == 1 && (time ? rir_cap <= kB : h_blocks == 1) && pl.bucket0;
    // time-domain rows: blockIdx.y is the output block; spectra: slot = (row, j), j fastest
    pl.grid_x = time ? (2 * n_units) << pl.parts_log2 : (2 * n_units * nb_y) << pl.parts_log2;
    pl.grid_y = time ? nb_y : 1;
    // more rows than CUs: persistent workgroups that prefetch the next row's RIR (spectra: H') under the current row's FFT
    // passes.  The fused kernel gains nothing from it (measured), see k_conv_rows; the half forms have no such kernel.
    if (!fuse && simple && !sw.no_row_kernel &&
        (form == Form::kRows ? planar && 2 * n_units > n_cus : form == Form::kSpec && n_cus > 0 && n_units > n_cus && hspec_aligned)) {
        pl.variant = Variant::kPersistRows;
        pl.grid_x = n_cus;
        pl.grid_y = 1;
        return pl;
    }
    pl.variant = xfade ? Variant::kXfade : simple ? Variant::kSimple : Variant::kLoop;
    pl.tab_ok = simple;
    return pl;
}

// ---- the one-block log-mel launches (k_conv / k_conv_spec <.., MEL>): one workgroup per (unit, ear) row, no parts, no unit table ---
// ss2: 0 = the one-block row of ssroute::obs_logmel_shape_ok; SoundSpaces 2.0 steps (ssroute::obs_logmel_ss2_shape, fp32 rows of
// one allocation): 1 = the cross-faded one-block row, 2 = the WIDE row (block 0 of a longer row, with or without the cross-fade).
// n_buckets: the launch's (ConvParams::n_buckets).  The loop-free kernel: one term, one RIR block, bucket 0 only.
inline ConvPlan plan_conv_mel(Form form, int ss2, int flags, int rir_cap, int h_blocks, int n_buckets, int fade_len, int n_units) {
    ConvPlan pl;
    const bool time = form == Form::kRows || form == Form::kRows16;
    const bool xfade = (flags & SS_FLAG_CROSSFADE) != 0;
    if (ss2 && (form != Form::kRows || (xfade && (fade_len < 1 || fade_len > 2 * ssk::kPrevPairs - 2)))) {
        pl.rc = SS_EINVAL;
        return pl;
    }
    pl.grid_x = 2 * n_units;
    pl.bucket0 = n_buckets == 1 || (flags & SS_FLAG_FIRST_BUCKET);
    const bool simple = (flags & SS_FLAG_NO_DISTRACTOR) && (time ? rir_cap <= kB : h_blocks == 1) && pl.bucket0;
    pl.variant = ss2 == 2 ? (xfade ? Variant::kWideXfade : Variant::kWide) : ss2 ? Variant::kXfade : simple ? Variant::kSimple : Variant::kLoop;
    return pl;
}

// ---- per-stream scratch (the k_obs_rows stash, the k_obs_blocks hand-off area) under a graph capture ----------------------------
// An allocation cannot be part of a capture: a launch that finds its scratch large enough uses it, capturing or not; one that
// would have to allocate (or grow) does so on a plain stream and is refused on a capturing one - ss_stream_reserve, or one
// eager call of the same shape, prepares the stream beforehand.
enum class Scratch { kUse, kAllocate, kRefuse };
inline Scratch scratch_decision(bool capturing, size_t have_bytes, size_t need_bytes) {
    if (have_bytes >= need_bytes) return Scratch::kUse;
    return capturing ? Scratch::kRefuse : Scratch::kAllocate;
}

// ---- k_obs_blocks: one workgroup per OUTPUT BLOCK of a row ---------------------------------------------------------------------
constexpr int kSyncRows = 512;        // (unit, ear) rows a k_obs_blocks launch may have: more than CUs / 2
// the hand-off area of `rows` rows: [rows][2] tails of kTailFloats floats + as many flag words
inline size_t handoff_floats(int rows) { return static_cast<size_t>(rows) * 2 * ssk::kTailFloats; }
inline size_t handoff_flags(int rows) { return static_cast<size_t>(rows) * 2; }
// ... in bytes, with the replay epoch word behind the flags (k_sync_next)
inline size_t handoff_bytes(int rows) {
    return handoff_floats(rows) * sizeof(float) + handoff_flags(rows) * sizeof(int) + sizeof(int);
}

// ss_stream_reserve's argument rule (before a device is touched): a row of 2 or 3 partition blocks, a bank capacity, one or two
// terms per unit.  stream_ok: not the per-thread stream (it can own no scratch).
inline bool reserve_args_ok(bool stream_ok, int out_len, int rir_cap, int n_terms) {
    return stream_ok && out_len > kB && out_len <= 3 * kB && rir_cap >= 1 && (n_terms == 1 || n_terms == 2);
}

struct ObsBlocksPlan {
    bool ok = false;                  // false: the launch does not qualify (the caller falls through to k_obs_rows)
    int parts_log2 = 0, nb = 0, grid = 1, n_terms = 2;
    size_t handoff_floats = 0, handoff_flags = 0;       // what this launch's rows use of the hand-off area
};

// Small steps of rows longer than one block (the reference's Replica arrangement: 5 envs per GPU at 44.1 kHz): one workgroup
// per OUTPUT BLOCK of a row instead of one per row (k_obs_blocks) - while the whole grid fits the launch's share of the chip at
// one workgroup per CU, which is also what makes the kernel's inter-workgroup hand-off safe.  Spare CUs go to parts (the STFT
// phase of a block split 2 / 4 / 8 ways: the budget alone decides, no switch forces them).
// stream_ok: the stream can own a hand-off area (not the per-thread stream).
inline ObsBlocksPlan plan_obs_blocks(int flags, int out_len, int n_valid, int n_units, int n_cus, int share, bool stream_ok,
                                     const Switches& sw) {
    ObsBlocksPlan pl;
    const int n_rows = 2 * n_units, nb = (out_len + kB - 1) / kB;
    const int budget = n_cus / (share > 1 ? share : 1);
    if (sw.no_obs_blocks || (flags & SS_FLAG_CROSSFADE) || n_valid != out_len || nb < 2 || nb > 3 || n_rows * nb > budget ||
        n_rows > kSyncRows || !stream_ok)
        return pl;
    int k = 0;
    while (k < 3 && ((n_rows * nb) << (k + 1)) <= budget) ++k;
    pl.ok = true;
    pl.parts_log2 = k;
    pl.nb = nb;
    pl.grid = (n_rows * nb) << k;
    pl.n_terms = (flags & SS_FLAG_NO_DISTRACTOR) ? 1 : 2;
    pl.handoff_floats = handoff_floats(n_rows);
    pl.handoff_flags = handoff_flags(n_rows);
    return pl;
}

// ---- the row kernels (k_obs_blocks / k_obs_rows): the bank form a launch reads ---------------------------------------------------
// half: a half spectral bank.  Half buckets: a launch that only touches bucket 0 (one bucket, or SS_FLAG_FIRST_BUCKET) is a
// single-allocation launch on bucket 0's arrays (Form::kSpec16: the caller sets ConvParams::n_buckets = 1).
inline Form rows_form(bool spectral, bool half, bool rows16, int n_buckets, int flags) {
    if (!spectral) return rows16 ? Form::kRows16 : Form::kRows;
    if (!half) return Form::kSpec;
    return n_buckets > 1 && !(flags & SS_FLAG_FIRST_BUCKET) ? Form::kSpec16Buckets : Form::kSpec16;
}

// ---- k_obs_rows: persistent workgroups walk the (unit, ear) rows ---------------------------------------------------------------
struct ObsRowsPlan {
    int rc = 0;                       // SS_EINVAL: refused, nothing else is set
    int parts_log2 = 0, grid = 1, nb_y = 0, n_terms = 2;
    int stash_nbh = 0, stash_terms = 0;
    size_t stash_bytes = 0;           // grid x stash_terms x stash_nbh block spectra (time-domain banks; 0: no stash)
};

// the deepest bucket's RIR blocks: what a workgroup's stash holds per term
template <class P>
inline int rows_nbh_max(const P& p) {
    int nbh_max = (p.rir_cap + kB - 1) / kB;
    for (int b = 0; b + 1 < p.n_buckets; ++b) nbh_max = nbh_max > (p.bk[b].cap + kB - 1) / kB ? nbh_max : (p.bk[b].cap + kB - 1) / kB;
    return nbh_max;
}

// spectral: the launch reads block spectra; plain_only: the log-mel, half and half-rows forms (no cross-fade);
// one_bank_only: the forms of one allocation (half spectra outside the bucketed form, half rows)
inline ObsRowsPlan plan_obs_rows(bool spectral, bool plain_only, bool one_bank_only, int flags, int n_valid, int n_buckets,
                                 int nbh_max, int n_units, int n_cus, int share, const Switches& sw) {
    ObsRowsPlan pl;
    const int n_rows = 2 * n_units;
    const bool xfade = (flags & SS_FLAG_CROSSFADE) != 0;
    pl.n_terms = (flags & SS_FLAG_NO_DISTRACTOR) ? 1 : 2;
    if ((plain_only && xfade) || (one_bank_only && n_buckets != 1) || (xfade && (spectral || pl.n_terms != 2))) {
        pl.rc = SS_EINVAL;
        return pl;
    }
    // small steps (the reference steps 5-10 envs per GPU at this rate): a row on 2 / 4 / 8 CUs, each rendering the row and
    // its share of every phase's pooled STFT blocks - only while every (row, part) still gets a workgroup of its own
    // Time-domain bank: every part also repeats the row's stash round trip (640 KiB per row), and the launch turns
    // memory-bound long before the CUs run out - same box, alternating, us per launch at 1 / 5 / 10 / 16 units with up to 8
    // parts per row: 58.7 / 62.2 / 69.5 / 75.4 against 70.8 / 71.1 / 72.1 / 72.6 with one (profiles/r5/kbench_parts_44k.txt) -
    // so the split stops at 96 workgroups there.  The spectral bank has no stash: -20 % up to 32 units (256 workgroups).
    pl.parts_log2 = parts_log2_for(n_rows, spectral ? n_cus : (n_cus < 96 ? n_cus : 96), share, sw.parts_log2);
    pl.grid = (n_rows << pl.parts_log2) < n_cus ? (n_rows << pl.parts_log2) : n_cus;
    pl.nb_y = n_valid == 0 ? 0 : nb_y_of(n_valid);
    // Time-domain bank: the kernel transforms every RIR block once per row and keeps the spectra that are needed again
    // in a per-workgroup stash (k_obs_rows); 44.1 kHz: 2 x 128 KiB written and 3 x 128 KiB read back per row.
    if (!spectral) {
        pl.stash_terms = pl.n_terms;                            // no distractor terms: half the stash
        pl.stash_nbh = nbh_max;
        const size_t per_wg = static_cast<size_t>(pl.stash_terms) * nbh_max * ssk::kSpecComplex * 2 * sizeof(float);
        pl.stash_bytes = per_wg * static_cast<size_t>(pl.grid);
    }
    return pl;
}

// ---- the feature kernels over a waveform: k_spectrogram (pooled blocks), k_logmel / k_gccphat / k_features (frame segments) ----
enum class Frames { kPooled, kSegments };
inline int groups_of(Frames kind, int len) {
    // kPooled: 4 pooled time blocks x 2 ears per round of a workgroup; kSegments: kSegFrames frames per round
    return kind == Frames::kPooled ? (t4_of(len) + 3) / 4 : (n_frames_of(len) + ssk::kSegFrames - 1) / ssk::kSegFrames;
}
struct FramesPlan {
    int n_frames = 0, t4 = 0, live = 0, groups = 0, gpw = 1, chunks = 1, grid = 1;
};
// n_valid: samples from n_valid on are KNOWN to be zero (len: nothing known).  wanted_gpw: the groups one workgroup should walk
// (large batches: tables staged once, next segment prefetched under the math; small batches keep one group per workgroup so
// that the launch still fills the chip), clamped to [1, groups]; one workgroup per (unit, chunk of gpw groups).
inline FramesPlan plan_frames(Frames kind, int n_units, int len, int n_valid, long long wanted_gpw) {
    FramesPlan pl;
    pl.n_frames = n_frames_of(len);
    pl.t4 = t4_of(len);
    pl.live = ssk::live_blocks(n_valid, len, pl.t4);
    pl.groups = groups_of(kind, len);
    pl.gpw = wanted_gpw < 1 ? 1 : wanted_gpw > pl.groups ? pl.groups : static_cast<int>(wanted_gpw);
    pl.chunks = (pl.groups + pl.gpw - 1) / pl.gpw;
    pl.grid = n_units * pl.chunks;
    return pl;
}
// k_features: resident workgroups share the (unit, group) rounds round-robin - at most max_wgs of them
inline int features_grid(int n_units, int len, long long max_wgs) {
    const long long tasks = static_cast<long long>(n_units) * groups_of(Frames::kSegments, len);
    return static_cast<int>(tasks < max_wgs ? tasks : max_wgs);
}

// ---- ConvParams: the shape fields and defaults every launch starts from (a template: the struct lives with the kernels) -------
template <class P>
inline void init_conv_params(P& p, int n_valid, int out_len) {
    p.n_valid = n_valid;
    p.out_len = out_len;
    p.n_frames = n_frames_of(out_len);
    p.t4 = t4_of(out_len);
    p.pad_mode = 0;
    p.fade_len = static_cast<int>(0.05 * out_len);     // crossfade_samples = int(0.05 * sr), rows are 1 s (out_len == sr)
    p.hspec = nullptr;
    p.h_blocks = 0;
    p.xcd_map = 0;
    p.nb_y = 1;
    p.stash = nullptr;
    p.stash_nbh = 0;
    p.stash_terms = 0;
    p.n_terms = 2;
    p.parts_log2 = 0;
    p.n_buckets = 1;
    using Bucket = std::remove_reference_t<decltype(p.bk[0])>;
    for (auto& b : p.bk) b = Bucket{nullptr, nullptr, 0x7fffffff, 0, 0, 0};
}

template <class P>
inline void apply(const ConvPlan& pl, P& p) {
    p.nb_y = pl.nb_y;
    p.parts_log2 = pl.parts_log2;
}
template <class P>
inline void apply(const ObsBlocksPlan& pl, P& p) {
    p.parts_log2 = pl.parts_log2;
    p.nb_y = pl.nb;
    p.n_terms = pl.n_terms;
    p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0;
}
// (the stash pointer: the caller's, once it holds pl.stash_bytes)
template <class P>
inline void apply(const ObsRowsPlan& pl, P& p) {
    p.parts_log2 = pl.parts_log2;
    p.nb_y = pl.nb_y;
    p.n_terms = pl.n_terms;
    p.stash = nullptr;
    p.stash_nbh = pl.stash_nbh;
    p.stash_terms = pl.stash_terms;
}

}  // namespace sslaunch
