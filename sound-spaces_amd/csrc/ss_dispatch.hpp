// ss_dispatch.hpp — which kernel INSTANTIATION a planned launch runs: the one place that names the instantiations of k_conv,
// k_conv_spec, k_obs_rows and k_obs_blocks.  ss_route.hpp decides WHICH launch serves a step, ss_launch.hpp its geometry (and, as
// the plan's variant / bucket0, which member of the kernel family it wants); the switches below turn that plan into a template
// instantiation and hand it, with the plan's grid and the kernel's arguments, to a LAUNCHER the caller supplies:
//
//     int launcher(void (*kernel)(Args...), dim3 grid, args...)      // a workgroup is ssk::kT threads; returns a status
//
// The library's launcher enqueues the kernel on a stream (ss_hip.hip), the host simulator's runs the grid on fibers
// (tests/hostsim/hostsim.cpp) - so the CPU tests of the kernels run the instantiation the library runs for the same plan.
// A kernel travels as a plain function pointer: default arguments do not survive that, so every trailing UnitTab / SpecScale /
// RowScale / epoch_word argument is written out.  Template parameter orders (they differ between the families):
//     k_conv      <FUSE, SIMPLE, XFADE, TAB, WIDE, MEL, HALF, RBK>        k_conv_spec  <FUSE, SIMPLE, TAB, MEL, HALF, HBK>
//     k_obs_rows  <SPECTRAL, XFADE, BUCKETS, MEL, HALF, ROWS16>           k_obs_blocks <SPECTRAL, MEL, HALF, HBK, ROWS16>
// Bucketed half banks (Form::kSpec16Buckets, Form::kRows16 with several buckets): a launch that only touches bucket 0
// (plan.bucket0) is a single-allocation launch on bucket 0's arrays - the HALF kernels, the loop-free ones included; everything
// else runs the loop kernel that resolves the buckets (HBK / RBK).
#pragma once

#include "ss_kernels.hpp"
#include "ss_launch.hpp"

namespace ssdispatch {

using sslaunch::Form;
using V = sslaunch::Variant;
using ssk::ConvParams;

inline dim3 grid_of(int x, int y = 1) { return dim3{static_cast<unsigned>(x), static_cast<unsigned>(y), 1u}; }
// bucket 0 of a bucketed half bank as the single allocation it is to a bucket-0 launch
inline ssk::RowScale<true> first_bucket(const ssk::RowScale<true, true>& rs) { return ssk::RowScale<true>{rs.rir16, rs.rscale}; }
inline ssk::SpecScale<true> first_bucket(const ssk::SpecScale<true, true>& hs) { return ssk::SpecScale<true>{hs.hscale}; }

// ---- the convolution launches of sslaunch::plan_conv, fused with the STFT (FUSE) or not ------------------------------------------
// ut: the filled unit table, or nullptr (only where pl.tab_ok); hs: the scales of Form::kSpec16 / kSpec16Buckets; rs: those of
// Form::kRows16.  The persistent kernels have no fused form and the wide ones no unfused form: a plan that asks for one is refused.
template <bool FUSE, class L>
int conv(L&& launch, Form form, const sslaunch::ConvPlan& pl, const ConvParams& p, int n_units, const ssk::UnitTab<true>* ut,
         const ssk::SpecScale<true, true>* hs, const ssk::RowScale<true, true>* rs) {
    const dim3 grid = grid_of(pl.grid_x, pl.grid_y);
    const ssk::UnitTab<false> nt;
    const ssk::RowScale<false> nr;
    const ssk::SpecScale<false> ns;
    const bool simple = pl.variant == V::kSimple, tab = simple && ut;
    switch (form) {
        case Form::kRows:
            switch (pl.variant) {
                case V::kPersistRows:
                    if constexpr (!FUSE) return launch(ssk::k_conv_rows, grid, p, 2 * n_units);
                    break;
                case V::kWide:
                    if constexpr (FUSE) return launch(ssk::k_conv<true, false, false, false, true, false, false, false>, grid, p, nt, nr);
                    break;
                case V::kWideXfade:
                    if constexpr (FUSE) return launch(ssk::k_conv<true, false, true, false, true, false, false, false>, grid, p, nt, nr);
                    break;
                case V::kXfade: return launch(ssk::k_conv<FUSE, false, true, false, false, false, false, false>, grid, p, nt, nr);
                case V::kSimple:
                    if (tab) return launch(ssk::k_conv<FUSE, true, false, true, false, false, false, false>, grid, p, *ut, nr);
                    return launch(ssk::k_conv<FUSE, true, false, false, false, false, false, false>, grid, p, nt, nr);
                case V::kLoop: return launch(ssk::k_conv<FUSE, false, false, false, false, false, false, false>, grid, p, nt, nr);
            }
            break;
        case Form::kRows16:
            if (!pl.bucket0) return launch(ssk::k_conv<FUSE, false, false, false, false, false, true, true>, grid, p, nt, *rs);
            if (tab) return launch(ssk::k_conv<FUSE, true, false, true, false, false, true, false>, grid, p, *ut, first_bucket(*rs));
            if (simple) return launch(ssk::k_conv<FUSE, true, false, false, false, false, true, false>, grid, p, nt, first_bucket(*rs));
            return launch(ssk::k_conv<FUSE, false, false, false, false, false, true, false>, grid, p, nt, first_bucket(*rs));
        case Form::kSpec:
            if (pl.variant == V::kPersistRows) {
                if constexpr (!FUSE) return launch(ssk::k_conv_spec_rows, grid, p, 2 * n_units);
                break;
            }
            if (tab) return launch(ssk::k_conv_spec<FUSE, true, true, false, false, false>, grid, p, *ut, ns);
            if (simple) return launch(ssk::k_conv_spec<FUSE, true, false, false, false, false>, grid, p, nt, ns);
            return launch(ssk::k_conv_spec<FUSE, false, false, false, false, false>, grid, p, nt, ns);
        case Form::kSpec16:
        case Form::kSpec16Buckets:
            if (form == Form::kSpec16Buckets && !pl.bucket0)
                return launch(ssk::k_conv_spec<FUSE, false, false, false, true, true>, grid, p, nt, *hs);
            if (tab) return launch(ssk::k_conv_spec<FUSE, true, true, false, true, false>, grid, p, *ut, first_bucket(*hs));
            if (simple) return launch(ssk::k_conv_spec<FUSE, true, false, false, true, false>, grid, p, nt, first_bucket(*hs));
            return launch(ssk::k_conv_spec<FUSE, false, false, false, true, false>, grid, p, nt, first_bucket(*hs));
    }
    return SS_EINVAL;
}

// ---- the one-block log-mel launches of sslaunch::plan_conv_mel: one workgroup per row, no unit table ------------------------------
template <class L>
int conv_mel(L&& launch, Form form, const sslaunch::ConvPlan& pl, const ConvParams& p, const ssk::MelArgs& m,
             const ssk::SpecScale<true, true>* hs, const ssk::RowScale<true, true>* rs) {
    const dim3 grid = grid_of(pl.grid_x, pl.grid_y);
    const ssk::RowScale<false> nr;
    const ssk::SpecScale<false> ns;
    const bool simple = pl.variant == V::kSimple;
    switch (form) {
        case Form::kRows:
            switch (pl.variant) {
                case V::kSimple: return launch(ssk::k_conv<true, true, false, false, false, true, false, false>, grid, p, m, nr);
                case V::kLoop: return launch(ssk::k_conv<true, false, false, false, false, true, false, false>, grid, p, m, nr);
                case V::kXfade: return launch(ssk::k_conv<true, false, true, false, false, true, false, false>, grid, p, m, nr);
                case V::kWide: return launch(ssk::k_conv<true, false, false, false, true, true, false, false>, grid, p, m, nr);
                case V::kWideXfade: return launch(ssk::k_conv<true, false, true, false, true, true, false, false>, grid, p, m, nr);
                case V::kPersistRows: break;
            }
            break;
        case Form::kRows16:
            if (!pl.bucket0) return launch(ssk::k_conv<true, false, false, false, false, true, true, true>, grid, p, m, *rs);
            if (simple) return launch(ssk::k_conv<true, true, false, false, false, true, true, false>, grid, p, m, first_bucket(*rs));
            return launch(ssk::k_conv<true, false, false, false, false, true, true, false>, grid, p, m, first_bucket(*rs));
        case Form::kSpec:
            if (simple) return launch(ssk::k_conv_spec<true, true, false, true, false, false>, grid, p, m, ns);
            return launch(ssk::k_conv_spec<true, false, false, true, false, false>, grid, p, m, ns);
        case Form::kSpec16:
        case Form::kSpec16Buckets:
            if (form == Form::kSpec16Buckets && !pl.bucket0)
                return launch(ssk::k_conv_spec<true, false, false, true, true, true>, grid, p, m, *hs);
            if (simple) return launch(ssk::k_conv_spec<true, true, false, true, true, false>, grid, p, m, first_bucket(*hs));
            return launch(ssk::k_conv_spec<true, false, false, true, true, false>, grid, p, m, first_bucket(*hs));
    }
    return SS_EINVAL;
}

// ---- the row kernels for rows of 2 or 3 partition blocks ---------------------------------------------------------------------------
// form: sslaunch::rows_form's; mel: the log-mel instantiations, or nullptr; hs: the scales of the half spectral forms; rs: those
// of Form::kRows16 (one allocation).  `p` arrives finished: plan applied, stash / hand-off pointers from the caller's scratch.
template <bool MEL, class L>
int obs_rows_as(L&& launch, Form form, bool xfade, int grid_x, const ConvParams& p, int n_rows, const ssk::UnitTab<false, MEL>& ut,
                const ssk::SpecScale<true, true>* hs, const ssk::RowScale<true>* rs) {
    const dim3 grid = grid_of(grid_x);
    const ssk::RowScale<false> nr;
    const ssk::SpecScale<false> ns;
    // one bank allocation (every launch but those of a length-bucketed store): the instantiation without the bucket descriptors
    const bool buckets = p.n_buckets != 1;
    switch (form) {
        case Form::kRows:
            if (xfade) {                                        // (the cross-fade: fp32 time-domain rows, no log-mel form)
                if constexpr (!MEL) return launch(ssk::k_obs_rows<false, true, true, false, false, false>, grid, p, n_rows, ut, ns, nr);
                break;
            }
            if (buckets) return launch(ssk::k_obs_rows<false, false, true, MEL, false, false>, grid, p, n_rows, ut, ns, nr);
            return launch(ssk::k_obs_rows<false, false, false, MEL, false, false>, grid, p, n_rows, ut, ns, nr);
        case Form::kRows16: return launch(ssk::k_obs_rows<false, false, false, MEL, false, true>, grid, p, n_rows, ut, ns, *rs);
        case Form::kSpec:
            if (xfade) break;
            if (buckets) return launch(ssk::k_obs_rows<true, false, true, MEL, false, false>, grid, p, n_rows, ut, ns, nr);
            return launch(ssk::k_obs_rows<true, false, false, MEL, false, false>, grid, p, n_rows, ut, ns, nr);
        case Form::kSpec16: return launch(ssk::k_obs_rows<true, false, false, MEL, true, false>, grid, p, n_rows, ut, first_bucket(*hs), nr);
        case Form::kSpec16Buckets: return launch(ssk::k_obs_rows<true, false, true, MEL, true, false>, grid, p, n_rows, ut, *hs, nr);
    }
    return SS_EINVAL;
}
template <class L>
int obs_rows(L&& launch, Form form, bool xfade, int grid_x, const ConvParams& p, int n_rows, const ssk::MelArgs* mel,
             const ssk::SpecScale<true, true>* hs, const ssk::RowScale<true>* rs) {
    if (mel) return obs_rows_as<true>(launch, form, xfade, grid_x, p, n_rows, *mel, hs, rs);
    return obs_rows_as<false>(launch, form, xfade, grid_x, p, n_rows, ssk::UnitTab<false>(), hs, rs);
}

// k_obs_blocks: tails / flags: the hand-off area; epoch: the launch's, or with epoch_word != nullptr read from that word
template <bool MEL, class L>
int obs_blocks_as(L&& launch, Form form, int grid_x, const ConvParams& p, int n_rows, float* tails, int* flags, int epoch,
                  const ssk::UnitTab<false, MEL>& ut, const ssk::SpecScale<true, true>* hs, const ssk::RowScale<true>* rs,
                  const int* epoch_word) {
    const dim3 grid = grid_of(grid_x);
    const ssk::RowScale<false> nr;
    const ssk::SpecScale<false> ns;
    switch (form) {
        case Form::kRows: return launch(ssk::k_obs_blocks<false, MEL, false, false, false>, grid, p, n_rows, tails, flags, epoch, ut, ns, nr, epoch_word);
        case Form::kRows16: return launch(ssk::k_obs_blocks<false, MEL, false, false, true>, grid, p, n_rows, tails, flags, epoch, ut, ns, *rs, epoch_word);
        case Form::kSpec: return launch(ssk::k_obs_blocks<true, MEL, false, false, false>, grid, p, n_rows, tails, flags, epoch, ut, ns, nr, epoch_word);
        case Form::kSpec16:
            return launch(ssk::k_obs_blocks<true, MEL, true, false, false>, grid, p, n_rows, tails, flags, epoch, ut, first_bucket(*hs), nr, epoch_word);
        case Form::kSpec16Buckets:
            return launch(ssk::k_obs_blocks<true, MEL, true, true, false>, grid, p, n_rows, tails, flags, epoch, ut, *hs, nr, epoch_word);
    }
    return SS_EINVAL;
}
template <class L>
int obs_blocks(L&& launch, Form form, int grid_x, const ConvParams& p, int n_rows, float* tails, int* flags, int epoch,
               const ssk::MelArgs* mel, const ssk::SpecScale<true, true>* hs, const ssk::RowScale<true>* rs, const int* epoch_word) {
    if (mel) return obs_blocks_as<true>(launch, form, grid_x, p, n_rows, tails, flags, epoch, *mel, hs, rs, epoch_word);
    return obs_blocks_as<false>(launch, form, grid_x, p, n_rows, tails, flags, epoch, ssk::UnitTab<false>(), hs, rs, epoch_word);
}

}  // namespace ssdispatch
