// rir16_buckets_host.cpp — TEST INFRASTRUCTURE: k_conv over HALF-PRECISION TIME-DOMAIN ROWS IN LENGTH BUCKETS (ss_kernels.hpp;
// include/ss_hip.h "Half-precision time-domain rows in length buckets") compiled for the host on the fibers of
// tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local), so tests/test_rir16_buckets_host.py can compare
// the bucketed half instantiation (k_conv<.., HALF, RBK>) with the fp32 bucketed k_conv fed the dequantised rows, and a bucket-0
// launch with the single-allocation half launch on bucket 0's arrays.  The launches are shaped by the library's own plan_conv.
// Never part of the product.
#include "hostsim/hostsim.cpp"

// One launch over n_buckets <= 4 buckets: bucket b holds global indices >= first[b] as rows of cap[b] samples - fp16 halves bank[b]
// with scales rscale[b] ([n, 2]) when half != 0, planar fp32 rows bank[b] otherwise.
// bucket0: 0 = the launch may touch every bucket (no flag: the loop kernel; half: the RBK instantiation);
//          1 = SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET, descriptors read from memory; 2 = ... through the unit table.
// fuse != 0: the one-output-block kernel with the pooled spectrogram.
extern "C" int hs_conv_rir16_buckets(int half, int fuse, int bucket0, const float* spec, const void* const* bank,
                                     const float* const* rscale, const int* first, const int* cap, int n_buckets, const int* rir_len,
                                     const int* desc, float* out, float* sgram, int n_units, int n_valid, int out_len, int pad_mode) {
    const int nb_y = sslaunch::nb_y_of(n_valid);
    if (n_buckets < 1 || n_buckets > ssk::kMaxBuckets || nb_y > 3) return -1;
    if (fuse && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1 || !sgram)) return -2;
    for (int b = 0; b < n_buckets; ++b)
        if (cap[b] < 2 || (cap[b] & 1) || ssroute::ceil_div(cap[b], ssk::kB) > 16) return -3;
    if (bucket0 == 2 && n_units > ssk::kTabUnits) return -4;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    p.fade_len = 0;
    const float* rows[ssk::kMaxBuckets] = {nullptr, nullptr, nullptr, nullptr};
    for (int b = 0; b < n_buckets; ++b) rows[b] = static_cast<const float*>(bank[b]);     // (half: halves behind a float pointer)
    if (half) p.rir_cap = cap[0];
    else set_rows(p, rows[0], 2LL * cap[0], cap[0], 1, cap[0]);
    set_buckets(p, rows, nullptr, first, cap, n_buckets);
    ssk::RowScale<true, true> rs{static_cast<const ssk::h16x2*>(bank[0]), half ? rscale[0] : nullptr, {nullptr, nullptr, nullptr}};
    for (int b = 1; half && b < n_buckets; ++b) rs.bk[b - 1] = rscale[b];
    const int flags = bucket0 ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0;
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(half ? sslaunch::Form::kRows16 : sslaunch::Form::kRows, fuse, false, flags, p.rir_cap, 0,
                                                      n_buckets, p.fade_len, false, false, n_units, nb_y, kBigChip, 1, forced_parts(0));
    if (pl.rc) return -5;
    if (pl.bucket0 != (bucket0 != 0 || n_buckets == 1)) return -6;
    sslaunch::apply(pl, p);
    if (pl.variant != sslaunch::Variant::kSimple && pl.variant != sslaunch::Variant::kLoop) return -7;
    ssk::UnitTab<true> ut;
    if (bucket0 == 2) fill_tab_reversed(ut, desc, n_units);
    // (-8: the unit table where the plan allows none)
    return dispatch_conv(fuse, half ? Form::kRows16 : Form::kRows, pl, p, n_units, bucket0 == 2 ? &ut : nullptr, nullptr, &rs);
}
