// spec_buckets_host.cpp — TEST INFRASTRUCTURE: the loop kernel k_conv_spec over SPECTRAL LENGTH BUCKETS (ss_kernels.hpp;
// include/ss_hip.h "Spectral length buckets") compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole:
// its runner and tables are file-local), so tests/test_spec_buckets_host.py can compare the bucketed HALF instantiations
// (k_conv_spec<.., HALF, HBK>) with the fp32 bucketed instantiation fed the dequantised spectra, and the fp32 launch without
// time-domain rows with the both-forms one.  Never part of the product.
#include "hostsim/hostsim.cpp"

// One launch of the loop kernel (SIMPLE = false) over n_buckets <= 4 buckets: bucket b holds global indices >= first[b] as
// block spectra hspec[b] ([n, 2, ceil(cap[b]/kB), 32768] fp32, or fp16 with scales hscale[b] when half != 0).  rows (fp32 form
// only): NULL = the spectral-only launch (no row pointer anywhere in the arguments), else per-bucket time-domain rows as the
// both-forms bucketed launch carries them.  fuse != 0: the one-output-block kernel with the pooled spectrogram.
extern "C" int hs_conv_spec_buckets(int half, int fuse, const float* spec, const void* const* hspec, const float* const* hscale,
                                    const float* const* rows, const int* first, const int* cap, int n_buckets, const int* rir_len,
                                    const int* desc, float* out, float* sgram, int n_units, int n_valid, int out_len, int pad_mode) {
    const int nb_y = sslaunch::nb_y_of(n_valid);
    if (n_buckets < 1 || n_buckets > ssk::kMaxBuckets || nb_y > 3) return -1;
    if (fuse && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1)) return -2;
    if (half && rows) return -3;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    if (rows) set_rows(p, rows[0], 2LL * cap[0], cap[0], 1, cap[0]);
    set_spectra(p, hspec[0], ssroute::ceil_div(cap[0], ssk::kB));
    p.fade_len = 0;
    set_buckets(p, rows, hspec, first, cap, n_buckets);
    const ssk::SpecScale<true, true> hs = bucket_scales(half ? hscale : nullptr, n_buckets);
    // the loop kernel over every bucket (no SS_FLAG_FIRST_BUCKET), one workgroup per (row, output block): no parts
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(half ? sslaunch::Form::kSpec16Buckets : sslaunch::Form::kSpec, fuse, false, 0, p.rir_cap,
                                                      p.h_blocks, n_buckets, p.fade_len, false, false, n_units, nb_y, kBigChip, 1, forced_parts(0));
    if (pl.rc) return -1;
    sslaunch::apply(pl, p);
    return dispatch_conv(fuse, half ? Form::kSpec16Buckets : Form::kSpec, pl, p, n_units, nullptr, &hs);
}
