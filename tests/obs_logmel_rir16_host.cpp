// obs_logmel_rir16_host.cpp — TEST INFRASTRUCTURE: the log-mel instantiations of the fused observation kernels over HALF-PRECISION
// TIME-DOMAIN ROWS (ss_kernels.hpp: k_conv<.., MEL, HALF>, k_conv<.., MEL, HALF, RBK>, k_obs_rows<.., MEL, .., ROWS16>,
// k_obs_blocks<.., MEL, .., ROWS16>) compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its runner
// and tables are file-local), so tests/test_obs_logmel_rir16_host.py can compare each with its fp32 log-mel sibling fed the
// dequantised rows and with the float64 model.  The kernel choice is the library's (sslaunch::plan_conv_mel and ssdispatch of
// sound-spaces_amd/csrc, through run_conv_mel / run_obs_rows / run_obs_blocks of hostsim.cpp).  Never part of the product.
#include "hostsim/hostsim.cpp"

#include <limits>

// One launch over n_buckets <= 4 buckets (1: one allocation): bucket b holds global indices >= first[b] as rows of cap[b] samples -
// fp16 halves bank[b] with scales rscale[b] ([n, 2]) when half != 0, planar fp32 rows bank[b] otherwise.
// kernel: 0 = the one-block kernels, one workgroup per row (flags pick the instantiation as the library does: loop-free under
//             SS_FLAG_NO_DISTRACTOR with cap[0] <= kB on a launch that touches bucket 0 only - one bucket or SS_FLAG_FIRST_BUCKET -
//             else the loop kernel; bucketed launches that may touch every bucket: the RBK / fp32 bucketed loop kernel);
//         1 = k_obs_rows (`wgs` persistent workgroups; parts_log2 > 0: one workgroup per (row, part)), one allocation only;
//         2 = k_obs_blocks (one workgroup per output block of a row and part, in blockIdx order), one allocation only.
// *taken (may be null): 0 loop-free, 1 loop, 2 bucketed loop, 3 rows, 4 blocks.  out / sgram may be null.
extern "C" int hs_obs_logmel_rir16(int half, int kernel, const float* spec, const void* const* bank, const float* const* rscale,
                                   const int* first, const int* cap, int n_buckets, const int* rir_len, const int* desc, float* out,
                                   float* sgram, float* logmel, const int* mel_start, const float* mel_w, int n_mels, int max_len,
                                   float mel_eps, int n_units, int n_valid, int out_len, int pad_mode, int wgs, int parts_log2,
                                   int flags, int* taken) {
    if (n_buckets < 1 || n_buckets > ssk::kMaxBuckets || !logmel || n_valid < 0 || n_valid > out_len) return -1;
    if (kernel < 0 || kernel > 2 || (kernel != 0 && n_buckets != 1) || (flags & SS_FLAG_CROSSFADE)) return -2;
    if (kernel == 0 ? (out_len < ssk::kNfft / 2 + 1 || out_len > ssk::kB) : (out_len <= ssk::kB || out_len > 3 * ssk::kB)) return -3;
    if (kernel == 2 && n_valid != out_len) return -4;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1 || (kernel == 0 && parts_log2)) return -5;
    for (int b = 0; b < n_buckets; ++b)
        if (cap[b] < 2 || (cap[b] & 1) || ssroute::ceil_div(cap[b], ssk::kB) > 16 || (half && !rscale[b])) return -6;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    p.fade_len = 0;
    const float* rows[ssk::kMaxBuckets] = {nullptr, nullptr, nullptr, nullptr};
    for (int b = 0; b < n_buckets; ++b) rows[b] = static_cast<const float*>(bank[b]);     // (half: halves behind a float pointer)
    if (half) p.rir_cap = cap[0];
    else set_rows(p, rows[0], 2LL * cap[0], cap[0], 1, cap[0]);
    set_buckets(p, rows, nullptr, first, cap, n_buckets);
    ssk::RowScale<true, true> rs{static_cast<const ssk::h16x2*>(bank[0]), half ? rscale[0] : nullptr, {nullptr, nullptr, nullptr}};
    for (int b = 1; half && b < n_buckets; ++b) rs.bk[b - 1] = rscale[b];
    const ssk::RowScale<true> rs1 = ssdispatch::first_bucket(rs);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const Form form = half ? Form::kRows16 : Form::kRows;
    int dummy = 0;
    if (!taken) taken = &dummy;
    if (kernel == 0) {
        if (!half && (flags & SS_FLAG_FIRST_BUCKET)) p.n_buckets = 1;      // (the fp32 entries' own rule for such launches)
        sslaunch::ConvPlan pl;
        const int rc = run_conv_mel(form, p, m, 0, n_units, flags, nullptr, &rs, &pl);
        *taken = !pl.bucket0 ? 2 : pl.variant == sslaunch::Variant::kSimple ? 0 : 1;
        return rc;
    }
    if (kernel == 2) {
        *taken = 4;
        return run_obs_blocks(p, form, n_units, flags, parts_log2, &m, nullptr, &rs1);
    }
    *taken = 3;
    return run_obs_rows(p, form, n_units, flags, wgs, parts_log2, std::numeric_limits<float>::quiet_NaN(), &m, nullptr, &rs1);
}
