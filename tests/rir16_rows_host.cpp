// rir16_rows_host.cpp — TEST INFRASTRUCTURE: the ROWS16 instantiations of the fused row kernels for rows of 2 or 3 partition
// blocks (k_obs_blocks<false, false, false, false, ROWS16> and k_obs_rows<false, false, false, false, false, ROWS16>,
// ss_kernels.hpp) compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its runner and tables are
// file-local), so tests/test_rir16_rows_host.py can compare them with the fp32 time-domain instantiations of the same templates
// fed the dequantised rows.  Never part of the product.
#include "hostsim/hostsim.cpp"

#include <limits>

// half != 0: `bank` = fp16 rows [R][2][cap] and rscale [R][2] their scales; half == 0: `bank` = the planar fp32 bank [R][2][cap]
// (rscale unused) - the same parameters otherwise.
// blocks != 0: k_obs_blocks (one workgroup per output block of a row and part, in ascending block order with xcd_map = 0:
// producers before consumers), else k_obs_rows with `wgs` persistent workgroups (parts_log2 > 0: one workgroup per (row, part))
// over a stash allocated here, [workgroup][term][RIR block] block spectra, filled with NaN.
// sgram is required, out may be null.
extern "C" int hs_obs_rows_rir16_ab(int half, int blocks, const float* spec, const void* bank, const float* rscale, const int* rir_len,
                                    const int* desc, float* out, float* sgram, int n_units, int cap, int n_valid, int out_len,
                                    int pad_mode, int wgs, int parts_log2, int no_distractor) {
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB || n_valid > out_len || n_valid < 0 || !sgram) return -1;
    if (half && !rscale) return -1;
    if (cap < 2 || (cap & 1) || ssroute::ceil_div(cap, ssk::kB) > 16) return -5;
    if (blocks && n_valid != out_len) return -3;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1) return -2;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    if (half) p.rir_cap = cap;                          // (half rows: addressed through rs, the stash sized from rir_cap)
    else set_rows(p, static_cast<const float*>(bank), 2LL * cap, cap, 1, cap);
    p.fade_len = 0;
    apply_bucket2(p);
    const ssk::RowScale<true> rs{static_cast<const ssk::h16x2*>(bank), rscale};
    const Form form = half ? Form::kRows16 : Form::kRows;
    const int flags = no_distractor ? SS_FLAG_NO_DISTRACTOR : 0;
    if (blocks) return run_obs_blocks(p, form, n_units, flags, parts_log2, nullptr, nullptr, &rs);
    return run_obs_rows(p, form, n_units, flags, wgs, parts_log2, std::numeric_limits<float>::quiet_NaN(), nullptr, nullptr, &rs);
}
