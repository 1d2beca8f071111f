// obs_logmel_buckets_host.cpp — TEST INFRASTRUCTURE: the log-mel instantiations of the fused observation kernels over a
// LENGTH-BUCKETED bank (ss_kernels.hpp: k_conv<loop, MEL>, k_conv_spec<loop, MEL>, k_conv_spec<.., MEL, HALF, HBK>,
// k_obs_rows<.., BUCKETS, MEL>, k_obs_blocks<.., MEL>) compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included
// whole: its runner and tables are file-local), so tests/test_obs_logmel_buckets_host.py can compare them with the oracle, with
// the single-allocation instantiations on a dense copy of the bank and with the float64 model.  Never part of the product.
#include "hostsim/hostsim.cpp"

// kernel: 0 = the one-block loop kernels (one workgroup per row), 1 = k_obs_rows (`wgs` persistent workgroups; parts_log2 > 0:
//         one workgroup per (row, part)), 2 = k_obs_blocks (one workgroup per output block of a row and part, in blockIdx order).
// form:   0 = time-domain rows bank[b] = [n, 2, cap[b]]; 1 = fp32 block spectra bank[b] = [n, 2, ceil(cap[b]/kB), 32768];
//         2 = fp16 block spectra with the scales hscale[b] (kernel 0 only).
// n_buckets <= 4 buckets, bucket b holds global indices >= first[b].  n_buckets == 1 on kernel 1 runs the single-allocation
// instantiation (BUCKETS = false), on the other kernels the same instantiation (they resolve buckets at run time); form 2 with one
// bucket is not offered (that is k_conv_spec<.., MEL, HALF> of tests/spec_half_host.cpp).  out / sgram may be null.
extern "C" int hs_obs_logmel_buckets(int kernel, int form, const float* spec, const void* const* bank, const float* const* hscale,
                                     const int* first, const int* cap, int n_buckets, const int* rir_len, const int* desc, float* out,
                                     float* sgram, float* logmel, const int* mel_start, const float* mel_w, int n_mels, int max_len,
                                     float mel_eps, int n_units, int n_valid, int out_len, int pad_mode, int wgs, int parts_log2,
                                     int no_distractor) {
    if (n_buckets < 1 || n_buckets > ssk::kMaxBuckets || !logmel || n_valid < 0 || n_valid > out_len) return -1;
    if (kernel < 0 || kernel > 2 || form < 0 || form > 2 || (form == 2 && (kernel != 0 || n_buckets < 2))) return -2;
    if (kernel == 0 ? (out_len < ssk::kNfft / 2 + 1 || out_len > ssk::kB) : (out_len <= ssk::kB || out_len > 3 * ssk::kB)) return -3;
    if (kernel == 2 && n_valid != out_len) return -4;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1 || (kernel == 0 && parts_log2)) return -5;
    const bool rows = form == 0;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    if (rows) set_rows(p, static_cast<const float*>(bank[0]), 2LL * cap[0], cap[0], 1, cap[0]);
    else set_spectra(p, bank[0], ssroute::ceil_div(cap[0], ssk::kB));
    p.fade_len = 0;
    set_buckets(p, rows ? reinterpret_cast<const float* const*>(bank) : nullptr, rows ? nullptr : bank, first, cap, n_buckets);
    const ssk::SpecScale<true, true> hs = bucket_scales(form == 2 ? hscale : nullptr, n_buckets);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const int flags = no_distractor ? SS_FLAG_NO_DISTRACTOR : 0;
    if (kernel == 0) {
        p.n_terms = no_distractor ? 1 : 2;
        return run_conv_mel(form == 2 ? Form::kSpec16Buckets : form == 1 ? Form::kSpec : Form::kRows, p, m, 0, n_units, flags, &hs);
    }
    const Form f = rows ? Form::kRows : Form::kSpec;
    if (kernel == 2) return run_obs_blocks(p, f, n_units, flags, parts_log2, &m);
    return run_obs_rows(p, f, n_units, flags, wgs, parts_log2, 12345.0f, &m);       // (the stash: the deepest bucket's blocks per term)
}
