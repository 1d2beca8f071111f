// spec_half_bucket_rows_host.cpp — TEST INFRASTRUCTURE: the fused row kernels for rows of 2 or 3 partition blocks over a HALF
// bank in LENGTH BUCKETS (k_obs_rows<true, false, BUCKETS, MEL, HALF> and k_obs_blocks<true, MEL, HALF, HBK>, ss_kernels.hpp)
// compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local), so
// tests/test_spec_half_bucket_rows_host.py can compare them with the fp32 BUCKETS instantiations fed the dequantised spectra,
// with the single-allocation HALF instantiations and with the float64 model.  Never part of the product.
#include "hostsim/hostsim.cpp"

// form: 0 = fp32 block spectra in buckets, bank[b] = [n_b][2][ceil(cap[b]/kB)][8192] f32x4 (hscale unused): k_obs_rows<true, false,
//           true, MEL> / k_obs_blocks<true, MEL>;
//       1 = fp16 block spectra in buckets, bank[b] = the same count of h16x4, hscale[b] their scales: the bucketed half forms;
//       2 = fp16 block spectra of ONE allocation (n_buckets == 1): k_obs_rows<true, false, false, MEL, HALF> / k_obs_blocks<true, MEL, HALF>.
// n_buckets <= 4 buckets, bucket b holds global indices >= first[b].
// blocks != 0: k_obs_blocks (one workgroup per output block of a row and part, in ascending block order: producers before
// consumers), else k_obs_rows with `wgs` persistent workgroups (parts_log2 > 0: one workgroup per (row, part)).
// mel != 0: the log-mel instantiation (out / sgram may then be null); mel == 0: sgram is required, out may be null.
extern "C" int hs_obs_rows_half_buckets(int form, int blocks, int mel, const float* spec, const void* const* bank,
                                        const float* const* hscale, const int* first, const int* cap, int n_buckets, const int* rir_len,
                                        const int* desc, float* out, float* sgram, float* logmel, const int* mel_start,
                                        const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int n_valid, int out_len,
                                        int pad_mode, int wgs, int parts_log2, int no_distractor) {
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB || n_valid > out_len || n_valid < 0) return -1;
    if (mel ? !logmel : !sgram) return -1;
    if (form < 0 || form > 2 || n_buckets < 1 || n_buckets > ssk::kMaxBuckets || (form == 2 && n_buckets != 1)) return -2;
    if (blocks && n_valid != out_len) return -3;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1) return -2;
    for (int b = 0; b < n_buckets; ++b)
        if (!bank[b] || (form && !hscale[b]) || cap[b] < 2 || ssroute::ceil_div(cap[b], ssk::kB) > 16) return -4;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_spectra(p, bank[0], ssroute::ceil_div(cap[0], ssk::kB));
    p.fade_len = 0;
    set_buckets(p, nullptr, bank, first, cap, n_buckets);
    const ssk::SpecScale<true, true> hs = bucket_scales(form ? hscale : nullptr, n_buckets);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const int flags = no_distractor ? SS_FLAG_NO_DISTRACTOR : 0;
    // form 1 over ONE bucket is not the library's choice (rows_form: a single allocation, form 2): the bucketed half instantiations
    // all the same - the test compares the two on the same bank
    const Form f = form == 0 ? Form::kSpec : form == 1 ? Form::kSpec16Buckets : sslaunch::rows_form(true, true, false, n_buckets, flags);
    if (blocks) return run_obs_blocks(p, f, n_units, flags, parts_log2, mel ? &m : nullptr, &hs);
    return run_obs_rows(p, f, n_units, flags, wgs, parts_log2, 12345.0f, mel ? &m : nullptr, &hs);
}
