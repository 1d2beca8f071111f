// obs_rows_logmel_host.cpp — TEST INFRASTRUCTURE: the log-mel instantiations of the fused row kernels for rows of 2 or 3 partition
// blocks (k_obs_rows<.., MEL> and k_obs_blocks<.., MEL>, ss_kernels.hpp) compiled for the host on the fibers of
// tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local), so tests/test_obs_rows_logmel_host.py can compare
// them with the oracle.  Never part of the product.
#include "hostsim/hostsim.cpp"

// blocks != 0: k_obs_blocks (one workgroup per output block of a row and part, producers before consumers), else k_obs_rows with
// `wgs` persistent workgroups (parts_log2 > 0: one workgroup per (row, part), whatever `wgs` says).
// spectral != 0: `bank` is the spectral bank [R][2][h_blocks][8192] f32x4 (hs_rir_spectra), else planar rows [R][2][cap].
// out / sgram may be null.
extern "C" int hs_obs_rows_logmel(int blocks, int spectral, const float* spec, const float* bank, const int* rir_len, const int* desc,
                                  float* out, float* sgram, float* logmel, const int* mel_start, const float* mel_w, int n_mels,
                                  int max_len, float mel_eps, int n_units, int cap, int h_blocks, int n_valid, int out_len,
                                  int pad_mode, int wgs, int parts_log2, int no_distractor) {
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB || n_valid > out_len || n_valid < 0 || !logmel) return -1;
    if (blocks && n_valid != out_len) return -3;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1) return -2;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    if (spectral) set_spectra(p, bank, h_blocks);
    else set_rows(p, bank, 2LL * cap, cap, 1, cap);
    p.fade_len = 0;
    apply_bucket2(p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const int flags = no_distractor ? SS_FLAG_NO_DISTRACTOR : 0;
    const Form form = spectral ? Form::kSpec : Form::kRows;
    if (blocks) return run_obs_blocks(p, form, n_units, flags, parts_log2, &m);
    return run_obs_rows(p, form, n_units, flags, wgs, parts_log2, 12345.0f, &m);
}
