// obs_logmel_host.cpp — TEST INFRASTRUCTURE: the log-mel instantiations of the fused observation kernels (k_conv<.., MEL> and
// k_conv_spec<.., MEL>, ss_kernels.hpp) compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its
// runner and tables are file-local), so tests/test_obs_logmel_host.py can compare them with the oracle.  Never part of the product.
#include "hostsim/hostsim.cpp"

// spectral != 0: `bank` is the spectral bank [R][2][h_blocks][8192] f32x4 (hs_rir_spectra), else planar rows [R][2][cap].
// simple != 0: the loop-free kernel.  out / sgram may be null; one workgroup per (unit, ear) row, as the library launches it.
extern "C" int hs_obs_logmel(int spectral, int simple, const float* spec, const float* bank, const int* rir_len, const int* desc,
                             float* out, float* sgram, float* logmel, const int* mel_start, const float* mel_w, int n_mels,
                             int max_len, float mel_eps, int n_units, int cap, int h_blocks, int n_valid, int out_len,
                             int pad_mode) {
    if (out_len < ssk::kNfft / 2 + 1 || out_len > ssk::kB || n_valid > out_len) return -1;
    if (simple && (spectral ? h_blocks != 1 : cap > ssk::kB)) return -2;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    if (spectral) set_spectra(p, bank, h_blocks);
    else set_rows(p, bank, 2LL * cap, cap, 1, cap);
    p.fade_len = 0;
    apply_bucket2(p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    // the caller chooses the kernel; the flags under which the library's plan chooses the same one
    return run_conv_mel(spectral ? Form::kSpec : Form::kRows, p, m, 0, n_units, simple ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0);
}
