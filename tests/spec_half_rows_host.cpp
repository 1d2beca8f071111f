// spec_half_rows_host.cpp — TEST INFRASTRUCTURE: the half-bank instantiations of the fused row kernels for rows of 2 or 3 partition
// blocks (k_obs_blocks<true, MEL, HALF> and k_obs_rows<true, false, false, MEL, HALF>, ss_kernels.hpp) compiled for the host on the
// fibers of tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local), so tests/test_spec_half_rows_host.py
// can compare them with the fp32 instantiations of the same templates fed the dequantised spectra.  Never part of the product.
#include "hostsim/hostsim.cpp"

// half != 0: `bank` = fp16 block spectra [R][2][h_blocks][8192] h16x4 and hscale their scales; half == 0: `bank` = fp32 block
// spectra [R][2][h_blocks][8192] f32x4 (hscale unused) - the same parameters otherwise.
// blocks != 0: k_obs_blocks (one workgroup per output block of a row and part, in ascending block order: producers before
// consumers), else k_obs_rows with `wgs` persistent workgroups (parts_log2 > 0: one workgroup per (row, part)).
// mel != 0: the log-mel instantiation (out / sgram may then be null); mel == 0: sgram is required, out may be null.
extern "C" int hs_obs_rows_spec_ab(int half, int blocks, int mel, const float* spec, const void* bank, const float* hscale,
                                   const int* rir_len, const int* desc, float* out, float* sgram, float* logmel, const int* mel_start,
                                   const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int h_blocks, int n_valid,
                                   int out_len, int pad_mode, int wgs, int parts_log2, int no_distractor) {
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB || n_valid > out_len || n_valid < 0) return -1;
    if (mel ? !logmel : !sgram) return -1;
    if (half && !hscale) return -1;
    if (blocks && n_valid != out_len) return -3;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1 || h_blocks < 1 || h_blocks > 16) return -2;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_spectra(p, bank, h_blocks);
    p.fade_len = 0;
    apply_bucket2(p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const ssk::SpecScale<true, true> hs{hscale, {nullptr, nullptr, nullptr}};
    const Form form = half ? Form::kSpec16 : Form::kSpec;
    const int flags = no_distractor ? SS_FLAG_NO_DISTRACTOR : 0;
    if (blocks) return run_obs_blocks(p, form, n_units, flags, parts_log2, mel ? &m : nullptr, &hs);
    return run_obs_rows(p, form, n_units, flags, wgs, parts_log2, 12345.0f, mel ? &m : nullptr, &hs);
}
