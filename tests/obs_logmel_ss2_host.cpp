// obs_logmel_ss2_host.cpp — TEST INFRASTRUCTURE: the log-mel instantiations of the fused loop kernel that serve SoundSpaces 2.0
// steps (k_conv<true, false, XFADE, false, WIDE, true>, ss_kernels.hpp: the cross-faded one-block row and the WIDE row with and
// without the cross-fade) compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its runner and tables
// are file-local), so tests/test_obs_logmel_ss2_host.py can compare them with the oracle.  Never part of the product.
#include "hostsim/hostsim.cpp"

// `bank`: planar rows [R][2][cap].  xfade != 0: SS_FLAG_CROSSFADE (term 1 of a unit = its previous RIR).  The shape picks the
// kernel as the library does: out_len <= kB needs the cross-fade, a longer row must be one the WIDE form serves.  out / sgram may
// be null; one workgroup per (unit, ear) row.
extern "C" int hs_obs_logmel_ss2(int xfade, const float* spec, const float* bank, const int* rir_len, const int* desc, float* out,
                                 float* sgram, float* logmel, const int* mel_start, const float* mel_w, int n_mels, int max_len,
                                 float mel_eps, int n_units, int cap, int n_valid, int out_len, int pad_mode) {
    if (out_len < ssk::kNfft / 2 + 1 || out_len > 3 * ssk::kB || n_valid < 0 || n_valid > out_len) return -1;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_rows(p, bank, 2LL * cap, cap, 1, cap);
    apply_bucket2(p);
    const bool wide = out_len > ssk::kB;
    if (wide && !ssroute::wide_one_block_ok(out_len, n_valid, 0, false, ssroute::Switches())) return -2;      // (the shape alone)
    if (!wide && !xfade) return -3;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    // (-4: a cross-fade ramp the kernels cannot keep - the plan's refusal)
    return run_conv_mel(Form::kRows, p, m, wide ? 2 : 1, n_units, xfade ? SS_FLAG_CROSSFADE : 0);
}
