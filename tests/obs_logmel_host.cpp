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
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir = spectral ? nullptr : bank;
    p.rir_unit_stride = spectral ? 0 : 2LL * cap; p.rir_chan_stride = spectral ? 0 : cap; p.rir_elem_stride = 1;
    p.rir_cap = spectral ? 0 : cap;
    p.hspec = spectral ? reinterpret_cast<const ssk::f32x4*>(bank) : nullptr;
    p.h_blocks = spectral ? h_blocks : 0;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.xcd_map = 0; p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0; p.n_terms = 2; p.parts_log2 = 0; p.nb_y = 1;
    apply_bucket2(p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    gridDim = dim3{(unsigned)(2 * n_units), 1, 1};
    for (int b = 0; b < 2 * n_units; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (spectral) {
                if (simple) ssk::k_conv_spec<true, true, false, true>(p, m);
                else ssk::k_conv_spec<true, false, false, true>(p, m);
            } else {
                if (simple) ssk::k_conv<true, true, false, false, false, true>(p, m);
                else ssk::k_conv<true, false, false, false, false, true>(p, m);
            }
        });
        if (rc) return rc;
    }
    return 0;
}
