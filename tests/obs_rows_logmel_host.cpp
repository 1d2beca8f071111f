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
    p.n_terms = no_distractor ? 1 : 2;
    p.parts_log2 = parts_log2;
    p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0;
    apply_bucket2(p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const int n_rows = 2 * n_units;
    if (blocks) {
        const int nb = (out_len + ssk::kB - 1) / ssk::kB, grid_b = (n_rows * nb) << parts_log2;
        p.nb_y = nb;
        p.xcd_map = 0;                                  // workgroups run in blockIdx order here: (row, j - 1) before (row, j)
        std::vector<float> tails(static_cast<size_t>(n_rows) * 2 * ssk::kTailFloats, 12345.0f);
        std::vector<int> fl(static_cast<size_t>(n_rows) * 2, 0);
        gridDim = dim3{(unsigned)grid_b, 1, 1};
        for (int b = 0; b < grid_b; ++b) {
            blockIdx = dim3{(unsigned)b, 0, 0};
            int rc = run_block(ssk::kT, [&] {
                if (spectral) ssk::k_obs_blocks<true, true>(p, n_rows, tails.data(), fl.data(), 7, m);
                else ssk::k_obs_blocks<false, true>(p, n_rows, tails.data(), fl.data(), 7, m);
            });
            if (rc) return rc;
        }
        return 0;
    }
    const int grid = parts_log2 ? (n_rows << parts_log2) : (wgs < n_rows ? wgs : n_rows);
    p.xcd_map = grid >= 8;
    p.nb_y = n_valid == 0 ? 0 : (n_valid + ssk::kB - 1) / ssk::kB;
    std::vector<float> stash;
    if (!spectral) {
        p.stash_nbh = (cap + ssk::kB - 1) / ssk::kB;
        p.stash_terms = p.n_terms;
        stash.assign(static_cast<size_t>(grid) * p.stash_terms * p.stash_nbh * 2 * ssk::kSpecComplex, 12345.0f);
        p.stash = reinterpret_cast<ssk::f32x4*>(stash.data());
    }
    gridDim = dim3{(unsigned)grid, 1, 1};
    for (int b = 0; b < grid; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (spectral) ssk::k_obs_rows<true, false, false, true>(p, n_rows, m);
            else ssk::k_obs_rows<false, false, false, true>(p, n_rows, m);
        });
        if (rc) return rc;
    }
    return 0;
}
