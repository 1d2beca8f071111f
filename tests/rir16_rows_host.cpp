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
    if (cap < 2 || (cap & 1) || (cap + ssk::kB - 1) / ssk::kB > 16) return -5;
    if (blocks && n_valid != out_len) return -3;
    if (parts_log2 < 0 || parts_log2 > 3 || wgs < 1) return -2;
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir = half ? nullptr : static_cast<const float*>(bank);
    p.rir_unit_stride = half ? 0 : 2LL * cap; p.rir_chan_stride = half ? 0 : cap; p.rir_elem_stride = 1; p.rir_cap = cap;
    p.hspec = nullptr; p.h_blocks = 0;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.n_terms = no_distractor ? 1 : 2;
    p.parts_log2 = parts_log2;
    p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0;
    apply_bucket2(p);
    const ssk::UnitTab<false> nt;
    const ssk::SpecScale<false> ns;
    const ssk::RowScale<true> rs{static_cast<const ssk::h16x2*>(bank), rscale};
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
                if (half) ssk::k_obs_blocks<false, false, false, false, true>(p, n_rows, tails.data(), fl.data(), 7, nt, ns, rs);
                else ssk::k_obs_blocks<false>(p, n_rows, tails.data(), fl.data(), 7);
            });
            if (rc) return rc;
        }
        return 0;
    }
    const int grid = parts_log2 ? (n_rows << parts_log2) : (wgs < n_rows ? wgs : n_rows);
    p.xcd_map = grid >= 8;
    p.nb_y = n_valid == 0 ? 0 : (n_valid + ssk::kB - 1) / ssk::kB;
    p.stash_terms = p.n_terms;                          // (as launch_obs_rows sizes it: from rir_cap and n_terms)
    p.stash_nbh = (cap + ssk::kB - 1) / ssk::kB;
    std::vector<float> stash(static_cast<size_t>(grid) * p.stash_terms * p.stash_nbh * 2 * ssk::kSpecComplex,
                             std::numeric_limits<float>::quiet_NaN());
    p.stash = reinterpret_cast<ssk::f32x4*>(stash.data());
    gridDim = dim3{(unsigned)grid, 1, 1};
    for (int b = 0; b < grid; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (half) ssk::k_obs_rows<false, false, false, false, false, true>(p, n_rows, nt, ns, rs);
            else ssk::k_obs_rows<false, false, false>(p, n_rows);
        });
        if (rc) return rc;
    }
    return 0;
}
