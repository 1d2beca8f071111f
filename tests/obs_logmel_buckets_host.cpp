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
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir = rows ? static_cast<const float*>(bank[0]) : nullptr;
    p.rir_unit_stride = rows ? 2LL * cap[0] : 0; p.rir_chan_stride = rows ? cap[0] : 0; p.rir_elem_stride = 1;
    p.rir_cap = rows ? cap[0] : 0;
    p.hspec = rows ? nullptr : static_cast<const ssk::f32x4*>(bank[0]);
    p.h_blocks = rows ? 0 : (cap[0] + ssk::kB - 1) / ssk::kB;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.xcd_map = 0; p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0; p.parts_log2 = parts_log2;
    p.n_terms = no_distractor ? 1 : 2;
    p.n_buckets = n_buckets;
    ssk::SpecScale<true, true> hs;
    hs.hscale = form == 2 ? hscale[0] : nullptr;
    int nbh_max = (cap[0] + ssk::kB - 1) / ssk::kB;
    for (int b = 0; b < ssk::kMaxBuckets - 1; ++b) {
        p.bk[b] = ssk::BankBucket{nullptr, nullptr, 0x7fffffff, 0, 0, 0};
        hs.bk[b] = nullptr;
    }
    for (int b = 1; b < n_buckets; ++b) {
        const int hb = (cap[b] + ssk::kB - 1) / ssk::kB;
        p.bk[b - 1] = ssk::BankBucket{rows ? static_cast<const float*>(bank[b]) : nullptr,
                                      rows ? nullptr : static_cast<const ssk::f32x4*>(bank[b]), first[b], cap[b], hb, 0};
        hs.bk[b - 1] = form == 2 ? hscale[b] : nullptr;
        nbh_max = hb > nbh_max ? hb : nbh_max;
    }
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const int n_rows = 2 * n_units;
    if (kernel == 0) {
        p.nb_y = 1;
        gridDim = dim3{(unsigned)n_rows, 1, 1};
        for (int b = 0; b < n_rows; ++b) {
            blockIdx = dim3{(unsigned)b, 0, 0};
            int rc = run_block(ssk::kT, [&] {
                if (form == 2) ssk::k_conv_spec<true, false, false, true, true, true>(p, m, hs);
                else if (form == 1) ssk::k_conv_spec<true, false, false, true>(p, m);
                else ssk::k_conv<true, false, false, false, false, true>(p, m);
            });
            if (rc) return rc;
        }
        return 0;
    }
    if (kernel == 2) {
        const int nb = (out_len + ssk::kB - 1) / ssk::kB, grid_b = (n_rows * nb) << parts_log2;
        p.nb_y = nb;
        std::vector<float> tails(static_cast<size_t>(n_rows) * 2 * ssk::kTailFloats, 12345.0f);
        std::vector<int> fl(static_cast<size_t>(n_rows) * 2, 0);
        gridDim = dim3{(unsigned)grid_b, 1, 1};
        for (int b = 0; b < grid_b; ++b) {              // (blockIdx order: (row, j - 1) before (row, j))
            blockIdx = dim3{(unsigned)b, 0, 0};
            int rc = run_block(ssk::kT, [&] {
                if (form == 1) ssk::k_obs_blocks<true, true>(p, n_rows, tails.data(), fl.data(), 7, m);
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
    if (rows) {                                         // as launch_obs_rows: the deepest bucket's blocks per term
        p.stash_nbh = nbh_max;
        p.stash_terms = p.n_terms;
        stash.assign(static_cast<size_t>(grid) * p.stash_terms * p.stash_nbh * 2 * ssk::kSpecComplex, 12345.0f);
        p.stash = reinterpret_cast<ssk::f32x4*>(stash.data());
    }
    gridDim = dim3{(unsigned)grid, 1, 1};
    for (int b = 0; b < grid; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (n_buckets == 1) {
                if (form == 1) ssk::k_obs_rows<true, false, false, true>(p, n_rows, m);
                else ssk::k_obs_rows<false, false, false, true>(p, n_rows, m);
            } else {
                if (form == 1) ssk::k_obs_rows<true, false, true, true>(p, n_rows, m);
                else ssk::k_obs_rows<false, false, true, true>(p, n_rows, m);
            }
        });
        if (rc) return rc;
    }
    return 0;
}
