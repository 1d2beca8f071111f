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
        if (!bank[b] || (form && !hscale[b]) || cap[b] < 2 || (cap[b] + ssk::kB - 1) / ssk::kB > 16) return -4;
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir = nullptr; p.rir_unit_stride = 0; p.rir_chan_stride = 0; p.rir_elem_stride = 1; p.rir_cap = 0;
    p.hspec = static_cast<const ssk::f32x4*>(bank[0]);
    p.h_blocks = (cap[0] + ssk::kB - 1) / ssk::kB;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.n_terms = no_distractor ? 1 : 2;
    p.parts_log2 = parts_log2;
    p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0;
    p.n_buckets = n_buckets;
    ssk::SpecScale<true, true> hs;
    hs.hscale = form ? hscale[0] : nullptr;
    for (int b = 0; b < ssk::kMaxBuckets - 1; ++b) {
        p.bk[b] = ssk::BankBucket{nullptr, nullptr, 0x7fffffff, 0, 0, 0};
        hs.bk[b] = nullptr;
    }
    for (int b = 1; b < n_buckets; ++b) {
        p.bk[b - 1] = ssk::BankBucket{nullptr, static_cast<const ssk::f32x4*>(bank[b]), first[b], cap[b], (cap[b] + ssk::kB - 1) / ssk::kB, 0};
        hs.bk[b - 1] = form ? hscale[b] : nullptr;
    }
    const ssk::SpecScale<true> hs1{hs.hscale};
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const ssk::UnitTab<false> nt;
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
                if (form == 1) {
                    if (mel) ssk::k_obs_blocks<true, true, true, true>(p, n_rows, tails.data(), fl.data(), 7, m, hs);
                    else ssk::k_obs_blocks<true, false, true, true>(p, n_rows, tails.data(), fl.data(), 7, nt, hs);
                } else if (form == 2) {
                    if (mel) ssk::k_obs_blocks<true, true, true>(p, n_rows, tails.data(), fl.data(), 7, m, hs1);
                    else ssk::k_obs_blocks<true, false, true>(p, n_rows, tails.data(), fl.data(), 7, nt, hs1);
                } else {
                    if (mel) ssk::k_obs_blocks<true, true>(p, n_rows, tails.data(), fl.data(), 7, m);
                    else ssk::k_obs_blocks<true>(p, n_rows, tails.data(), fl.data(), 7);
                }
            });
            if (rc) return rc;
        }
        return 0;
    }
    const int grid = parts_log2 ? (n_rows << parts_log2) : (wgs < n_rows ? wgs : n_rows);
    p.xcd_map = grid >= 8;
    p.nb_y = n_valid == 0 ? 0 : (n_valid + ssk::kB - 1) / ssk::kB;
    gridDim = dim3{(unsigned)grid, 1, 1};
    for (int b = 0; b < grid; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (form == 1) {
                if (mel) ssk::k_obs_rows<true, false, true, true, true>(p, n_rows, m, hs);
                else ssk::k_obs_rows<true, false, true, false, true>(p, n_rows, nt, hs);
            } else if (form == 2) {
                if (mel) ssk::k_obs_rows<true, false, false, true, true>(p, n_rows, m, hs1);
                else ssk::k_obs_rows<true, false, false, false, true>(p, n_rows, nt, hs1);
            } else {
                if (mel) ssk::k_obs_rows<true, false, true, true>(p, n_rows, m);
                else ssk::k_obs_rows<true, false, true>(p, n_rows);
            }
        });
        if (rc) return rc;
    }
    return 0;
}
