// spec_half_host.cpp — TEST INFRASTRUCTURE: the half-bank kernels (k_stage_spectra16 and k_conv_spec<.., HALF>, ss_kernels.hpp)
// compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local), so
// tests/test_spec_half_host.py can compare the quantiser with numpy and the consumer with the fp32 instantiations of the same
// template fed the dequantised spectra.  Never part of the product.
#include "hostsim/hostsim.cpp"

// as ss_bank_scatter_spectra16_f32
extern "C" int hs_stage_spectra16(const float* staged, long long staged_stride, int planar, const int* slots, const int* lens, int n,
                                  void* hspec16, float* hscale, int h_blocks, int* bank_len) {
    ssk::StageSpecParams p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.hspec = static_cast<ssk::f32x4*>(hspec16); p.bank_len = bank_len;
    p.tb = host_tables();
    p.staged_stride = staged_stride; p.planar = planar; p.h_blocks = h_blocks;
    const long long frames = staged_stride / 2, hb_frames = static_cast<long long>(h_blocks) * ssk::kB;
    p.cap = static_cast<int>(frames < hb_frames ? frames : hb_frames);
    p.hscale = hscale; p.ear_off = staged_stride >> 1; p.slot0 = 0; p.pair_loads = 1;
    gridDim = dim3{(unsigned)h_blocks, (unsigned)n, 1};
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < h_blocks; ++b) {
            blockIdx = dim3{(unsigned)b, (unsigned)i, 0};
            int rc = run_block(ssk::kT, [&] { ssk::k_stage_spectra16(p); });
            if (rc) return rc;
        }
    return 0;
}

// as ss_rir_spectra16_f32: a planar bank (entry stride us, ear stride cs, rows of cap frames), entry r to entry r
extern "C" int hs_rir_spectra16(const float* rir, void* hspec16, float* hscale, int n_entries, long long us, int cs, int cap) {
    ssk::StageSpecParams p;
    p.staged = rir; p.slots = nullptr; p.lens = nullptr; p.hspec = static_cast<ssk::f32x4*>(hspec16); p.bank_len = nullptr;
    p.tb = host_tables();
    p.staged_stride = us; p.planar = 1; p.h_blocks = (cap + ssk::kB - 1) / ssk::kB; p.cap = cap;
    p.hscale = hscale; p.ear_off = cs; p.slot0 = 0;
    p.pair_loads = !(reinterpret_cast<size_t>(rir) & 7) && !(us & 1) && !(cs & 1);
    gridDim = dim3{(unsigned)p.h_blocks, (unsigned)n_entries, 1};
    for (int i = 0; i < n_entries; ++i)
        for (int b = 0; b < p.h_blocks; ++b) {
            blockIdx = dim3{(unsigned)b, (unsigned)i, 0};
            int rc = run_block(ssk::kT, [&] { ssk::k_stage_spectra16(p); });
            if (rc) return rc;
        }
    return 0;
}

// k_conv_spec over a half bank (half != 0: `bank` = fp16 spectra, hscale their scales) or over an fp32 spectral bank (half == 0),
// the same parameters otherwise.  fuse / simple / mel select the instantiation; use_tab != 0 the unit-table form (SIMPLE, no mel).
extern "C" int hs_conv_spec_ab(int half, int fuse, int simple, int mel, int use_tab, const float* spec, const void* bank,
                               const float* hscale, const int* rir_len, const int* desc, float* out, float* sgram, float* logmel,
                               const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                               int h_blocks, int n_valid, int out_len, int pad_mode) {
    const int nb_y = n_valid == 0 ? 1 : (n_valid + ssk::kB - 1) / ssk::kB;
    if ((fuse || mel) && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1)) return -1;
    if (simple && (nb_y != 1 || h_blocks != 1)) return -2;
    if (mel && !fuse) return -3;
    if (use_tab && (!simple || mel || n_units > ssk::kTabUnits)) return -4;
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir = nullptr; p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir_unit_stride = 0; p.rir_chan_stride = 0; p.rir_elem_stride = 1; p.rir_cap = 0;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.hspec = static_cast<const ssk::f32x4*>(bank);
    p.h_blocks = h_blocks; p.xcd_map = 0; p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0; p.n_terms = 2; p.parts_log2 = 0;
    p.nb_y = nb_y;
    apply_bucket2(p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const ssk::SpecScale<true> hs{hscale};
    ssk::UnitTab<true> ut;
    if (use_tab)
        for (int k = 0; k < n_units; ++k) {                 // launch slot k renders unit n - 1 - k (as hs_conv32)
            const int i = n_units - 1 - k;
            const int* d = desc + 8 * i;
            const bool ok = d[0] >= 0 && d[2] <= 0 && d[2] + d[3] > 0;
            ut.tab[ssk::kTabWords * k] = ok ? d[0] : -1;
            ut.tab[ssk::kTabWords * k + 1] = ok ? d[1] - d[2] : 0;
            ut.tab[ssk::kTabWords * k + 2] = i;
        }
    const int grid = 2 * n_units * nb_y;
    gridDim = dim3{(unsigned)grid, 1, 1};
    const ssk::UnitTab<false> nt;
    for (int b = 0; b < grid; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (half) {
                if (mel) { if (simple) ssk::k_conv_spec<true, true, false, true, true>(p, m, hs); else ssk::k_conv_spec<true, false, false, true, true>(p, m, hs); }
                else if (use_tab) { if (fuse) ssk::k_conv_spec<true, true, true, false, true>(p, ut, hs); else ssk::k_conv_spec<false, true, true, false, true>(p, ut, hs); }
                else if (fuse) { if (simple) ssk::k_conv_spec<true, true, false, false, true>(p, nt, hs); else ssk::k_conv_spec<true, false, false, false, true>(p, nt, hs); }
                else { if (simple) ssk::k_conv_spec<false, true, false, false, true>(p, nt, hs); else ssk::k_conv_spec<false, false, false, false, true>(p, nt, hs); }
            } else {
                if (mel) { if (simple) ssk::k_conv_spec<true, true, false, true>(p, m); else ssk::k_conv_spec<true, false, false, true>(p, m); }
                else if (use_tab) { if (fuse) ssk::k_conv_spec<true, true, true>(p, ut); else ssk::k_conv_spec<false, true, true>(p, ut); }
                else if (fuse) { if (simple) ssk::k_conv_spec<true, true>(p); else ssk::k_conv_spec<true, false>(p); }
                else { if (simple) ssk::k_conv_spec<false, true>(p); else ssk::k_conv_spec<false, false>(p); }
            }
        });
        if (rc) return rc;
    }
    return 0;
}
