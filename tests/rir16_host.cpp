// rir16_host.cpp — TEST INFRASTRUCTURE: the kernels of the half-precision time-domain rows (k_rows_half, k_scatter_rows16 and
// k_conv<.., HALF>, ss_kernels.hpp) compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole: its runner
// and tables are file-local), so tests/test_rir16_host.py can compare the producers with numpy and the consumer with the fp32
// instantiations of the same template fed the dequantised rows.  Never part of the product.
#include "hostsim/hostsim.cpp"

// as ss_rir_rows16_f32: a planar fp32 bank (entry stride us, ear stride cs, rows of cap samples), entry r to entry r
extern "C" int hs_rows_half(const float* rir, void* rir16, float* rscale, int n_entries, long long us, int cs, int cap) {
    if (cap < 2 || (cap & 1)) return -1;
    ssk::RowsHalfParams p;
    p.rir = rir; p.rir16 = static_cast<ssk::h16x2*>(rir16); p.rscale = rscale; p.unit_stride = us; p.chan_stride = cs; p.cap = cap;
    gridDim = dim3{2, (unsigned)n_entries, 1};
    for (int r = 0; r < n_entries; ++r)
        for (int c = 0; c < 2; ++c) {
            blockIdx = dim3{(unsigned)c, (unsigned)r, 0};
            int rc = run_block(256, [&] { ssk::k_rows_half(p); });
            if (rc) return rc;
        }
    return 0;
}

// as ss_bank_scatter_rows16_f32
extern "C" int hs_scatter_rows16(const float* staged, long long staged_stride, const int* slots, const int* lens, int n, void* rir16,
                                 float* rscale, int cap, int* bank_len) {
    if (cap < 2 || (cap & 1) || staged_stride < 2LL * cap || (staged_stride & 1)) return -1;
    ssk::ScatterRows16Params p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.rir16 = static_cast<ssk::h16x2*>(rir16); p.rscale = rscale;
    p.bank_len = bank_len; p.staged_stride = staged_stride; p.cap = cap;
    gridDim = dim3{(unsigned)n, 1, 1};
    for (int i = 0; i < n; ++i) {
        blockIdx = dim3{(unsigned)i, 0, 0};
        int rc = run_block(256, [&] { ssk::k_scatter_rows16(p); });
        if (rc) return rc;
    }
    return 0;
}

// k_conv over a bank of half rows (half != 0: `bank` = fp16 [R][2][cap], rscale [R][2]) or over the planar fp32 bank [R][2][cap]
// (half == 0), the same parameters otherwise.  fuse / simple select the instantiation, use_tab != 0 the unit-table form (SIMPLE);
// parts_log2: 2^k workgroups per fused row.  Unfused rows of up to 3 output blocks (grid.y).
extern "C" int hs_conv_rir16_ab(int half, int fuse, int simple, int use_tab, const float* spec, const void* bank, const float* rscale,
                                const int* rir_len, const int* desc, float* out, float* sgram, int n_units, int cap, int n_valid,
                                int out_len, int pad_mode, int parts_log2) {
    const int nb_y = n_valid == 0 ? 1 : (n_valid + ssk::kB - 1) / ssk::kB;
    if (cap < 2 || (cap & 1) || (cap + ssk::kB - 1) / ssk::kB > 16 || nb_y > 3) return -5;
    if (fuse && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1 || !sgram)) return -1;
    if (simple && (nb_y != 1 || cap > ssk::kB)) return -2;
    if (use_tab && (!simple || n_units > ssk::kTabUnits)) return -4;
    if (parts_log2 < 0 || parts_log2 > 3 || (parts_log2 && !fuse)) return -3;
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir = half ? nullptr : static_cast<const float*>(bank);
    p.rir_unit_stride = half ? 0 : 2LL * cap; p.rir_chan_stride = half ? 0 : cap; p.rir_elem_stride = 1; p.rir_cap = cap;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.hspec = nullptr; p.h_blocks = 0; p.xcd_map = 0; p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0; p.n_terms = 2;
    p.parts_log2 = parts_log2;
    p.nb_y = nb_y;
    apply_bucket2(p);
    const ssk::RowScale<true> rs{static_cast<const ssk::h16x2*>(bank), rscale};
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
    const int gx = (2 * n_units) << parts_log2;
    gridDim = dim3{(unsigned)gx, (unsigned)nb_y, 1};
    const ssk::UnitTab<false> nt;
    for (int b = 0; b < gx * nb_y; ++b) {
        blockIdx = dim3{(unsigned)(b % gx), (unsigned)(b / gx), 0};
        int rc = run_block(ssk::kT, [&] {
            if (half) {
                if (use_tab) { if (fuse) ssk::k_conv<true, true, false, true, false, false, true>(p, ut, rs); else ssk::k_conv<false, true, false, true, false, false, true>(p, ut, rs); }
                else if (fuse) { if (simple) ssk::k_conv<true, true, false, false, false, false, true>(p, nt, rs); else ssk::k_conv<true, false, false, false, false, false, true>(p, nt, rs); }
                else { if (simple) ssk::k_conv<false, true, false, false, false, false, true>(p, nt, rs); else ssk::k_conv<false, false, false, false, false, false, true>(p, nt, rs); }
            } else {
                if (use_tab) { if (fuse) ssk::k_conv<true, true, false, true>(p, ut); else ssk::k_conv<false, true, false, true>(p, ut); }
                else if (fuse) { if (simple) ssk::k_conv<true, true>(p); else ssk::k_conv<true, false>(p); }
                else { if (simple) ssk::k_conv<false, true>(p); else ssk::k_conv<false, false>(p); }
            }
        });
        if (rc) return rc;
    }
    return 0;
}
