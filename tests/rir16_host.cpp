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
    return run_grid(2, n_entries, 256, [&] { ssk::k_rows_half(p); });
}

// as ss_bank_scatter_rows16_f32
extern "C" int hs_scatter_rows16(const float* staged, long long staged_stride, const int* slots, const int* lens, int n, void* rir16,
                                 float* rscale, int cap, int* bank_len) {
    if (cap < 2 || (cap & 1) || staged_stride < 2LL * cap || (staged_stride & 1)) return -1;
    ssk::ScatterRows16Params p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.rir16 = static_cast<ssk::h16x2*>(rir16); p.rscale = rscale;
    p.bank_len = bank_len; p.staged_stride = staged_stride; p.cap = cap;
    return run_grid(n, 1, 256, [&] { ssk::k_scatter_rows16(p); });
}

// k_conv over a bank of half rows (half != 0: `bank` = fp16 [R][2][cap], rscale [R][2]) or over the planar fp32 bank [R][2][cap]
// (half == 0), the same parameters otherwise.  fuse / simple select the instantiation, use_tab != 0 the unit-table form (SIMPLE);
// parts_log2: 2^k workgroups per fused row.  Unfused rows of up to 3 output blocks (grid.y).
extern "C" int hs_conv_rir16_ab(int half, int fuse, int simple, int use_tab, const float* spec, const void* bank, const float* rscale,
                                const int* rir_len, const int* desc, float* out, float* sgram, int n_units, int cap, int n_valid,
                                int out_len, int pad_mode, int parts_log2) {
    const int nb_y = sslaunch::nb_y_of(n_valid);
    if (cap < 2 || (cap & 1) || ssroute::ceil_div(cap, ssk::kB) > 16 || nb_y > 3) return -5;
    if (fuse && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1 || !sgram)) return -1;
    if (simple && (nb_y != 1 || cap > ssk::kB)) return -2;
    if (use_tab && (!simple || n_units > ssk::kTabUnits)) return -4;
    if (parts_log2 < 0 || parts_log2 > 3 || (parts_log2 && !fuse)) return -3;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    if (half) p.rir_cap = cap;                          // (half rows: addressed through rs)
    else set_rows(p, static_cast<const float*>(bank), 2LL * cap, cap, 1, cap);
    p.fade_len = 0;
    apply_bucket2(p);
    // the caller chooses the kernel (simple); never the persistent one: the half form has none, the fp32 arm keeps the same grid
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(half ? sslaunch::Form::kRows16 : sslaunch::Form::kRows, fuse, false,
                                                      simple ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0, cap, 0, p.n_buckets, p.fade_len,
                                                      false, false, n_units, nb_y, kBigChip, 1, forced_parts(parts_log2));
    if (pl.rc) return -5;
    sslaunch::apply(pl, p);
    const ssk::RowScale<true, true> rs{static_cast<const ssk::h16x2*>(bank), rscale, {nullptr, nullptr, nullptr}};
    ssk::UnitTab<true> ut;
    if (use_tab) fill_tab_reversed(ut, desc, n_units);
    return dispatch_conv(fuse, half ? Form::kRows16 : Form::kRows, pl, p, n_units, use_tab ? &ut : nullptr, nullptr, &rs);
}
