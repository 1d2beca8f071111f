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
    return run_grid(h_blocks, n, ssk::kT, [&] { ssk::k_stage_spectra16(p); });
}

// as ss_rir_spectra16_f32: a planar bank (entry stride us, ear stride cs, rows of cap frames), entry r to entry r
extern "C" int hs_rir_spectra16(const float* rir, void* hspec16, float* hscale, int n_entries, long long us, int cs, int cap) {
    ssk::StageSpecParams p;
    p.staged = rir; p.slots = nullptr; p.lens = nullptr; p.hspec = static_cast<ssk::f32x4*>(hspec16); p.bank_len = nullptr;
    p.tb = host_tables();
    p.staged_stride = us; p.planar = 1; p.h_blocks = ssroute::ceil_div(cap, ssk::kB); p.cap = cap;
    p.hscale = hscale; p.ear_off = cs; p.slot0 = 0;
    p.pair_loads = !(reinterpret_cast<size_t>(rir) & 7) && !(us & 1) && !(cs & 1);
    return run_grid(p.h_blocks, n_entries, ssk::kT, [&] { ssk::k_stage_spectra16(p); });
}

// k_conv_spec over a half bank (half != 0: `bank` = fp16 spectra, hscale their scales) or over an fp32 spectral bank (half == 0),
// the same parameters otherwise.  fuse / simple / mel select the instantiation; use_tab != 0 the unit-table form (SIMPLE, no mel).
extern "C" int hs_conv_spec_ab(int half, int fuse, int simple, int mel, int use_tab, const float* spec, const void* bank,
                               const float* hscale, const int* rir_len, const int* desc, float* out, float* sgram, float* logmel,
                               const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                               int h_blocks, int n_valid, int out_len, int pad_mode) {
    const int nb_y = sslaunch::nb_y_of(n_valid);
    if ((fuse || mel) && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1)) return -1;
    if (simple && (nb_y != 1 || h_blocks != 1)) return -2;
    if (mel && !fuse) return -3;
    if (use_tab && (!simple || mel || n_units > ssk::kTabUnits)) return -4;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_spectra(p, bank, h_blocks);
    p.fade_len = 0;
    apply_bucket2(p);
    // the caller chooses the kernel (simple); one workgroup per (row, output block): no parts, never the persistent kernel
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(half ? sslaunch::Form::kSpec16 : sslaunch::Form::kSpec, fuse, false,
                                                      simple ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0, 0, h_blocks, p.n_buckets, p.fade_len,
                                                      false, false, n_units, nb_y, kBigChip, 1, forced_parts(0));
    if (pl.rc) return -1;
    sslaunch::apply(pl, p);
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    const ssk::SpecScale<true, true> hs{hscale, {nullptr, nullptr, nullptr}};
    const Form form = half ? Form::kSpec16 : Form::kSpec;
    if (mel) return run_conv_mel(form, p, m, 0, n_units, simple ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0, &hs);
    ssk::UnitTab<true> ut;
    if (use_tab) fill_tab_reversed(ut, desc, n_units);
    return dispatch_conv(fuse, form, pl, p, n_units, use_tab ? &ut : nullptr, &hs);
}
