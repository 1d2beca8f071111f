// stage_spectra_host.cpp — TEST INFRASTRUCTURE: k_stage_spectra (ss_kernels.hpp) compiled for the host on the fibers of
// tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local), so tests/test_stage_spectra_host.py can
// compare it with the host-sim spectral-bank entry hs_rir_spectra over the same rows.  Never part of the product.
#include "hostsim/hostsim.cpp"

extern "C" int hs_stage_spectra(const float* staged, long long staged_stride, int planar, const int* slots, const int* lens, int n,
                                float* hspec, int h_blocks, int* bank_len) {
    ssk::StageSpecParams p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.hspec = reinterpret_cast<ssk::f32x4*>(hspec); p.bank_len = bank_len;
    p.tb = host_tables();
    p.staged_stride = staged_stride; p.planar = planar; p.h_blocks = h_blocks;
    const long long frames = staged_stride / 2, hb_frames = static_cast<long long>(h_blocks) * ssk::kB;
    p.cap = static_cast<int>(frames < hb_frames ? frames : hb_frames);       // (as ss_bank_scatter_spectra_f32)
    return run_grid(h_blocks, n, ssk::kT, [&] { ssk::k_stage_spectra(p); });
}
