// scatter_rows16_max_host.cpp — TEST INFRASTRUCTURE: the two scatter kernels of the half-precision time-domain rows
// (k_scatter_rows16 and its one-pass form k_scatter_rows16_max, ss_kernels.hpp) compiled for the host on the fibers of
// tests/hostsim/hostsim.cpp (included whole: its runner is file-local), so tests/test_scatter_rows16_max_host.py can compare them
// with each other and with the numpy rule.  Never part of the product.
#include "hostsim/hostsim.cpp"

// as ss_bank_scatter_rows16_f32: one workgroup per row
extern "C" int hs_scatter_rows16(const float* staged, long long staged_stride, const int* slots, const int* lens, int n, void* rir16,
                                 float* rscale, int cap, int* bank_len) {
    if (cap < 2 || (cap & 1) || staged_stride < 2LL * cap || (staged_stride & 1)) return -1;
    ssk::ScatterRows16Params p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.rir16 = static_cast<ssk::h16x2*>(rir16); p.rscale = rscale;
    p.bank_len = bank_len; p.staged_stride = staged_stride; p.cap = cap;
    return run_grid(n, 1, 256, [&] { ssk::k_scatter_rows16(p); });
}

// as ss_bank_scatter_rows16_max_f32: grid (chunks of 512 frames, rows)
extern "C" int hs_scatter_rows16_max(const float* staged, long long staged_stride, const int* slots, const int* lens,
                                     const float* row_max, int n, void* rir16, float* rscale, int cap, int* bank_len) {
    if (cap < 2 || (cap & 1) || staged_stride < 2LL * cap || (staged_stride & 1) || !row_max) return -1;
    ssk::ScatterRows16MaxParams p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.row_max = row_max; p.rir16 = static_cast<ssk::h16x2*>(rir16);
    p.rscale = rscale; p.bank_len = bank_len; p.staged_stride = staged_stride; p.cap = cap;
    return run_grid((cap + 511) / 512, n, 256, [&] { ssk::k_scatter_rows16_max(p); });
}
