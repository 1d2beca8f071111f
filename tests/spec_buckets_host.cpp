// spec_buckets_host.cpp — TEST INFRASTRUCTURE: the loop kernel k_conv_spec over SPECTRAL LENGTH BUCKETS (ss_kernels.hpp;
// include/ss_hip.h "Spectral length buckets") compiled for the host on the fibers of tests/hostsim/hostsim.cpp (included whole:
// its runner and tables are file-local), so tests/test_spec_buckets_host.py can compare the bucketed HALF instantiations
// (k_conv_spec<.., HALF, HBK>) with the fp32 bucketed instantiation fed the dequantised spectra, and the fp32 launch without
// time-domain rows with the both-forms one.  Never part of the product.
#include "hostsim/hostsim.cpp"

// One launch of the loop kernel (SIMPLE = false) over n_buckets <= 4 buckets: bucket b holds global indices >= first[b] as
// block spectra hspec[b] ([n, 2, ceil(cap[b]/kB), 32768] fp32, or fp16 with scales hscale[b] when half != 0).  rows (fp32 form
// only): NULL = the spectral-only launch (no row pointer anywhere in the arguments), else per-bucket time-domain rows as the
// both-forms bucketed launch carries them.  fuse != 0: the one-output-block kernel with the pooled spectrogram.
extern "C" int hs_conv_spec_buckets(int half, int fuse, const float* spec, const void* const* hspec, const float* const* hscale,
                                    const float* const* rows, const int* first, const int* cap, int n_buckets, const int* rir_len,
                                    const int* desc, float* out, float* sgram, int n_units, int n_valid, int out_len, int pad_mode) {
    const int nb_y = n_valid == 0 ? 1 : (n_valid + ssk::kB - 1) / ssk::kB;
    if (n_buckets < 1 || n_buckets > ssk::kMaxBuckets || nb_y > 3) return -1;
    if (fuse && (nb_y != 1 || out_len > ssk::kB || out_len < ssk::kNfft / 2 + 1)) return -2;
    if (half && rows) return -3;
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir = rows ? rows[0] : nullptr;
    p.rir_unit_stride = rows ? 2LL * cap[0] : 0; p.rir_chan_stride = rows ? cap[0] : 0; p.rir_elem_stride = 1; p.rir_cap = rows ? cap[0] : 0;
    p.n_valid = n_valid; p.out_len = out_len;
    p.n_frames = 1 + out_len / ssk::kHop;
    p.t4 = (p.n_frames + 3) / 4;
    p.pad_mode = pad_mode;
    p.fade_len = 0;
    p.hspec = static_cast<const ssk::f32x4*>(hspec[0]);
    p.h_blocks = (cap[0] + ssk::kB - 1) / ssk::kB;
    p.xcd_map = 0; p.stash = nullptr; p.stash_nbh = 0; p.stash_terms = 0; p.n_terms = 2; p.parts_log2 = 0;
    p.nb_y = nb_y;
    p.n_buckets = n_buckets;
    ssk::SpecScale<true, true> hs;
    hs.hscale = half ? hscale[0] : nullptr;
    for (int b = 0; b < ssk::kMaxBuckets - 1; ++b) {
        p.bk[b] = ssk::BankBucket{nullptr, nullptr, 0x7fffffff, 0, 0, 0};
        hs.bk[b] = nullptr;
    }
    for (int b = 1; b < n_buckets; ++b) {
        p.bk[b - 1] = ssk::BankBucket{rows ? rows[b] : nullptr, static_cast<const ssk::f32x4*>(hspec[b]), first[b], cap[b],
                                      (cap[b] + ssk::kB - 1) / ssk::kB, 0};
        hs.bk[b - 1] = half ? hscale[b] : nullptr;
    }
    const int grid = 2 * n_units * nb_y;
    gridDim = dim3{(unsigned)grid, 1, 1};
    const ssk::UnitTab<false> nt;
    for (int b = 0; b < grid; ++b) {
        blockIdx = dim3{(unsigned)b, 0, 0};
        int rc = run_block(ssk::kT, [&] {
            if (half) {
                if (fuse) ssk::k_conv_spec<true, false, false, false, true, true>(p, nt, hs);
                else ssk::k_conv_spec<false, false, false, false, true, true>(p, nt, hs);
            } else {
                if (fuse) ssk::k_conv_spec<true, false>(p);
                else ssk::k_conv_spec<false, false>(p);
            }
        });
        if (rc) return rc;
    }
    return 0;
}
