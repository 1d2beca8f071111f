// ss_consts.hpp — the shape constants the kernels (ss_fft_core.hpp, ss_kernels.hpp) and the host-side routing and launch
// geometry (ss_route.hpp, ss_launch.hpp) share.  No HIP runtime: the header also compiles in a stand-alone host program.
#pragma once

#if defined(__HIP__)
#define SSK_HOST_DEVICE __host__ __device__
#else
#define SSK_HOST_DEVICE
#endif

namespace ssk {

constexpr int kB = 16384;            // real samples of one partition block (FFT covers 2*kB)

// STFT geometry of SpectrogramSensor.compute_spectrogram (nav.py:88-93)
constexpr int kNfft = 512, kHop = 160, kPool = 4, kBins4 = 65;   // 257 bins -> 65 pooled rows
constexpr int kPrevPairs = 1208;          // XFADE: packed pairs of the cross-fade ramp kept per row (fade_len <= 2414: 48 kHz)

// what the launch geometry (ss_launch.hpp) shares with the kernels
constexpr int kT = 1024;             // threads per workgroup
constexpr int kSpecComplex = 16384;  // complex values of one stored block spectrum (kernel order)
constexpr int kSegFrames = 16;       // frames of one group of the feature kernels (k_logmel, k_gccphat, k_features)
constexpr int kMaxBuckets = 4;       // length buckets of one bank
constexpr int kTabUnits = 256;       // units of the kernel-argument table (UnitTab)
constexpr int kTailFloats = 640;     // k_obs_blocks: context handed from output block j to j+1 (nb_rows <= 3: 640, 384)
constexpr int kRowsMaxNbh = 16;      // k_obs_rows: RIR blocks per term the pair masks can hold (2 terms x 16 bits)

// pooled time blocks that can be non-zero when a row of `len` samples is zero from sample n_valid on: block b is exactly
// zero once all of its frames start behind the rendered samples (640 b - 256 >= n_valid) - provided the right centre
// padding mirrors zeros as well (n_valid <= len - 512); |STFT| of zeros is 0 and log1p(0) = 0
SSK_HOST_DEVICE constexpr int live_blocks(int n_valid, int len, int t4) {
    return n_valid <= len - kNfft ? ((n_valid + kNfft / 2 + kHop * kPool - 1) / (kHop * kPool) < t4
                                         ? (n_valid + kNfft / 2 + kHop * kPool - 1) / (kHop * kPool) : t4)
                                  : t4;
}

}  // namespace ssk
