// ss_consts.hpp — the shape constants the kernels (ss_fft_core.hpp, ss_kernels.hpp) and the host-side routing (ss_route.hpp)
// share.  No HIP runtime: the header also compiles in a stand-alone host program.
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

// pooled time blocks that can be non-zero when a row of `len` samples is zero from sample n_valid on: block b is exactly
// zero once all of its frames start behind the rendered samples (640 b - 256 >= n_valid) - provided the right centre
// padding mirrors zeros as well (n_valid <= len - 512); |STFT| of zeros is 0 and log1p(0) = 0
SSK_HOST_DEVICE constexpr int live_blocks(int n_valid, int len, int t4) {
    return n_valid <= len - kNfft ? ((n_valid + kNfft / 2 + kHop * kPool - 1) / (kHop * kPool) < t4
                                         ? (n_valid + kNfft / 2 + kHop * kPool - 1) / (kHop * kPool) : t4)
                                  : t4;
}

}  // namespace ssk
