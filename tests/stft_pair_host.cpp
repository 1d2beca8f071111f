// stft_pair_host.cpp — TEST INFRASTRUCTURE: the host build of the kernels (tests/hostsim/hostsim.cpp, included whole) as a
// library of its own, so tests/test_stft_pair_host.py can compile it twice - as the product does, and with -DSS_NO_STFT_PAIR -
// and hold the fused observation kernels whose waves run their two pooled blocks as a pair (stft_block_pair, ss_kernels.hpp)
// to the same kernels running them one after the other.  Never part of the product.
#include "hostsim/hostsim.cpp"

// 1: this build's fused STFT phase hands a wave's two blocks to stft_block_pair; 0: the -DSS_NO_STFT_PAIR arm
extern "C" int hs_stft_pair_enabled() {
#if defined(SS_NO_STFT_PAIR)
    return 0;
#else
    return 1;
#endif
}

// ssk::live_blocks itself: the test picks n_valid by it
extern "C" int hs_live_blocks(int n_valid, int out_len, int t4) { return ssk::live_blocks(n_valid, out_len, t4); }
