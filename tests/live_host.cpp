// live_host.cpp — TEST INFRASTRUCTURE: the zero-column shortcut of the observation kernels (ssk::live_blocks, csrc/ss_consts.hpp)
// on its own, without HIP and without a kernel.  For every row length given on the command line prints one line
//
//     <len> <t4> <live_blocks(0, len, t4)> <live_blocks(1, len, t4)> ... <live_blocks(len, len, t4)>
//
// (t4: the pooled columns of a row of `len` samples).  tests/test_live_blocks_host.py builds this with
// -fsanitize=address,undefined, runs it and compares every value with the truth it derives from the STFT geometry.
// Never part of the product.
#include <cstdio>
#include <cstdlib>

#include "../sound-spaces_amd/csrc/ss_consts.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const int len = std::atoi(argv[a]);
        if (len < 1) return 2;
        const int n_frames = 1 + len / ssk::kHop, t4 = (n_frames + ssk::kPool - 1) / ssk::kPool;
        std::printf("%d %d", len, t4);
        for (int n_valid = 0; n_valid <= len; ++n_valid) std::printf(" %d", ssk::live_blocks(n_valid, len, t4));
        std::printf("\n");
    }
    return 0;
}
