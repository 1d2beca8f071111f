// launch_rir16_buckets_host.cpp — TEST INFRASTRUCTURE: the launch plan (sound-spaces_amd/csrc/ss_launch.hpp) of the convolution
// over half-precision time-domain rows in length buckets - Form::kRows16 with n_buckets > 1 - without HIP.  tests/launch_host.cpp
// is included whole (its main renamed): "table" prints the grid of tests/golden/launch_table.txt.  "rows16bk" prints one line per
// (fuse, bucket 0's blocks, buckets 1..4, out_len / n_valid): the plans per flags (0, 1, 2, 3, 1 + FIRST_BUCKET) and units
// (1, 5, 257) at 256 CUs, in launch_host.cpp's format
//     <variant SLXWYP>/<unit table>/<bucket 0>/<grid x>/<grid y>/<parts_log2>/<nb_y>, E: refused.
// tests/test_rir16_buckets_host.py builds and runs it and pins the output in tests/golden/launch_rir16_buckets_table.txt.
// Never part of the product.
#define main launch_host_main
#include "launch_host.cpp"
#undef main

#include <cstring>

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "table")) return launch_host_main(1, argv);
    if (argc != 2 || std::strcmp(argv[1], "rows16bk")) return 2;
    const int shapes[3] = {1, 4, 5};                    // 16000 / 16000, 44100 / 44100, 44100 / 11025
    for (int fuse = 0; fuse < 2; ++fuse)
        for (int depth : {1, 3, 16})
            for (int n_buckets = 1; n_buckets <= 4; ++n_buckets)
                for (int s : shapes) {
                    std::printf("conv-rows16bk %d %d %d %d %d |", fuse, depth, n_buckets, kShapes[s][0], kShapes[s][1]);
                    for (int flags : kFlags)
                        for (int n_units : {1, 5, 257}) conv(1, fuse != 0, kShapes[s], flags, depth, n_buckets, n_units, 256, 1, -1, true, true);
                    end_line();
                }
    return 0;
}
