// route_rir16_rows_host.cpp — TEST INFRASTRUCTURE: the routing (sound-spaces_amd/csrc/ss_route.hpp) of a context bound by
// ss_ctx_set_rir_bank16_rows - half-precision time-domain rows opted in to the fused row kernels, Bank::rows16 + Bank::rows16_rows -
// without HIP.  tests/route_host.cpp is included whole (its main renamed): that program never touches the two fields, so "table"
// prints the grid of tests/golden/route_table.txt with both clear.  "rows16" prints the grid of tests/route_rir16_host.cpp (rows16
// alone: the plain binding), "rows16_rows" the same grid with both fields set, one line per case:
//
//     <out_len> <n_valid> <blocks> <flags> <wants> <n> <policy> <route>
//
// wants and route as in route_host.cpp; policy 0 = the defaults, 1 = every log-mel range [1, 100], 2 = spectral_max_units = 100.
// tests/test_rir16_rows_host.py builds and runs it.  Never part of the product.
#define main route_host_main
#include "route_host.cpp"
#undef main

#include <cstring>

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "table")) return route_host_main();
    if (argc != 2 || (std::strcmp(argv[1], "rows16") && std::strcmp(argv[1], "rows16_rows"))) return 2;
    const bool fused_rows = !std::strcmp(argv[1], "rows16_rows");
    ssroute::Policies pol[3];
    pol[1].mel_fused_min = pol[1].mel_rows_min = pol[1].mel_ss2_min = pol[1].mel_bk_min = 1;
    pol[1].mel_fused_max = pol[1].mel_rows_max = pol[1].mel_ss2_max = pol[1].mel_bk_max = 100;
    pol[2].spectral_max_units = 100;
    const int depths[3] = {1, 3, 16};
    const int ns[2] = {1, 200};
    for (const auto& shape : kShapes)
        for (int depth : depths)
            for (int flags = 0; flags < 4; ++flags)
                for (int w = 0; w < 5; ++w)
                    for (int n : ns)
                        for (int p = 0; p < 3; ++p) {
                            Bank b;
                            b.rows16 = true;
                            b.rows16_rows = fused_rows;
                            b.rir_cap = depth * kB;
                            const ssroute::Route r = ssroute::route_step(b, shape[0], shape[1], pol[p], n, flags, kWants[w]);
                            std::printf("%d %d %d %d %d %d %d %c%x\n", shape[0], shape[1], depth, flags, w, n, p, launch_char(r),
                                        (r.spectral ? 1 : 0) | (r.wave_scratch ? 2 : 0) | (r.handover ? 4 : 0) | (r.refused ? 8 : 0));
                        }
    return 0;
}
