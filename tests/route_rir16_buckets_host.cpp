// route_rir16_buckets_host.cpp — TEST INFRASTRUCTURE: the routing (sound-spaces_amd/csrc/ss_route.hpp) of a context bound by
// ss_ctx_set_rir16_buckets - half-precision time-domain rows in length buckets, Bank::rows16_buckets - without HIP.
// tests/route_host.cpp is included whole (its main renamed): that program never touches the field, so "table" prints the grid of
// tests/golden/route_table.txt with the field clear.  "rows16bk" prints, with the field set, one line per case:
//
//     <out_len> <n_valid> <blocks> <flags> <wants> <n> <policy> <route>
//
// over the grid of tests/route_rir16_host.cpp (blocks = the deepest bucket's; the planner's SS_FLAG_FIRST_BUCKET on top of every
// flag value, which the route does not read); wants and route as in route_host.cpp; policy 0 = the defaults, 1 = every log-mel
// range [1, 100], 2 = spectral_max_units = 100.  tests/test_rir16_buckets_host.py builds and runs it and pins the output in
// tests/golden/route_rir16_buckets_table.txt.  Never part of the product.
#define main route_host_main
#include "route_host.cpp"
#undef main

#include <cstring>

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "table")) return route_host_main();
    if (argc != 2 || std::strcmp(argv[1], "rows16bk")) return 2;
    ssroute::Policies pol[3];
    pol[1].mel_fused_min = pol[1].mel_rows_min = pol[1].mel_ss2_min = pol[1].mel_bk_min = 1;
    pol[1].mel_fused_max = pol[1].mel_rows_max = pol[1].mel_ss2_max = pol[1].mel_bk_max = 100;
    pol[2].spectral_max_units = 100;
    const int depths[3] = {1, 3, 16};
    const int ns[2] = {1, 200};
    for (const auto& shape : kShapes)
        for (int depth : depths)
            for (int flags = 0; flags < 8; ++flags)
                for (int w = 0; w < 5; ++w)
                    for (int n : ns)
                        for (int p = 0; p < 3; ++p) {
                            Bank b;
                            b.rows16_buckets = true;
                            b.rir_cap = depth * kB;
                            const int fl = (flags & 3) | ((flags & 4) ? SS_FLAG_FIRST_BUCKET : 0);
                            const ssroute::Route r = ssroute::route_step(b, shape[0], shape[1], pol[p], n, fl, kWants[w]);
                            std::printf("%d %d %d %d %d %d %d %c%x\n", shape[0], shape[1], depth, fl, w, n, p, launch_char(r),
                                        (r.spectral ? 1 : 0) | (r.wave_scratch ? 2 : 0) | (r.handover ? 4 : 0) | (r.refused ? 8 : 0));
                        }
    return 0;
}
