// route_rir16_logmel_host.cpp — TEST INFRASTRUCTURE: the routing (sound-spaces_amd/csrc/ss_route.hpp) of log-mel steps on contexts
// bound to half-precision time-domain rows - ss_ctx_set_rir_bank16 (Bank::rows16), ss_ctx_set_rir_bank16_rows (+ Bank::rows16_rows),
// ss_ctx_set_rir16_buckets (Bank::rows16_buckets) - under ss_ctx_set_logmel_rir16_policy (Policies::mel_r16_min / _max), without HIP.
// tests/route_host.cpp is included whole (its main renamed): "table" prints the grid of tests/golden/route_table.txt.
// "rows16", "rows16_rows", "rows16bk": the grids of tests/route_rir16_host.cpp, route_rir16_rows_host.cpp and
// route_rir16_buckets_host.cpp line for line - the new range at its default (never), the four older ranges as those programs set
// them.  "logmel": the new range set to [1, 100], everything else at its default, one line per case:
//
//     <binding> <out_len> <n_valid> <blocks> <flags> <wants> <n> <route>
//
// binding 0 / 1 / 2 = rows16 / rows16 + rows16_rows / rows16_buckets; wants 0-4 as in route_host.cpp, 5 = log-mel asked WITH a
// waveform buffer; n = 1 (inside the range) and 200 (outside); route as in route_host.cpp.  tests/test_obs_logmel_rir16_args.py
// builds this with -fsanitize=address,undefined, runs it and pins "logmel" in tests/golden/route_rir16_logmel_table.txt.
// Never part of the product.
#define main route_host_main
#include "route_host.cpp"
#undef main

#include <cstring>

namespace {

Bank bank_of(int binding, int depth) {
    Bank b;
    b.rows16 = binding < 2;
    b.rows16_rows = binding == 1;
    b.rows16_buckets = binding == 2;
    b.rir_cap = depth * kB;
    return b;
}

void print_route(const ssroute::Route& r) {
    std::printf("%c%x\n", launch_char(r), (r.spectral ? 1 : 0) | (r.wave_scratch ? 2 : 0) | (r.handover ? 4 : 0) | (r.refused ? 8 : 0));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "table")) return route_host_main();
    if (argc != 2) return 2;
    const int depths[3] = {1, 3, 16};
    const int ns[2] = {1, 200};
    if (!std::strcmp(argv[1], "logmel")) {
        ssroute::Policies pol;
        pol.mel_r16_min = 1;
        pol.mel_r16_max = 100;
        const ssroute::Wants with_wave{true, false, true};
        for (int binding = 0; binding < 3; ++binding)
            for (const auto& shape : kShapes)
                for (int depth : depths)
                    for (int flags = 0; flags < 4; ++flags)
                        for (int w = 0; w < 6; ++w)
                            for (int n : ns) {
                                std::printf("%d %d %d %d %d %d %d ", binding, shape[0], shape[1], depth, flags, w, n);
                                print_route(ssroute::route_step(bank_of(binding, depth), shape[0], shape[1], pol, n, flags,
                                                                w < 5 ? kWants[w] : with_wave));
                            }
        return 0;
    }
    const int binding = !std::strcmp(argv[1], "rows16") ? 0 : !std::strcmp(argv[1], "rows16_rows") ? 1 : !std::strcmp(argv[1], "rows16bk") ? 2 : -1;
    if (binding < 0) return 2;
    ssroute::Policies pol[3];
    pol[1].mel_fused_min = pol[1].mel_rows_min = pol[1].mel_ss2_min = pol[1].mel_bk_min = 1;
    pol[1].mel_fused_max = pol[1].mel_rows_max = pol[1].mel_ss2_max = pol[1].mel_bk_max = 100;
    pol[2].spectral_max_units = 100;
    for (const auto& shape : kShapes)
        for (int depth : depths)
            for (int flags = 0; flags < (binding == 2 ? 8 : 4); ++flags)
                for (int w = 0; w < 5; ++w)
                    for (int n : ns)
                        for (int p = 0; p < 3; ++p) {
                            const int fl = (flags & 3) | ((flags & 4) ? SS_FLAG_FIRST_BUCKET : 0);
                            std::printf("%d %d %d %d %d %d %d ", shape[0], shape[1], depth, fl, w, n, p);
                            print_route(ssroute::route_step(bank_of(binding, depth), shape[0], shape[1], pol[p], n, fl, kWants[w]));
                        }
    return 0;
}
