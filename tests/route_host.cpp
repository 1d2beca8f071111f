// route_host.cpp — TEST INFRASTRUCTURE: the routing of a context's step (sound-spaces_amd/csrc/ss_route.hpp) on its own, without
// HIP.  Prints the Route of every case of a fixed grid, one line per (bank form, out_len, n_valid, RIR blocks, planner flags):
//
//     <bank> <out_len> <n_valid> <blocks> <flags> | <wants 0> | ... | <wants 4>
//
// wants: waveform only, spectrogram only, both, log-mel only, log-mel + spectrogram.  Per wants six routes, n = 1 then n = 200,
// each under the default policies, every log-mel range set to [1, 100], and spectral_max_units = 100 - printed once where all
// six are the same.  A route is two characters:
// the launch (- none, C convolution, F fused one-block, W wide, R rows, T two launches, m / s / r log-mel one-block / SS2.0 /
// rows) and a hex digit of 1 spectral + 2 waveform scratch + 4 hand-over buffer + 8 refused.
// Behind the fixed grid, the same line for rows of three blocks with n_valid ON and right behind the block seam (44100 / 48000
// samples, n_valid = kB and kB + 1: the wide kernel's last step, the first one of the row kernels), every form, depth and flag.
// tests/test_route_host.py builds this with -fsanitize=address,undefined, runs it and compares the output with
// tests/golden/route_table.txt.  Never part of the product.
#include <cstdio>

#include "../sound-spaces_amd/csrc/ss_route.hpp"

namespace {

using ssroute::Bank;
using ssroute::kB;

struct Form { const char* name; bool rows, spectra, half, buckets, buckets_spectra, spec_buckets, spec_buckets_half; };
const Form kForms[10] = {
    {"rows", true, false, false, false, false, false, false},
    {"rows+spec", true, true, false, false, false, false, false},
    {"spec", false, true, false, false, false, false, false},
    {"rows+half", true, true, true, false, false, false, false},
    {"half", false, true, true, false, false, false, false},
    {"half-rows", false, true, true, false, false, false, false},      // (bound by ss_ctx_set_rir_spectra16_rows: the same to a step)
    {"buckets", true, false, false, true, false, false, false},
    {"buckets+spec", true, false, false, true, true, false, false},
    {"specbk", false, false, false, false, false, true, false},
    {"specbk-half", false, false, false, false, false, true, true},
};
const int kShapes[9][2] = {{257, 257},     {16000, 16000}, {16384, 16384}, {16385, 16385}, {44100, 44100},
                           {44100, 11025}, {48000, 48000}, {48000, 12000}, {49153, 49153}};
const int kSeamShapes[4][2] = {{44100, kB}, {44100, kB + 1}, {48000, kB}, {48000, kB + 1}};
const int kDepths[3] = {1, 3, 17};
const ssroute::Wants kWants[5] = {{true, false, false}, {false, true, false}, {true, true, false}, {false, false, true}, {false, true, true}};

char launch_char(const ssroute::Route& r) {
    switch (r.launch) {
        case ssroute::Launch::kNone: return '-';
        case ssroute::Launch::kConv: return 'C';
        case ssroute::Launch::kObs: return "FWRT"[static_cast<int>(r.chain)];
        case ssroute::Launch::kMelOneBlock: return 'm';
        case ssroute::Launch::kMelSs2: return 's';
        case ssroute::Launch::kMelRows: return 'r';
    }
    return '?';
}

}  // namespace

int main() {
    ssroute::Policies pol[3];
    pol[1].mel_fused_min = pol[1].mel_rows_min = pol[1].mel_ss2_min = pol[1].mel_bk_min = 1;
    pol[1].mel_fused_max = pol[1].mel_rows_max = pol[1].mel_ss2_max = pol[1].mel_bk_max = 100;
    pol[2].spectral_max_units = 100;
    const int ns[2] = {1, 200};
    auto line = [&](const Form& f, const int (&shape)[2], int depth, int flags) {
        Bank b;
        b.rows = f.rows; b.spectra = f.spectra; b.half = f.half; b.buckets = f.buckets;
        b.buckets_spectra = f.buckets_spectra; b.spec_buckets = f.spec_buckets; b.spec_buckets_half = f.spec_buckets_half;
        b.rir_cap = depth * kB;
        b.h_blocks = f.spectra ? depth : 0;
        std::printf("%s %d %d %d %d", f.name, shape[0], shape[1], depth, flags);
        for (const ssroute::Wants& w : kWants) {
            char code[6][3];
            int k = 0;
            bool same = true;
            for (int n : ns)
                for (const ssroute::Policies& p : pol) {
                    const ssroute::Route r = ssroute::route_step(b, shape[0], shape[1], p, n, flags, w);
                    std::snprintf(code[k], 3, "%c%x", launch_char(r),
                                  (r.spectral ? 1 : 0) | (r.wave_scratch ? 2 : 0) | (r.handover ? 4 : 0) | (r.refused ? 8 : 0));
                    same = same && code[k][0] == code[0][0] && code[k][1] == code[0][1];
                    ++k;
                }
            std::printf(" |");
            for (int i = 0; i < (same ? 1 : 6); ++i) std::printf(" %s", code[i]);
        }
        std::printf("\n");
    };
    for (const Form& f : kForms)
        for (const auto& shape : kShapes)
            for (int depth : kDepths)
                for (int flags = 0; flags < 4; ++flags) line(f, shape, depth, flags);      // SS_FLAG_NO_DISTRACTOR = 1, SS_FLAG_CROSSFADE = 2
    for (const Form& f : kForms)                            // appended: n_valid on the block seam of a three-block row
        for (const auto& shape : kSeamShapes)
            for (int depth : kDepths)
                for (int flags = 0; flags < 4; ++flags) line(f, shape, depth, flags);
    return 0;
}
