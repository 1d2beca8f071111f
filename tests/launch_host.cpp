// launch_host.cpp — TEST INFRASTRUCTURE: the launch geometry (sound-spaces_amd/csrc/ss_launch.hpp) on its own, without HIP.
// Prints the plan of every launcher over a fixed grid, one line per group of cases: "<kind> <fixed inputs> | <plan> <plan> ...",
// the plans in the order of the loops named below (innermost last); a run of n equal plans is written once as "<plan>*n".
// A plan's fields are joined by '/':
//
//     conv-shape <form> <fuse> <out_len> <n_valid>          | per flags (0, 1, 2, 3, 1 + FIRST_BUCKET): 5 units, 256 CUs, one RIR block
//     conv-units <form> <fuse> <CUs> <share> <forced parts>  | per units, flags (0, 1), planar = aligned (0, 1): 16 000-sample rows
//     conv-depth <form> <fuse> <RIR blocks>                  | per buckets (1, 2), flags (the five above): 5 units, 256 CUs
//          plan: <variant SLXWYP>/<unit table>/<bucket 0>/<grid x>/<grid y>/<parts_log2>/<nb_y>, E: refused (nothing else is read)
//     blocks <out_len> <n_valid> <CUs> <share>               | per flags (0..3), units
//          plan: <parts_log2>/<nb>/<grid>/<n_terms>/<hand-off floats>/<flag words>, -: the launch does not qualify
//     rows <spectral> <out_len> <n_valid> <flags> <CUs>      | per units, (share, forced parts) = (1, -1), (2, -1), (1, 2): 3 RIR blocks
//     rows-depth <spectral> <RIR blocks>                     | per buckets (1, 2), flags (0..3): 44 100-sample rows, 5 units, 256 CUs
//          plan: <parts_log2>/<grid>/<nb_y>/<n_terms>/<stash_nbh>/<stash_terms>/<stash_bytes>, E: refused
//     frames <kind> <len> <n_valid>                          | per units, wanted gpw (units x groups / 2048, / 1024, 1, 3)
//          plan: <n_frames>/<t4>/<live>/<groups>/<gpw>/<chunks>/<grid>
//     features <len>                                         | per units, max workgroups (512, 16, 1): the grid
//     params <out_len> <n_valid>                             | the shape fields and defaults init_conv_params sets
// and, with the argument `mel`, the one-block log-mel plan alone (plan_conv_mel; tests/golden/launch_mel_table.txt):
//     mel <form> <ss2 shape 0 1 2> <RIR blocks 1, 1 + a sample / 2> | per buckets (1, 2), flags (0, NO_DISTRACTOR, NO_DISTRACTOR +
//          FIRST_BUCKET, CROSSFADE), fade_len (0, 1, 2 kPrevPairs - 2, one beyond), units (1, 5, 257)
//          plan: <variant SLXWY>/<bucket 0>/<grid>, E: refused; grid y, parts and nb_y are fixed (1, 0, 1: anything else prints ?)
//
// units: 1 2 5 16 32 33 64 128 129 256 257.  The values of every input are the smallest at which a rule flips; each launcher is
// walked over the inputs it reads.  tests/test_launch_host.py builds this with -fsanitize=address,undefined, runs it and compares
// the output with tests/golden/launch_table.txt.  Never part of the product.
#include <cstdio>
#include <initializer_list>
#include <string>

#include "../sound-spaces_amd/csrc/ss_launch.hpp"

namespace {

using ssk::kB;
using namespace sslaunch;

const int kShapes[13][2] = {{257, 257},     {16000, 16000}, {16384, 16384}, {16385, 16385}, {44100, 44100},   {44100, 11025}, {48000, 48000},
                            {48000, 12000}, {49153, 49153}, {44100, kB},    {44100, kB + 1}, {48000, kB}, {48000, kB + 1}};
const int kUnits[11] = {1, 2, 5, 16, 32, 33, 64, 128, 129, 256, 257};
const int kCus[2] = {256, 8};
const int kFlags[5] = {0, 1, 2, 3, SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET};
const int kDepths[4] = {1, 3, 16, 17};
const Form kForms[5] = {Form::kRows, Form::kRows16, Form::kSpec, Form::kSpec16, Form::kSpec16Buckets};
const char* const kFormNames[5] = {"rows", "rows16", "spec", "spec16", "spec16bk"};

// one output line: the key, then the plans with runs of equal ones collapsed
std::string g_last;
int g_run = 0;
void flush_run() {
    if (g_run == 1) std::printf(" %s", g_last.c_str());
    else if (g_run > 1) std::printf(" %s*%d", g_last.c_str(), g_run);
    g_run = 0;
}
void add(const char* plan) {
    if (g_run && g_last == plan) { ++g_run; return; }
    flush_run();
    g_last = plan;
    g_run = 1;
}
void end_line() { flush_run(); std::printf("\n"); }

void conv(int f, bool fuse, const int (&shape)[2], int flags, int depth, int n_buckets, int n_units, int n_cus, int share, int forced,
          bool planar, bool aligned) {
    const bool time = kForms[f] == Form::kRows || kForms[f] == Form::kRows16;
    const bool wide = fuse && ssroute::wide_one_block_ok(shape[0], shape[1], flags, !time, ssroute::Switches());
    const ConvPlan pl = plan_conv(kForms[f], fuse, wide, flags, time ? depth * kB : 0, time ? 0 : depth, n_buckets,
                                  static_cast<int>(0.05 * shape[0]), planar, aligned, n_units, wide ? 1 : nb_y_of(shape[1]), n_cus, share,
                                  Switches{forced, false, false});
    char buf[96];
    if (pl.rc) std::snprintf(buf, sizeof buf, "E");
    else std::snprintf(buf, sizeof buf, "%c/%d/%d/%d/%d/%d/%d", "SLXWYP"[static_cast<int>(pl.variant)], pl.tab_ok, pl.bucket0, pl.grid_x,
                       pl.grid_y, pl.parts_log2, pl.nb_y);
    add(buf);
}

void rows(bool spectral, const int (&shape)[2], int flags, int depth, int n_buckets, int n_units, int n_cus, int share, int forced) {
    const ObsRowsPlan pl = plan_obs_rows(spectral, false, false, flags, shape[1], n_buckets, depth, n_units, n_cus, share,
                                         Switches{forced, false, false});
    char buf[96];
    if (pl.rc) std::snprintf(buf, sizeof buf, "E");
    else std::snprintf(buf, sizeof buf, "%d/%d/%d/%d/%d/%d/%zu", pl.parts_log2, pl.grid, pl.nb_y, pl.n_terms, pl.stash_nbh, pl.stash_terms,
                       pl.stash_bytes);
    add(buf);
}

}  // namespace

// ---- plan_conv_mel: `launch_host mel` prints this table alone (tests/golden/launch_mel_table.txt)
int mel_table() {
    const int kMelFlags[4] = {0, SS_FLAG_NO_DISTRACTOR, SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET, SS_FLAG_CROSSFADE};
    const int kFades[4] = {0, 1, 2 * ssk::kPrevPairs - 2, 2 * ssk::kPrevPairs - 1};
    char buf[64];
    for (int f = 0; f < 5; ++f)
        for (int ss2 = 0; ss2 < 3; ++ss2)
            for (int depth = 1; depth <= 2; ++depth) {
                const bool time = kForms[f] == Form::kRows || kForms[f] == Form::kRows16;
                std::printf("mel %s %d %d |", kFormNames[f], ss2, depth);
                for (int n_buckets = 1; n_buckets <= 2; ++n_buckets)
                    for (int flags : kMelFlags)
                        for (int fade : kFades)
                            for (int n_units : {1, 5, 257}) {
                                const ConvPlan pl = plan_conv_mel(kForms[f], ss2, flags, time ? (depth == 1 ? kB : kB + 1) : 0, time ? 0 : depth,
                                                                  n_buckets, fade, n_units);
                                if (pl.rc) std::snprintf(buf, sizeof buf, "E");
                                else if (pl.grid_y != 1 || pl.parts_log2 != 0 || pl.nb_y != 1 || pl.tab_ok) std::snprintf(buf, sizeof buf, "?");
                                else std::snprintf(buf, sizeof buf, "%c/%d/%d", "SLXWYP"[static_cast<int>(pl.variant)], pl.bucket0, pl.grid_x);
                                add(buf);
                            }
                end_line();
            }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "mel") return mel_table();
    char buf[128];
    // ---- plan_conv
    for (int f = 0; f < 5; ++f)
        for (int fuse = 0; fuse < 2; ++fuse) {
            for (const auto& shape : kShapes) {
                std::printf("conv-shape %s %d %d %d |", kFormNames[f], fuse, shape[0], shape[1]);
                for (int flags : kFlags) conv(f, fuse, shape, flags, 1, 1, 5, 256, 1, -1, true, true);
                end_line();
            }
            for (int n_cus : kCus)
                for (int share = 1; share <= 2; ++share)
                    for (int forced : {-1, 2}) {
                        std::printf("conv-units %s %d %d %d %d |", kFormNames[f], fuse, n_cus, share, forced);
                        for (int n_units : kUnits)
                            for (int flags : {0, 1})
                                for (int al = 0; al < 2; ++al) conv(f, fuse, kShapes[1], flags, 1, 1, n_units, n_cus, share, forced, al, al);
                        end_line();
                    }
            for (int depth : kDepths) {
                std::printf("conv-depth %s %d %d |", kFormNames[f], fuse, depth);
                for (int n_buckets = 1; n_buckets <= 2; ++n_buckets)
                    for (int flags : kFlags) conv(f, fuse, kShapes[1], flags, depth, n_buckets, 5, 256, 1, -1, true, true);
                end_line();
            }
        }
    // ---- plan_obs_blocks
    for (const auto& shape : kShapes)
        for (int n_cus : kCus)
            for (int share = 1; share <= 2; ++share) {
                std::printf("blocks %d %d %d %d |", shape[0], shape[1], n_cus, share);
                for (int flags = 0; flags < 4; ++flags)
                    for (int n_units : kUnits) {
                        const ObsBlocksPlan pl = plan_obs_blocks(flags, shape[0], shape[1], n_units, n_cus, share, true, Switches());
                        if (!pl.ok) std::snprintf(buf, sizeof buf, "-");
                        else std::snprintf(buf, sizeof buf, "%d/%d/%d/%d/%zu/%zu", pl.parts_log2, pl.nb, pl.grid, pl.n_terms, pl.handoff_floats,
                                           pl.handoff_flags);
                        add(buf);
                    }
                end_line();
            }
    {   // (what keeps a launch out whatever its shape: the per-thread stream, the A/B switch, more rows than the hand-off area holds)
        const ObsBlocksPlan a = plan_obs_blocks(1, 44100, 44100, 5, 256, 1, false, Switches());
        const ObsBlocksPlan b = plan_obs_blocks(1, 44100, 44100, 5, 256, 1, true, Switches{-1, false, true});
        const ObsBlocksPlan c = plan_obs_blocks(1, 44100, 44100, kSyncRows / 2 + 1, 1 << 20, 1, true, Switches());
        std::printf("blocks-off %d %d %d\n", a.ok, b.ok, c.ok);
    }
    // ---- plan_obs_rows: the shapes of rows of 2 or 3 blocks
    for (int spectral = 0; spectral < 2; ++spectral) {
        for (int s = 4; s < 13; ++s)
            for (int flags = 0; flags < 4; ++flags)
                for (int n_cus : kCus) {
                    std::printf("rows %d %d %d %d %d |", spectral, kShapes[s][0], kShapes[s][1], flags, n_cus);
                    for (int n_units : kUnits) {
                        rows(spectral, kShapes[s], flags, 3, 1, n_units, n_cus, 1, -1);
                        rows(spectral, kShapes[s], flags, 3, 1, n_units, n_cus, 2, -1);
                        rows(spectral, kShapes[s], flags, 3, 1, n_units, n_cus, 1, 2);
                    }
                    end_line();
                }
        for (int depth : kDepths) {
            std::printf("rows-depth %d %d |", spectral, depth);
            for (int n_buckets = 1; n_buckets <= 2; ++n_buckets)
                for (int flags = 0; flags < 4; ++flags) rows(spectral, kShapes[4], flags, depth, n_buckets, 5, 256, 1, -1);
            end_line();
        }
    }
    {   // (the forms that take plain rows only / one allocation only)
        const ObsRowsPlan a = plan_obs_rows(true, true, false, SS_FLAG_CROSSFADE, 44100, 1, 3, 5, 256, 1, Switches());
        const ObsRowsPlan b = plan_obs_rows(true, true, true, 0, 44100, 2, 3, 5, 256, 1, Switches());
        const ObsRowsPlan c = plan_obs_rows(true, true, true, 0, 44100, 1, 3, 5, 256, 1, Switches());
        std::printf("rows-refused %d %d %d\n", a.rc != 0, b.rc != 0, c.rc != 0);
    }
    // ---- plan_frames / features_grid: the library's rules (units x groups / 2048, / 1024) and two of the tests' own
    for (int kind = 0; kind < 2; ++kind)
        for (const auto& shape : kShapes) {
            std::printf("frames %d %d %d |", kind, shape[0], shape[1]);
            for (int n_units : kUnits) {
                const Frames k = kind ? Frames::kSegments : Frames::kPooled;
                const long long g = groups_of(k, shape[0]);
                for (long long wanted : {n_units * g / 2048, n_units * g / 1024, 1LL, 3LL}) {
                    const FramesPlan pl = plan_frames(k, n_units, shape[0], shape[1], wanted);
                    std::snprintf(buf, sizeof buf, "%d/%d/%d/%d/%d/%d/%d", pl.n_frames, pl.t4, pl.live, pl.groups, pl.gpw, pl.chunks, pl.grid);
                    add(buf);
                }
            }
            end_line();
        }
    for (const auto& shape : kShapes) {
        std::printf("features %d |", shape[0]);
        for (int n_units : kUnits)
            for (long long max_wgs : {512LL, 16LL, 1LL}) {
                std::snprintf(buf, sizeof buf, "%d", features_grid(n_units, shape[0], max_wgs));
                add(buf);
            }
        end_line();
    }
    // ---- init_conv_params / apply on a struct of this file's own (the header needs no ss_kernels.hpp)
    struct Bucket { const float* rir; const void* hspec; int first, cap, h_blocks, pad_; };
    struct Params {
        int n_valid, out_len, n_frames, t4, pad_mode, fade_len, h_blocks, xcd_map, nb_y, parts_log2, stash_nbh, stash_terms, n_terms, n_buckets, rir_cap;
        const void* hspec;
        void* stash;
        Bucket bk[ssk::kMaxBuckets - 1];
    };
    for (const auto& shape : kShapes) {
        Params p;
        init_conv_params(p, shape[1], shape[0]);
        p.rir_cap = 3 * kB;
        std::printf("params %d %d | %d %d %d %d %d %d %d %d %d %d %d %d %d\n", shape[0], shape[1], p.n_frames, p.t4, p.pad_mode, p.fade_len, p.h_blocks,
                    p.nb_y, p.parts_log2, p.stash_nbh, p.stash_terms, p.n_terms, p.n_buckets, p.bk[0].first, rows_nbh_max(p));
    }
    return 0;
}
