// blocks_replay_host.cpp — TEST INFRASTRUCTURE: k_obs_blocks<false> / <true> with the epoch read from a word of the hand-off
// area (the form a captured graph replays: k_sync_next in front, `epoch_word` given) against the kernel-argument form, on the
// fibers of tests/hostsim/hostsim.cpp (included whole: its runner and tables are file-local).  ONE hand-off area lives across the
// calls, as the library keeps one per (device, stream), so that tests/test_blocks_replay_host.py can run replay after replay -
// and an eager launch in between - over it.  Never part of the product.
#include "hostsim/hostsim.cpp"

#include <cstring>

namespace {
std::vector<float> g_area_tails;      // [rows][2][kTailFloats]
std::vector<int> g_area_flags;        // [rows][2] flag words + the replay epoch word
}  // namespace

// the area as the library zeroes it on allocation, for `rows` (unit, ear) rows
extern "C" void hs_replay_area_reset(int rows) {
    g_area_tails.assign(sslaunch::handoff_floats(rows), 0.f);
    g_area_flags.assign(sslaunch::handoff_flags(rows) + 1, 0);
}

// the flag words of the area and the epoch word behind them -> out[handoff_flags(rows) + 1]
extern "C" int hs_replay_area_flags(int* out, int n) {
    if (n != static_cast<int>(g_area_flags.size())) return -1;
    std::memcpy(out, g_area_flags.data(), sizeof(int) * g_area_flags.size());
    return 0;
}

// mode 0: the kernel-argument form over a PRIVATE fresh area (run_obs_blocks: the reference), epoch = `epoch`
// mode 1: a replay over the shared area: k_sync_next on its epoch word, then the kernel with `epoch_word` (the kernel argument
//         is the 0 the launcher passes there)
// mode 2: an eager launch over the shared area: the kernel argument `epoch` (> 0), no epoch word
// hspec != nullptr: k_obs_blocks<true> on block spectra [R][2][h_blocks]; else k_obs_blocks<false> on planar fp32 rows [R][2][cap].
extern "C" int hs_obs_blocks_replay(int mode, int epoch, const float* spec, const float* rir, const float* hspec, const int* rir_len,
                                    const int* desc, float* out, float* sgram, int n_units, int cap, int h_blocks, int out_len) {
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB || !sgram || mode < 0 || mode > 2) return -1;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, out_len, out_len, 0);
    set_rows(p, rir, 2LL * cap, cap, 1, cap);
    set_spectra(p, hspec, h_blocks);
    p.fade_len = 0;
    const int n_rows = 2 * n_units;
    const Form form = hspec ? Form::kSpec : Form::kRows;
    if (mode == 0) return run_obs_blocks(p, form, n_units, 0, 0, nullptr, nullptr, nullptr, epoch);
    const sslaunch::ObsBlocksPlan pl = sslaunch::plan_obs_blocks(0, p.out_len, p.n_valid, n_units, n_rows * ssroute::ceil_div(out_len, ssk::kB), 1,
                                                                 true, sslaunch::Switches());
    if (!pl.ok || pl.parts_log2 != 0) return -3;
    if (g_area_tails.size() != pl.handoff_floats || g_area_flags.size() != pl.handoff_flags + 1) return -4;
    sslaunch::apply(pl, p);
    p.xcd_map = 0;
    float* tails = g_area_tails.data();
    int* fl = g_area_flags.data();
    int* word = fl + pl.handoff_flags;
    if (mode == 1) {
        const int rc = run_grid(1, 1, 64, [&] { ssk::k_sync_next(word); });
        if (rc) return rc;
    }
    const int* epoch_word = mode == 1 ? word : nullptr;
    const int arg = mode == 1 ? 0 : epoch;
    return ssdispatch::obs_blocks(HostLaunch{}, form, pl.grid, p, n_rows, tails, fl, arg, nullptr, nullptr, nullptr, epoch_word);
}

// next_replay_epoch at the ends of its range (the wrap cannot be reached by running replays)
extern "C" int hs_next_replay_epoch(int e) { return ssk::next_replay_epoch(e); }
