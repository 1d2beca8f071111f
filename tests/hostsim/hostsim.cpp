// hostsim.cpp — TEST INFRASTRUCTURE: runs the HIP kernels of sound-spaces_amd/csrc on the host, one workgroup
// at a time, each thread a ucontext fiber, so tests/test_hostsim.py can compare them with the oracle on CPU.
#include <ucontext.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "hip_shim.h"
#include "../../sound-spaces_amd/csrc/ss_kernels.hpp"
#include "../../sound-spaces_amd/csrc/ss_kernels32.hpp"
#include "../../sound-spaces_amd/csrc/ss_features.hpp"
#include "../../sound-spaces_amd/csrc/ss_tables.hpp"
#include "../../sound-spaces_amd/csrc/ss_launch.hpp"
#include "../../sound-spaces_amd/csrc/ss_dispatch.hpp"

dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace {
constexpr size_t kStack = 128 * 1024;
ucontext_t g_main;
std::vector<ucontext_t> g_ctx;
std::vector<char> g_stacks;
std::vector<char> g_done;
int g_cur = 0, g_nthreads = 0;
long g_progress = 0;
std::function<void()> g_body;

struct Barrier { int count = 0; long generation = 0; };
Barrier g_block_barrier;
std::vector<Barrier> g_wave_barrier;

void yield_fiber() {
    const int me = g_cur;
    swapcontext(&g_ctx[me], &g_main);
    threadIdx.x = me;
}

void barrier_wait(Barrier& b, int expected) {
    const long gen = b.generation;
    if (++b.count == expected) { b.count = 0; ++b.generation; ++g_progress; return; }
    while (b.generation == gen) yield_fiber();
}

void fiber_entry() {
    g_body();
    g_done[g_cur] = 1;
    ++g_progress;
    swapcontext(&g_ctx[g_cur], &g_main);
}

// run one workgroup: fibers are resumed round-robin; barriers are generation counters
int run_block(int nthreads, const std::function<void()>& body) {
    g_body = body;
    g_nthreads = nthreads;
    g_ctx.assign(nthreads, ucontext_t{});
    if (g_stacks.size() < kStack * nthreads) g_stacks.resize(kStack * nthreads);
    g_done.assign(nthreads, 0);
    g_block_barrier = Barrier{};
    g_wave_barrier.assign((nthreads + 63) / 64, Barrier{});
    for (int i = 0; i < nthreads; ++i) {
        getcontext(&g_ctx[i]);
        g_ctx[i].uc_stack.ss_sp = g_stacks.data() + kStack * i;
        g_ctx[i].uc_stack.ss_size = kStack;
        g_ctx[i].uc_link = &g_main;
        makecontext(&g_ctx[i], fiber_entry, 0);
    }
    blockDim.x = nthreads;
    for (;;) {
        int live = 0;
        const long before = g_progress;
        for (int i = 0; i < nthreads; ++i) {
            if (g_done[i]) continue;
            g_cur = i;
            threadIdx.x = i;
            swapcontext(&g_main, &g_ctx[i]);
            live += !g_done[i];
        }
        if (!live) break;
        if (g_progress == before) {
            std::fprintf(stderr, "hostsim: deadlock (divergent barriers) with %d live threads\n", live);
            return -2;
        }
    }
    return 0;
}

ssk::Tables host_tables() {
    static std::vector<float> tab = ssk_host::build_tables();
    ssk::Tables tb;
    tb.twM = reinterpret_cast<const ssk::c32*>(tab.data() + ssk_host::kTwMOff);
    tb.twItem = reinterpret_cast<const ssk::c32*>(tab.data() + ssk_host::kTwItemOff);
    tb.tw512 = reinterpret_cast<const ssk::c32*>(tab.data() + ssk_host::kTw512Off);
    tb.win = tab.data() + ssk_host::kWinOff;
    tb.twG = reinterpret_cast<const ssk::c32*>(tab.data() + ssk_host::kTwGOff);
    tb.twP2 = reinterpret_cast<const ssk::c32*>(tab.data() + ssk_host::kTwP2Off);
    return tb;
}

// one launch: the workgroups of a grid one after the other, blockIdx.x fastest (reversed: the last workgroup first)
int run_grid(int grid_x, int grid_y, int nthreads, const std::function<void()>& body, bool reversed = false) {
    gridDim = dim3{(unsigned)grid_x, (unsigned)grid_y, 1};
    const int n = grid_x * grid_y;
    for (int i = 0; i < n; ++i) {
        const int b = reversed ? n - 1 - i : i;
        blockIdx = dim3{(unsigned)(b % grid_x), (unsigned)(b / grid_x), 0};
        const int rc = run_block(nthreads, body);
        if (rc) return rc;
    }
    return 0;
}

// The launch geometry is the library's (sound-spaces_amd/csrc/ss_launch.hpp).  What a test chooses freely arrives as a plan
// INPUT: the parts of a row as the forced parts_log2 (the library's A/B switch), persistent workgroups as the chip's CUs.
constexpr int kBigChip = 1 << 20;                     // more CUs than any launch here has rows: never the persistent kernels
sslaunch::Switches forced_parts(int parts_log2) { return sslaunch::Switches{parts_log2, false, false}; }

// ConvParams as the library's fill_conv leaves them (xcd_map off, the host's tables), without a bank
ssk::ConvParams conv_params(const float* spec, const int* rir_len, const int* desc, float* out, float* sgram, int n_valid,
                            int out_len, int pad_mode) {
    ssk::ConvParams p;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec); p.rir = nullptr; p.rir_len = rir_len; p.desc = desc;
    p.out = out; p.sgram = sgram; p.tb = host_tables();
    p.rir_unit_stride = 0; p.rir_chan_stride = 0; p.rir_elem_stride = 1; p.rir_cap = 0;
    sslaunch::init_conv_params(p, n_valid, out_len);
    p.pad_mode = pad_mode;
    return p;
}
void set_rows(ssk::ConvParams& p, const float* rir, long long us, int cs, int es, int cap) {
    p.rir = rir; p.rir_unit_stride = us; p.rir_chan_stride = cs; p.rir_elem_stride = es; p.rir_cap = cap;
}
void set_spectra(ssk::ConvParams& p, const void* hspec, int h_blocks) {
    p.hspec = static_cast<const ssk::f32x4*>(hspec); p.h_blocks = h_blocks;
}
// buckets 1.. of a length-bucketed bank (bucket 0: set_rows / set_spectra); rows / hspec: per bucket, or nullptr
void set_buckets(ssk::ConvParams& p, const float* const* rows, const void* const* hspec, const int* first, const int* cap, int n_buckets) {
    p.n_buckets = n_buckets;
    for (int b = 1; b < n_buckets; ++b)
        p.bk[b - 1] = ssk::BankBucket{rows ? rows[b] : nullptr, hspec ? static_cast<const ssk::f32x4*>(hspec[b]) : nullptr, first[b], cap[b],
                                      ssroute::ceil_div(cap[b], ssk::kB), 0};
}
// the scales of a half bank in buckets (hscale == nullptr: none)
ssk::SpecScale<true, true> bucket_scales(const float* const* hscale, int n_buckets) {
    ssk::SpecScale<true, true> hs;
    hs.hscale = hscale ? hscale[0] : nullptr;
    for (int b = 0; b < ssk::kMaxBuckets - 1; ++b) hs.bk[b] = hscale && b + 1 < n_buckets ? hscale[b + 1] : nullptr;
    return hs;
}
// the unit table with launch slot k rendering unit n - 1 - k (the library deals the units out sorted by window spectrum:
// word 2 = where the results go)
void fill_tab_reversed(ssk::UnitTab<true>& ut, const int* desc, int n_units) {
    for (int k = 0; k < n_units; ++k) {
        const int i = n_units - 1 - k;
        const int* d = desc + 8 * i;
        const bool ok = d[0] >= 0 && d[2] <= 0 && d[2] + d[3] > 0;
        ut.tab[ssk::kTabWords * k] = ok ? d[0] : -1;
        ut.tab[ssk::kTabWords * k + 1] = ok ? d[1] - d[2] : 0;
        ut.tab[ssk::kTabWords * k + 2] = i;
    }
}

// The kernel choice is the library's too (sound-spaces_amd/csrc/ss_dispatch.hpp).  Its launcher here: the grid on the fibers, one
// workgroup after the other (reversed: the last first) - under the shim __global__ is empty, a kernel is an ordinary function.
struct HostLaunch {
    bool reversed = false;
    template <class... A, class... B>
    int operator()(void (*kernel)(A...), dim3 grid, const B&... args) const {
        return run_grid(static_cast<int>(grid.x), static_cast<int>(grid.y), ssk::kT, [&] { kernel(args...); }, reversed);
    }
};
using sslaunch::Form;
// ssdispatch::conv with FUSE as a value; ut != nullptr: the unit table, where the plan allows one
int dispatch_conv(bool fuse, Form form, const sslaunch::ConvPlan& pl, const ssk::ConvParams& p, int n_units,
                  const ssk::UnitTab<true>* ut = nullptr, const ssk::SpecScale<true, true>* hs = nullptr,
                  const ssk::RowScale<true, true>* rs = nullptr) {
    if (ut && !pl.tab_ok) return -8;
    return fuse ? ssdispatch::conv<true>(HostLaunch{}, form, pl, p, n_units, ut, hs, rs)
                : ssdispatch::conv<false>(HostLaunch{}, form, pl, p, n_units, ut, hs, rs);
}
// the one-block log-mel launch as the library shapes and dispatches it (launch_conv_mel of ss_hip.hip); *plan_out: the plan it ran;
// -4: the plan refuses the launch
int run_conv_mel(Form form, ssk::ConvParams& p, const ssk::MelArgs& m, int ss2, int n_units, int flags,
                 const ssk::SpecScale<true, true>* hs = nullptr, const ssk::RowScale<true, true>* rs = nullptr,
                 sslaunch::ConvPlan* plan_out = nullptr) {
    const sslaunch::ConvPlan pl = sslaunch::plan_conv_mel(form, ss2, flags, p.rir_cap, p.h_blocks, p.n_buckets, p.fade_len, n_units);
    if (plan_out) *plan_out = pl;
    if (pl.rc) return -4;
    sslaunch::apply(pl, p);
    return ssdispatch::conv_mel(HostLaunch{}, form, pl, p, m, hs, rs);
}

// k_obs_blocks as sslaunch::plan_obs_blocks shapes it: the plan sees a chip of exactly the (row, block, part) workgroups the
// test wants, so that its own rule arrives at `parts_log2`; the hand-off area at the plan's sizes; the workgroups run in
// blockIdx order with xcd_map = 0 - (row, j - 1) before (row, j): producers before consumers - or reversed.
// The instantiation: ssdispatch::obs_blocks for `form` (mel / hs / rs: as there).  -3: the plan does not take the launch (a
// cross-fade, n_valid < out_len).
int run_obs_blocks(ssk::ConvParams& p, Form form, int n_units, int flags, int parts_log2, const ssk::MelArgs* mel = nullptr,
                   const ssk::SpecScale<true, true>* hs = nullptr, const ssk::RowScale<true>* rs = nullptr, int epoch = 7,
                   bool reversed = false, std::vector<int>* flags_out = nullptr) {
    const int wanted = (2 * n_units * ssroute::ceil_div(p.out_len, ssk::kB)) << parts_log2;
    const sslaunch::ObsBlocksPlan pl = sslaunch::plan_obs_blocks(flags, p.out_len, p.n_valid, n_units, wanted, 1, true, sslaunch::Switches());
    if (!pl.ok) return -3;
    if (form == Form::kSpec16) p.n_buckets = 1;
    sslaunch::apply(pl, p);
    p.xcd_map = 0;
    std::vector<float> tails(pl.handoff_floats, 12345.0f);
    std::vector<int> fl(pl.handoff_flags, 0);
    const int rc = ssdispatch::obs_blocks(HostLaunch{reversed}, form, pl.grid, p, 2 * n_units, tails.data(), fl.data(), epoch, mel, hs, rs, nullptr);
    if (flags_out) flags_out->swap(fl);
    return rc;
}

// k_obs_rows as sslaunch::plan_obs_rows shapes it: `wgs` persistent workgroups are the plan's CUs (parts_log2 > 0: one workgroup
// per (row, part), whatever `wgs` says), the stash of a time-domain bank at the plan's size, filled with `fill`.
// The instantiation: ssdispatch::obs_rows for `form`.  -2: the plan refuses the launch.
int run_obs_rows(ssk::ConvParams& p, Form form, int n_units, int flags, int wgs, int parts_log2, float fill,
                 const ssk::MelArgs* mel = nullptr, const ssk::SpecScale<true, true>* hs = nullptr, const ssk::RowScale<true>* rs = nullptr,
                 int xcd_map = -1) {
    const bool spectral = form != Form::kRows && form != Form::kRows16;
    if (form == Form::kSpec16) p.n_buckets = 1;
    const sslaunch::ObsRowsPlan pl = sslaunch::plan_obs_rows(spectral, false, false, flags, p.n_valid, p.n_buckets, sslaunch::rows_nbh_max(p),
                                                             n_units, parts_log2 ? (2 * n_units) << parts_log2 : wgs, 1,
                                                             forced_parts(parts_log2));
    if (pl.rc) return -2;
    sslaunch::apply(pl, p);
    p.xcd_map = xcd_map >= 0 ? xcd_map : pl.grid >= 8;
    std::vector<float> stash(pl.stash_bytes / sizeof(float), fill);
    if (!spectral) p.stash = reinterpret_cast<ssk::f32x4*>(stash.data());
    return ssdispatch::obs_rows(HostLaunch{}, form, (flags & SS_FLAG_CROSSFADE) != 0, pl.grid, p, 2 * n_units, mel, hs, rs);
}
}  // namespace

// a second length bucket for the next hs_conv / hs_obs_rows call (cleared by it): entries >= first live in `rir` [n,2,cap]
static int g_spec_n_valid = -1;
static int g_parts_log2 = 0;          // the next fused hs_conv / hs_conv_spec / hs_obs_rows call: 2^k workgroups per row (cleared by it)
static const float* g_b2_rir = nullptr;
static int g_b2_first = 0, g_b2_cap = 0;
static void apply_bucket2(ssk::ConvParams& p) {
    if (g_b2_rir) {
        p.n_buckets = 2;
        p.bk[0] = ssk::BankBucket{g_b2_rir, nullptr, g_b2_first, g_b2_cap, ssroute::ceil_div(g_b2_cap, ssk::kB), 0};
    }
    g_b2_rir = nullptr;
}

void hostsim_syncthreads() { barrier_wait(g_block_barrier, g_nthreads); }
void hostsim_wave_sync() { barrier_wait(g_wave_barrier[g_cur / 64], 64); }
static float g_xch[16][64];
float hostsim_lane_read(float v, int src_lane) {
    const int w = g_cur / 64;
    g_xch[w][g_cur % 64] = v;
    hostsim_wave_sync();
    const float r = g_xch[w][src_lane];
    hostsim_wave_sync();
    return r;
}

// window spectra / block spectra: one workgroup per descriptor row
static int run_source_windows(const float* src, const int* desc, float* spec, int n_windows, float scale, bool core32) {
    ssk::SrcParams p;
    p.src = src; p.desc = desc; p.spec = reinterpret_cast<ssk::f32x4*>(spec); p.tb = host_tables();
    p.desc_stride = 4; p.scale = scale;
    if (core32) return run_grid(n_windows, 1, ssk::kT32, [&] { ssk::k_source_windows32(p); });
    return run_grid(n_windows, 1, ssk::kT, [&] { ssk::k_source_windows(p); });
}

extern "C" {

void hs_set_bucket2(const float* rir, int first, int cap) { g_b2_rir = rir; g_b2_first = first; g_b2_cap = cap; }
// the next hs_spectrogram call: rows are known to be zero from sample n_valid on (the library's own two-launch path)
void hs_set_spec_n_valid(int n_valid) { g_spec_n_valid = n_valid; }
void hs_set_parts_log2(int k) { g_parts_log2 = k; }
// the next hs_obs_rows call runs k_obs_blocks (one workgroup per OUTPUT BLOCK of a row, tails handed over through memory)
static int g_obs_blocks = 0;
void hs_set_obs_blocks(int on) { g_obs_blocks = on; }

int hs_source_windows(const float* src, const int* desc, float* spec, int n_windows) {
    return run_source_windows(src, desc, spec, n_windows, ssk::kWindowScale, false);
}

int hs_conv(int fuse, int simple, const float* spec, const float* rir, const int* rir_len, const int* desc, float* out,
            float* sgram, int n_units, long long us, int cs, int es, int cap, int n_valid, int out_len, int pad_mode,
            int persist) {
    using V = sslaunch::Variant;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_rows(p, rir, us, cs, es, cap);
    apply_bucket2(p);
    const bool xfade = simple == 2;                     // simple: 0 = loop kernel, 1 = SIMPLE, 2 = loop kernel + XFADE
    if (xfade) simple = 0;
    // the caller chooses the kernel; the flags under which the library's plan chooses the same one
    const int flags = (simple ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0) | (xfade ? SS_FLAG_CROSSFADE : 0);
    const int nb_y = sslaunch::nb_y_of(n_valid);
    // WIDE: a row longer than one block of which only block 0 is rendered
    const bool wide = fuse && ssroute::wide_one_block_ok(out_len, n_valid, flags, false, ssroute::Switches());
    if (wide && simple) return -3;
    if (fuse && !wide && (nb_y != 1 || out_len > ssk::kB || p.t4 > 26)) return -1;
    // k_conv_rows: `persist` workgroups walk the 2*n_units rows - the plan's CUs
    if (persist > 0 && (fuse || !simple || nb_y != 1 || es != 1 || (cap & 1) || cap > ssk::kB)) return -2;
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(sslaunch::Form::kRows, fuse, wide, flags, cap, 0, p.n_buckets, p.fade_len, persist > 0,
                                                      false, n_units, nb_y, persist > 0 ? persist : kBigChip, 1, forced_parts(g_parts_log2));
    if (pl.rc) return -1;
    g_parts_log2 = 0;
    sslaunch::apply(pl, p);
    if (persist > 0 && pl.variant != V::kPersistRows)   // not the plan's choice (no more rows than workgroups): the test's, one workgroup per row
        return run_grid(2 * n_units, 1, ssk::kT, [&] { ssk::k_conv_rows(p, 2 * n_units); });
    return dispatch_conv(fuse, Form::kRows, pl, p, n_units);
}

// ---- 512-thread core (ss_kernels32.hpp): window spectra in ITS order + the loop-free row kernel
int hs_source_windows32(const float* src, const int* desc, float* spec, int n_windows) {
    return run_source_windows(src, desc, spec, n_windows, ssk::kWindowScale, true);
}

int hs_conv32(int fuse, const float* spec, const float* rir, const int* rir_len, const int* desc, float* out,
              float* sgram, int n_units, long long us, int cs, int es, int cap, int n_valid, int out_len, int pad_mode,
              int use_tab) {
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_rows(p, rir, us, cs, es, cap);
    p.n_terms = 1;
    p.fade_len = 0;
    apply_bucket2(p);
    if (n_valid > ssk::kB || cap > ssk::kB || (fuse && (out_len > ssk::kB || p.t4 > 26))) return -1;
    ssk::UnitTab<true> ut;
    if (use_tab) {
        if (n_units > ssk::kTabUnits) return -2;
        fill_tab_reversed(ut, desc, n_units);
    }
    return run_grid(2 * n_units, 1, ssk::kT32, [&] {
        if (fuse) { if (use_tab) ssk::k_conv32<true, true>(p, ut); else ssk::k_conv32<true, false>(p); }
        else { if (use_tab) ssk::k_conv32<false, true>(p, ut); else ssk::k_conv32<false, false>(p); }
    });
}

// spectral RIR bank: block spectra of every (entry, ear), like ss_rir_spectra_f32 (k_source_windows with scale 1)
int hs_rir_spectra(const float* rir, float* hspec, int n_entries, long long us, int cs, int cap) {
    const int hb = ssroute::ceil_div(cap, ssk::kB);
    std::vector<int> desc;
    for (int r = 0; r < n_entries; ++r)
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < hb; ++i) {
                const int left = cap - i * ssk::kB;
                desc.push_back(static_cast<int>(r * us + (long long)c * cs + (long long)i * ssk::kB));
                desc.push_back(left < ssk::kB ? left : ssk::kB);
                desc.push_back(0);
                desc.push_back(0);
            }
    return run_source_windows(rir, desc.data(), hspec, static_cast<int>(desc.size() / 4), 1.0f, false);
}

int hs_conv_spec(int fuse, int simple, const float* spec, const float* hspec, const int* rir_len, const int* desc,
                 float* out, float* sgram, int n_units, int h_blocks, int n_valid, int out_len, int pad_mode, int persist) {
    using V = sslaunch::Variant;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_spectra(p, hspec, h_blocks);
    p.fade_len = 0;
    apply_bucket2(p);
    const int flags = simple ? SS_FLAG_NO_DISTRACTOR | SS_FLAG_FIRST_BUCKET : 0;
    const int nb_y = sslaunch::nb_y_of(n_valid);
    // the shapes the WIDE rule takes are let through as well (asked as of time-domain rows: no spectral launch is wide)
    const bool wide = fuse && ssroute::wide_one_block_ok(out_len, n_valid, flags, false, ssroute::Switches());
    if (wide && simple) return -3;
    if (fuse && !wide && (nb_y != 1 || out_len > ssk::kB || p.t4 > 26)) return -1;
    if (simple && (nb_y != 1 || h_blocks != 1)) return -2;
    if (persist > 0 && (fuse || !simple)) return -3;    // k_conv_spec_rows: `persist` workgroups walk the units - the plan's CUs
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(sslaunch::Form::kSpec, fuse, false, flags, 0, h_blocks, p.n_buckets, p.fade_len, false,
                                                      persist > 0, n_units, nb_y, persist > 0 ? persist : kBigChip, 1,
                                                      forced_parts(fuse ? g_parts_log2 : 0));
    if (pl.rc) return -1;
    sslaunch::apply(pl, p);
    if (persist > 0 && pl.variant != V::kPersistRows)   // not the plan's choice (no more units than workgroups): the test's, one workgroup per unit
        return run_grid(n_units, 1, ssk::kT, [&] { ssk::k_conv_spec_rows(p, 2 * n_units); });
    if (persist <= 0) g_parts_log2 = 0;
    return dispatch_conv(fuse, Form::kSpec, pl, p, n_units);
}

// k_obs_rows: `wgs` persistent workgroups walk the (unit, ear) rows; hspec != nullptr selects the spectral-bank variant
int hs_obs_rows(const float* spec, const float* rir, const float* hspec, const int* rir_len, const int* desc, float* out,
                float* sgram, int n_units, long long us, int cs, int es, int cap, int h_blocks, int n_valid, int out_len,
                int pad_mode, int wgs, int no_distractor, int use_stash, int crossfade) {
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB || !sgram) return -1;
    ssk::ConvParams p = conv_params(spec, rir_len, desc, out, sgram, n_valid, out_len, pad_mode);
    set_rows(p, rir, us, cs, es, cap);
    if (crossfade && (hspec || no_distractor || p.fade_len > 2 * ssk::kPrevPairs - 2)) return -2;
    set_spectra(p, hspec, h_blocks);
    apply_bucket2(p);
    const int flags = (no_distractor ? SS_FLAG_NO_DISTRACTOR : 0) | (crossfade ? SS_FLAG_CROSSFADE : 0);
    const int parts_log2 = g_parts_log2;                // split rows: one workgroup per (row, part), whatever `wgs` says
    g_parts_log2 = 0;
    const int n_rows = 2 * n_units;
    const Form form = hspec ? Form::kSpec : Form::kRows;
    (void)use_stash;                                    // (the time-domain path always has its stash)
    if (g_obs_blocks) {
        const bool reversed = g_obs_blocks == 2;        // consumers BEFORE producers: every hand-off wait runs out (poisoned frames)
        g_obs_blocks = 0;
        std::vector<int> fl;
        const int rc = run_obs_blocks(p, form, n_units, flags, parts_log2, nullptr, nullptr, nullptr, 7, reversed, &fl);
        if (rc) return rc;
        for (int r = 0; r < n_rows; ++r)                // every hand-off of a non-silent row was released exactly once
            for (int j = 0; j + 1 < p.nb_y; ++j)
                if (fl[static_cast<size_t>(r) * (p.nb_y - 1) + j] != 7 && fl[static_cast<size_t>(r) * (p.nb_y - 1) + j] != 0) return -4;
        return 0;
    }
    return run_obs_rows(p, form, n_units, flags, wgs, parts_log2, 12345.0f, nullptr, nullptr, nullptr, wgs >= 8);
}

// the stand-alone feature kernels: gpw = the groups one workgroup should walk (sslaunch::plan_frames clamps it)
int hs_spectrogram(const float* x, float* out, int n_units, int len, int pad_mode, int gpw) {
    ssk::SpecParams p;
    p.x = x; p.out = out; p.tb = host_tables();
    const int n_valid = g_spec_n_valid >= 0 ? g_spec_n_valid : len;
    g_spec_n_valid = -1;
    if (len < 1) return -2;                             // (the entry points' own argument checks, here and below)
    const sslaunch::FramesPlan pl = sslaunch::plan_frames(sslaunch::Frames::kPooled, n_units, len, n_valid, gpw);
    p.len = len; p.n_frames = pl.n_frames; p.t4 = pl.t4; p.pad_mode = pad_mode; p.live = pl.live; p.gpw = pl.gpw;
    return run_grid(pl.grid, 1, 512, [&] { ssk::k_spectrogram(p); });
}

int hs_logmel(const float* x, float* out, int n_units, int len, int pad_mode, const int* start, const float* w,
              int n_mels, int max_len, float eps, int gpw) {
    ssk::MelParams p;
    p.x = x; p.out = out; p.tb = host_tables(); p.start = start; p.w = w;
    p.n_mels = n_mels; p.max_len = max_len; p.eps = eps;
    if (len < 1 || n_mels < 1 || n_mels > ssk::kMelMaxBands || max_len > ssk::kMelMaxLen || (max_len & 3) || n_mels * max_len > ssk::kMelTableFloats) return -2;
    const sslaunch::FramesPlan pl = sslaunch::plan_frames(sslaunch::Frames::kSegments, n_units, len, len, gpw);
    p.len = len; p.n_frames = pl.n_frames; p.pad_mode = pad_mode; p.gpw = pl.gpw;
    return run_grid(pl.grid, 1, 512, [&] { ssk::k_logmel(p); });
}

int hs_gccphat(const float* x, float* out, int n_units, int len, int pad_mode, int max_lag, float eps, int gpw) {
    ssk::GccParams p;
    p.x = x; p.out = out; p.tb = host_tables();
    p.max_lag = max_lag; p.eps = eps;
    if (len < 1 || max_lag < 1 || max_lag > ssk::kGccMaxLag) return -2;
    const sslaunch::FramesPlan pl = sslaunch::plan_frames(sslaunch::Frames::kSegments, n_units, len, len, gpw);
    p.len = len; p.n_frames = pl.n_frames; p.pad_mode = pad_mode; p.gpw = pl.gpw;
    return run_grid(pl.grid, 1, 256, [&] { ssk::k_gccphat(p); });
}

int hs_features(const float* x, int n_units, int len, int pad_mode, float* sgram, float* mel, const int* start, const float* w,
                int n_mels, int max_len, float mel_eps, float* gcc, int max_lag, float gcc_eps, int gpw) {
    ssk::FeatParams p;
    p.x = x; p.sgram = sgram; p.mel = mel; p.gcc = gcc; p.tb = host_tables(); p.mel_start = start; p.mel_w = w;
    p.n_mels = mel ? n_mels : 0; p.max_len = mel ? max_len : 4; p.max_lag = gcc ? max_lag : 1;
    p.mel_eps = mel_eps; p.gcc_eps = gcc_eps;
    if (len < 1 || (!sgram && !mel && !gcc)) return -2;
    if (mel && (n_mels < 1 || n_mels > ssk::kFeatMaxMels || max_len > ssk::kFeatMaxLen || (max_len & 3) || n_mels * max_len > ssk::kFeatMelTable)) return -2;
    if (gcc && (max_lag < 1 || max_lag > ssk::kGccMaxLag)) return -2;
    p.len = len; p.n_frames = sslaunch::n_frames_of(len); p.t4 = sslaunch::t4_of(len); p.pad_mode = pad_mode;
    p.n_units = n_units;
    // gpw: rounds per workgroup wanted -> at most ceil(tasks / gpw) resident workgroups
    const int tasks = n_units * sslaunch::groups_of(sslaunch::Frames::kSegments, len), per_wg = gpw < 1 ? 1 : gpw;
    const int wgs = sslaunch::features_grid(n_units, len, (tasks + per_wg - 1) / per_wg);
    const int which = (mel ? 1 : 0) | (sgram ? 2 : 0) | (gcc ? 4 : 0);
    return run_grid(wgs, 1, 256, [&] {
        switch (which) {
            case 1: ssk::k_features<true, false, false>(p); break;
            case 2: ssk::k_features<false, true, false>(p); break;
            case 3: ssk::k_features<true, true, false>(p); break;
            case 4: ssk::k_features<false, false, true>(p); break;
            case 5: ssk::k_features<true, false, true>(p); break;
            case 6: ssk::k_features<false, true, true>(p); break;
            default: ssk::k_features<true, true, true>(p); break;
        }
    });
}

int hs_intensity(const float* x, float* out, int n_units, int len, int num_frame) {
    ssk::IntensityParams p;
    p.x = x; p.out = out; p.len = len; p.num_frame = num_frame;
    return run_grid(n_units, 1, 256, [&] { ssk::k_intensity(p); });
}

}  // extern "C"
