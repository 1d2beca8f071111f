// ss_hip.hip — host side of libss_hip.so: table construction and kernel launches (gfx950 only).
// A launch of the four hot kernel families is three steps: plan (ss_route.hpp decides which launch, ss_launch.hpp its geometry),
// acquire the resources the plan sizes (unit table, stash, hand-off area), dispatch (ss_dispatch.hpp decides which instantiation
// and hands it to StreamLaunch below) - no instantiation of those families is named in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iterator>
#include <map>
#include <mutex>
#include <utility>
#include <new>
#include <string>
#include <vector>

#include "../../include/ss_hip.h"
#include "ss_context.hpp"
#include "ss_kernels.hpp"
#include "ss_kernels32.hpp"
#include "ss_route.hpp"
#include "ss_launch.hpp"
#include "ss_dispatch.hpp"
#include "ss_features.hpp"
#include "ss_tables.hpp"
#include "ss_wavio.hpp"

namespace {

constexpr int kMaxDevices = 64;
struct DeviceTables {
    bool ready = false;
    ssk::Tables tb{};
    int n_cus = 0;
};
DeviceTables g_tables[kMaxDevices];
std::mutex g_mu;

inline int hip_err(hipError_t e) { return e == hipSuccess ? 0 : -static_cast<int>(e); }

// A/B switches for benchmarking (scripts/gpu_ab_*.sh) exist only in -DSS_AB builds: the product library reads no
// environment variables ("benchmark knobs inside a shipped .so")
#if defined(SS_AB)
inline bool ab_flag(const char* name) { return std::getenv(name) != nullptr; }
inline int ab_int(const char* name, int dflt) { const char* v = std::getenv(name); return v ? std::atoi(v) : dflt; }
#else
constexpr bool ab_flag(const char*) { return false; }
constexpr int ab_int(const char*, int dflt) { return dflt; }
#endif

// Host time of one ss_ctx_observe call by segment (A/B builds only; ss_ab_host_profile reads and clears the sums)
#if defined(SS_AB)
double g_prof_ns[8] = {0};
long long g_prof_calls = 0;
struct ProfClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(int seg) {
        const auto n = std::chrono::steady_clock::now();
        g_prof_ns[seg] += std::chrono::duration<double, std::nano>(n - t).count();
        t = n;
    }
};
#define SS_PROF_BEGIN() ProfClock prof_clock
#define SS_PROF_MARK(seg) prof_clock.mark(seg)
#define SS_PROF_CALL() (++g_prof_calls)
#else
#define SS_PROF_BEGIN() ((void)0)
#define SS_PROF_MARK(seg) ((void)0)
#define SS_PROF_CALL() ((void)0)
#endif

int get_tables(ssk::Tables* out, int* n_cus = nullptr) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e);
    if (dev < 0 || dev >= kMaxDevices) return SS_EINVAL;
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceTables& d = g_tables[dev];
    if (!d.ready) {
        const std::vector<float> host = ssk_host::build_tables();
        float* dev_buf = nullptr;
        e = hipMalloc(&dev_buf, host.size() * sizeof(float));
        if (e != hipSuccess) return hip_err(e);
        e = hipMemcpy(dev_buf, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(dev_buf); return hip_err(e); }
        d.tb.twM = reinterpret_cast<const ssk::c32*>(dev_buf + ssk_host::kTwMOff);
        d.tb.twItem = reinterpret_cast<const ssk::c32*>(dev_buf + ssk_host::kTwItemOff);
        d.tb.tw512 = reinterpret_cast<const ssk::c32*>(dev_buf + ssk_host::kTw512Off);
        d.tb.win = dev_buf + ssk_host::kWinOff;
        d.tb.twG = reinterpret_cast<const ssk::c32*>(dev_buf + ssk_host::kTwGOff);
        d.tb.twP2 = reinterpret_cast<const ssk::c32*>(dev_buf + ssk_host::kTwP2Off);
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);   // slow call: once per device
        if (e != hipSuccess) { (void)hipFree(dev_buf); return hip_err(e); }
        d.n_cus = cus > 0 ? cus : 1;
        d.ready = true;
    }
    *out = d.tb;
    if (n_cus) *n_cus = d.n_cus;
    return 0;
}

using ssroute::n_frames_of;
using ssroute::t4_of;

// the A/B switches the shape rules of ss_route.hpp take as plain values
inline const ssroute::Switches& route_switches() {
    static const ssroute::Switches sw{ab_flag("SS_HIP_NO_WIDE")};      // (A/B builds only: -DSS_AB)
    return sw;
}

// What a launch is given besides its parameters.
struct LaunchEnv {
    hipStream_t st = nullptr;
    // The context API knows the unit descriptors of a step on the HOST (it has just planned them): loop-free launches of
    // <= kTabUnits units then carry {index, slot} per unit in the kernel arguments (ConvParams::tab).  Callers of the stateless
    // entry points hand over device pointers only: nullptr.
    const int* host_desc = nullptr;
    // ... and, in its overlap mode, the number of launches it keeps in flight (its lanes): a launch that spreads its rows over
    // idle CUs (parts_log2_for) then leaves the other lanes' launches their share of the chip.  1 for everybody else.
    int share = 1;
    // ... and reads back whether the launch took the unit-table route: such a launch never dereferences its descriptor pointer,
    // so the ring slot the descriptors lie in holds nothing the device reads (ss_ring.hpp).  Set by fill_unit_tab only.  (Every
    // entry point issues ONE launch that consumes descriptors, so one flag per call is enough.)
    bool* tab_taken = nullptr;
};

inline bool fill_unit_tab(ssk::UnitTab<true>& ut, const LaunchEnv& env, int n_units) {
    const int* host_desc = env.host_desc;
    if (!host_desc || n_units > ssk::kTabUnits) return false;
    // Units are dealt to the launch slots SORTED by their window spectrum (stable; silent units last): row_slot() gives every
    // XCD a contiguous range of slots, so the rows that read one 128-KiB spectrum - 128 envs draw from 102 sounds, ~73 distinct
    // per step - meet in ONE L2 instead of pulling it through several (r4 PMC: TCC hit rate 0.55, 1.9 x the algorithmic bytes).
    // Word 2 of an entry = the unit the row's results belong to, so the caller's order of outputs is untouched.
    static const bool no_sort = ab_flag("SS_HIP_NO_SORT");            // (A/B builds only)
    unsigned key[ssk::kTabUnits];                                     // (slot << 8) | unit: 32-bit keys, ~1 us for 128 units
    // (steps of >= 64 units only: with fewer, few rows share a spectrum and the ~2 us of host time per call - measured:
    // 13.9 vs 11.7 us at 128 units - are the bottleneck of a small step, not its bytes)
    bool sortable = !no_sort && n_units >= 64;
    for (int i = 0; i < n_units; ++i) {
        const int* d = host_desc + 8 * i;
        const bool ok = d[0] >= 0 && d[2] <= 0 && d[2] + d[3] > 0;          // window m = 0 of the unit's key is stored
        const int slot = ok ? d[1] - d[2] : 0xffffff;
        if (slot < 0 || slot > 0xffffff) sortable = false;
        key[i] = (static_cast<unsigned>(slot & 0xffffff) << 8) | static_cast<unsigned>(i);
    }
    if (sortable) std::sort(key, key + n_units);
    for (int k = 0; k < n_units; ++k) {
        const int i = sortable ? static_cast<int>(key[k] & 0xffu) : k;
        const int* d = host_desc + 8 * i;
        const bool ok = d[0] >= 0 && d[2] <= 0 && d[2] + d[3] > 0;
        ut.tab[ssk::kTabWords * k] = ok ? d[0] : -1;
        ut.tab[ssk::kTabWords * k + 1] = ok ? d[1] - d[2] : 0;
        ut.tab[ssk::kTabWords * k + 2] = i;
    }
    if (env.tab_taken) *env.tab_taken = true;
    return true;
}

// the A/B switches the launch geometry of ss_launch.hpp takes as plain values (A/B builds only: -DSS_AB)
inline const sslaunch::Switches& launch_switches() {
    static const sslaunch::Switches sw{ab_int("SS_HIP_PARTS_LOG2", -1), ab_flag("SS_HIP_NO_ROW_KERNEL"), ab_flag("SS_HIP_NO_OBS_BLOCKS")};
    return sw;
}

// The launcher ss_dispatch.hpp hands its kernel choice to: the instantiation onto the stream, workgroups of ssk::kT threads
struct StreamLaunch {
    hipStream_t st;
    template <class... A, class... B>
    int operator()(void (*kernel)(A...), dim3 grid, const B&... args) const {
        hipLaunchKernelGGL(kernel, grid, dim3(ssk::kT), 0, st, args...);
        return hip_err(hipGetLastError());
    }
};

// The convolution of whichever bank form the launch reads, fused with the STFT (FUSE) or not: sslaunch::plan_conv decides
// refusal, kernel variant, parts and grid; here the unit table is filled where the plan allows one; ssdispatch::conv picks the
// instantiation.  hs: the scales of a half spectral bank (Form::kSpec16 / kSpec16Buckets), rs: those of half rows (Form::kRows16).
template <bool FUSE>
int launch_conv(sslaunch::Form form, ssk::ConvParams p, int n_units, int nb_y, int flags, int n_cus, const LaunchEnv& env,
                bool wide = false, const ssk::SpecScale<true, true>* hs = nullptr, const ssk::RowScale<true, true>* rs = nullptr) {
    const bool planar = p.rir_elem_stride == 1 && !(p.rir_cap & 1) && !(reinterpret_cast<size_t>(p.rir) & 7) &&
                        !(p.rir_unit_stride & 1) && !(p.rir_chan_stride & 1) && p.rir_cap >= 2;
    const sslaunch::ConvPlan pl = sslaunch::plan_conv(form, FUSE, wide, flags, p.rir_cap, p.h_blocks, p.n_buckets, p.fade_len, planar,
                                                      !(reinterpret_cast<size_t>(p.hspec) & 15), n_units, nb_y, n_cus, env.share,
                                                      launch_switches());
    if (pl.rc) return pl.rc;
    sslaunch::apply(pl, p);
    ssk::UnitTab<true> ut;
    const bool tab = pl.tab_ok && fill_unit_tab(ut, env, n_units);
    return ssdispatch::conv<FUSE>(StreamLaunch{env.st}, form, pl, p, n_units, tab ? &ut : nullptr, hs, rs);
}

// the arguments every half-rows entry refuses before a device is touched
inline bool rows16_bank_ok(const void* rir16, const float* rscale, int cap) {
    return rir16 && rscale && !(reinterpret_cast<size_t>(rir16) & 3) && cap >= 2 && !(cap & 1) && (cap + ssk::kB - 1) / ssk::kB <= 16;
}

// ---- half-precision time-domain rows in length buckets (include/ss_hip.h "... in length buckets") -------------------------------
// the bucket rules of ss_rir_bucket, each bucket under rows16_bank_ok; *hb_max = the deepest bucket's blocks
int rir16_buckets_check(const ss_rir16_bucket* bk, int n_buckets, int* hb_max) {
    if (!bk || n_buckets < 1 || n_buckets > ssk::kMaxBuckets) return SS_EINVAL;
    int hb = 1;
    for (int b = 0; b < n_buckets; ++b) {
        if (!rows16_bank_ok(bk[b].rir16, bk[b].rscale, bk[b].cap) || bk[b].n_entries < 0 || bk[b].first < 0) return SS_EINVAL;
        if (b && bk[b].first < bk[b - 1].first + bk[b - 1].n_entries) return SS_EINVAL;         // ascending, disjoint ranges
        hb = std::max(hb, (bk[b].cap + ssk::kB - 1) / ssk::kB);
    }
    if (bk[0].first != 0) return SS_EINVAL;
    *hb_max = hb;
    return 0;
}

// bucket 0 into rir_cap and the head of rs, the others into p.bk[].rir (halves, read as h16x2) and rs.bk[]
void fill_rir16_buckets(ssk::ConvParams& p, ssk::RowScale<true, true>& rs, const ss_rir16_bucket* bk, int n_buckets) {
    p.rir_cap = bk[0].cap;
    p.n_buckets = n_buckets;
    rs.rir16 = static_cast<const ssk::h16x2*>(bk[0].rir16);
    rs.rscale = bk[0].rscale;
    for (auto& s : rs.bk) s = nullptr;
    for (int b = 1; b < n_buckets; ++b) {
        p.bk[b - 1] = ssk::BankBucket{static_cast<const float*>(bk[b].rir16), nullptr, bk[b].first, bk[b].cap,
                                      (bk[b].cap + ssk::kB - 1) / ssk::kB, 0};
        rs.bk[b - 1] = bk[b].rscale;
    }
}

// ---- k_obs_rows: fused observation for rows longer than one partition block -------------------------------------
// The kernel's workgroups keep the block spectra of the row they are rendering in a private stash (see k_obs_rows).
// Launches on ONE stream run one after the other, so the stash is owned by (device, stream): two streams never share
// one, whatever their launches overlap with.  Grown on demand (first long-row launch of a stream), never shrunk.
struct StashBuf { float* ptr = nullptr; size_t bytes = 0; };
std::map<std::pair<int, hipStream_t>, StashBuf> g_stash;

// is `st` being captured into a graph?  (a stream that cannot be asked counts as refused: SS_EINVAL)
int stream_capturing(hipStream_t st, bool* capturing) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return SS_EINVAL; }
    *capturing = cap != hipStreamCaptureStatusNone;
    return 0;
}

// A growth needed while the stream is being captured is refused (an allocation cannot be part of a capture: ss_stream_reserve,
// or one eager call of the shape, prepares the stream) - sslaunch::scratch_decision, as get_wave_scratch.
int get_stash(hipStream_t st, size_t bytes, float** out) {
    // one handle for a different stream on every thread: two concurrent launches would share one stash
    if (st == hipStreamPerThread) return SS_EINVAL;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e);
    std::lock_guard<std::mutex> lk(g_mu);
    const auto key = std::make_pair(dev, st);
    const auto found = g_stash.find(key);
    if ((found == g_stash.end() ? 0 : found->second.bytes) < bytes) {      // (asked only where the answer matters)
        bool capturing = false;
        if (stream_capturing(st, &capturing)) return SS_EINVAL;
        if (sslaunch::scratch_decision(capturing, found == g_stash.end() ? 0 : found->second.bytes, bytes) == sslaunch::Scratch::kRefuse)
            return SS_EINVAL;
    }
    StashBuf& b = g_stash[key];
    if (b.bytes < bytes) {
        if (b.ptr) {
            e = hipStreamSynchronize(st);                       // earlier launches of this stream still use the old one
            if (e != hipSuccess) return hip_err(e);
            (void)hipFree(b.ptr);
            b.ptr = nullptr; b.bytes = 0;
        }
        e = hipMalloc(reinterpret_cast<void**>(&b.ptr), bytes);
        if (e != hipSuccess) { b.ptr = nullptr; return hip_err(e); }
        b.bytes = bytes;
    }
    *out = b.ptr;
    return 0;
}

// k_obs_blocks' hand-off area per (device, stream): [sslaunch::kSyncRows][2] tails of kTailFloats floats + as many flag words, zeroed once;
// + the replay epoch word behind the flags (sslaunch::handoff_bytes).  `epoch` counts the EAGER launches that used the area (a
// flag holds the epoch of the launch that set it: nothing is reset in between) and travels as a kernel argument.  A launch that
// is being captured into a graph cannot do that - every replay would repeat the argument - so it leaves the host counter alone
// and reads its epoch from the word, which k_sync_next, captured in front of it, moves on at every replay (*epoch_word != null:
// the caller enqueues that pair; the two kinds of epoch never meet, see k_sync_next).  The area cannot be allocated inside a
// capture: without one such a launch is refused (ss_stream_reserve, or one eager call, prepares the stream).
struct SyncBuf { float* tails = nullptr; int* flags = nullptr; int* word = nullptr; int epoch = 0; };
std::map<std::pair<int, hipStream_t>, SyncBuf> g_sync;

// the hand-off area of (dev, st), allocated and zeroed (stream-ordered) where absent; g_mu held; the stream is not capturing
int make_block_sync(int dev, hipStream_t st, SyncBuf** out) {
    SyncBuf& b = g_sync[std::make_pair(dev, st)];
    if (!b.tails) {
        const size_t n_hand = sslaunch::handoff_flags(sslaunch::kSyncRows);
        const size_t bytes = sslaunch::handoff_bytes(sslaunch::kSyncRows);
        void* ptr = nullptr;
        hipError_t e = hipMalloc(&ptr, bytes);
        if (e != hipSuccess) return hip_err(e);
        e = hipMemsetAsync(ptr, 0, bytes, st);                  // (stream-ordered in front of the first launch that reads it)
        if (e != hipSuccess) { (void)hipFree(ptr); return hip_err(e); }
        b.tails = static_cast<float*>(ptr);
        b.flags = reinterpret_cast<int*>(b.tails + n_hand * ssk::kTailFloats);
        b.word = b.flags + n_hand;
        b.epoch = 0;
    }
    *out = &b;
    return 0;
}

int get_block_sync(hipStream_t st, float** tails, int** flags, int* epoch, int** epoch_word) {
    if (st == hipStreamPerThread) return SS_EINVAL;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e);
    bool capturing = false;
    if (stream_capturing(st, &capturing)) return SS_EINVAL;
    std::lock_guard<std::mutex> lk(g_mu);
    if (capturing) {
        const auto it = g_sync.find(std::make_pair(dev, st));
        const size_t have = it != g_sync.end() && it->second.tails ? sslaunch::handoff_bytes(sslaunch::kSyncRows) : 0;
        if (sslaunch::scratch_decision(true, have, sslaunch::handoff_bytes(sslaunch::kSyncRows)) != sslaunch::Scratch::kUse) return SS_EINVAL;
        *tails = it->second.tails; *flags = it->second.flags; *epoch = 0; *epoch_word = it->second.word;
        return 0;
    }
    SyncBuf* b = nullptr;
    const int rc = make_block_sync(dev, st, &b);
    if (rc) return rc;
    b->epoch = b->epoch == 0x7fffffff ? 1 : b->epoch + 1;
    *tails = b->tails; *flags = b->flags; *epoch = b->epoch; *epoch_word = nullptr;
    return 0;
}

// a stream is about to be destroyed (the context's overlap lanes): its stash goes with it (~96 MiB per lane
// leaked by every create / destroy of a context with overlap); the caller has synchronised the stream
void drop_stash(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(g_mu);
    auto sy = g_sync.find(std::make_pair(dev, st));
    if (sy != g_sync.end()) {
        if (sy->second.tails) (void)hipFree(sy->second.tails);
        g_sync.erase(sy);
    }
    auto it = g_stash.find(std::make_pair(dev, st));
    if (it == g_stash.end()) return;
    if (it->second.ptr) (void)hipFree(it->second.ptr);
    g_stash.erase(it);
}

// k_obs_blocks / k_obs_rows behind one launcher: sslaunch::plan_obs_rows gives the refusals and the row kernel's shape,
// sslaunch::plan_obs_blocks says whether the step is small enough for one workgroup per OUTPUT BLOCK of a row (k_obs_blocks:
// the hand-off area of the stream) - else k_obs_rows with its stash.  Plan, scratch, then ssdispatch picks the instantiation.
// form: sslaunch::rows_form's; mel: the log-mel instantiations, same rule, same hand-off area; hs: the scales of the half spectral
// forms; rs: those of half-precision time-domain rows (Form::kRows16).
int launch_obs_rows(sslaunch::Form form, ssk::ConvParams p, int n_units, int flags, int n_cus, const LaunchEnv& env,
                    const ssk::MelArgs* mel = nullptr, const ssk::SpecScale<true, true>* hs = nullptr,
                    const ssk::RowScale<true>* rs = nullptr) {
    using sslaunch::Form;
    const hipStream_t st = env.st;
    const bool spectral = form != Form::kRows && form != Form::kRows16;
    const bool half = form == Form::kSpec16 || form == Form::kSpec16Buckets, rows16 = form == Form::kRows16;
    const int n_rows = 2 * n_units;
    if (form == Form::kSpec16) p.n_buckets = 1;                 // (a bucket-0 launch of half buckets: bucket 0's arrays alone)
    // (the log-mel and half forms: plain rows; half: one allocation, or the bucketed form)
    const sslaunch::ObsRowsPlan pr = sslaunch::plan_obs_rows(spectral, mel || half || rows16, form == Form::kSpec16 || rows16, flags,
                                                             p.n_valid, p.n_buckets, sslaunch::rows_nbh_max(p), n_units, n_cus, env.share,
                                                             launch_switches());
    if (pr.rc) return pr.rc;
    const sslaunch::ObsBlocksPlan pb = sslaunch::plan_obs_blocks(flags, p.out_len, p.n_valid, n_units, n_cus, env.share,
                                                                 st != hipStreamPerThread, launch_switches());
    if (pb.ok) {
        float* tails = nullptr;
        int* fl = nullptr;
        int epoch = 0;
        int* word = nullptr;                                    // a capturing stream: the epoch comes from the area's word
        const int rc = get_block_sync(st, &tails, &fl, &epoch, &word);
        if (rc) return rc;
        sslaunch::apply(pb, p);
        if (word) {                                             // ... which k_sync_next moves on first, at every replay
            hipLaunchKernelGGL(ssk::k_sync_next, dim3(1), dim3(64), 0, st, word);
            const int rc2 = hip_err(hipGetLastError());
            if (rc2) return rc2;
        }
        return ssdispatch::obs_blocks(StreamLaunch{st}, form, pb.grid, p, n_rows, tails, fl, epoch, mel, hs, rs, word);
    }
    sslaunch::apply(pr, p);
    if (!spectral) {                                            // (sized from the deepest bucket and n_terms - half rows as fp32 rows)
        float* buf = nullptr;
        const int rc = get_stash(st, pr.stash_bytes, &buf);
        if (rc) return rc;
        p.stash = reinterpret_cast<ssk::f32x4*>(buf);
    }
    return ssdispatch::obs_rows(StreamLaunch{st}, form, (flags & SS_FLAG_CROSSFADE) != 0, pr.grid, p, n_rows, mel, hs, rs);
}

// ---- log-mel form of the fused one-block kernels (k_conv / k_conv_spec <.., MEL>): one workgroup per row, no unit table ----
// the mel arguments of the fused entries: the limits of ss_audio_features_f32
inline bool mel_args_ok(const float* logmel, const int* mel_start, const float* mel_w, int n_mels, int max_len, float eps) {
    return logmel && mel_start && mel_w && n_mels >= 1 && n_mels <= ssk::kFeatMaxMels && max_len >= 4 &&
           max_len <= ssk::kFeatMaxLen && !(max_len & 3) && n_mels * max_len <= ssk::kFeatMelTable && eps > 0.f &&
           !(reinterpret_cast<size_t>(mel_w) & 15);
}
// ss2: 0 = the one-block row; SoundSpaces 2.0 steps (ss_audio_obs_logmel_ss2_f32): ssroute::obs_logmel_ss2_shape's answer
int launch_conv_mel(sslaunch::Form form, ssk::ConvParams p, const ssk::MelArgs& m, int ss2, int n_units, int flags, hipStream_t st,
                    const ssk::SpecScale<true, true>* hs = nullptr, const ssk::RowScale<true, true>* rs = nullptr) {
    const sslaunch::ConvPlan pl = sslaunch::plan_conv_mel(form, ss2, flags, p.rir_cap, p.h_blocks, p.n_buckets, p.fade_len, n_units);
    if (pl.rc) return pl.rc;
    sslaunch::apply(pl, p);
    return ssdispatch::conv_mel(StreamLaunch{st}, form, pl, p, m, hs, rs);
}

// Waveform scratch of the contexts: ss_ctx_observe_features without an audiogoal buffer, on the shapes the log-mel form does
// not serve, renders into [n, 2, sr] floats the library owns - one buffer per (context, overlap lane), grown on demand, freed
// with the context (drop_wave_scratch) and by ss_release_scratch.  A growth needed while the stream is being captured is
// refused (an allocation cannot be part of a capture: warm the stream up first).
struct WaveScratch { float* ptr = nullptr; size_t floats = 0; int dev = 0; };
std::map<std::pair<const void*, int>, WaveScratch> g_wave_scratch;

int get_wave_scratch(const void* owner, int lane, hipStream_t st, size_t floats, float** out) {
    std::lock_guard<std::mutex> lk(g_mu);
    WaveScratch& b = g_wave_scratch[std::make_pair(owner, lane)];
    if (b.floats < floats) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return SS_EINVAL; }
        if (cap != hipStreamCaptureStatusNone) return SS_EINVAL;
        hipError_t e = hipGetDevice(&b.dev);
        if (e != hipSuccess) return hip_err(e);
        if (b.ptr) {
            e = hipDeviceSynchronize();                         // earlier steps may still read the old buffer
            if (e != hipSuccess) return hip_err(e);
            (void)hipFree(b.ptr);
            b.ptr = nullptr; b.floats = 0;
        }
        e = hipMalloc(reinterpret_cast<void**>(&b.ptr), floats * sizeof(float));
        if (e != hipSuccess) { b.ptr = nullptr; return hip_err(e); }
        b.floats = floats;
    }
    *out = b.ptr;
    return 0;
}

// the context is going away (its streams have been synchronised by the caller or belong to the caller)
void drop_wave_scratch(const void* owner) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto it = g_wave_scratch.begin(); it != g_wave_scratch.end();) {
        if (it->first.first != owner) { ++it; continue; }
        if (it->second.ptr) { (void)hipDeviceSynchronize(); (void)hipFree(it->second.ptr); }
        it = g_wave_scratch.erase(it);
    }
}

template <bool FUSE>
int launch_conv32(ssk::ConvParams& p, int n_units, const LaunchEnv& env) {
    const hipStream_t st = env.st;
    const dim3 grid(2 * n_units), block(ssk::kT32);
    ssk::UnitTab<true> ut;
    if (fill_unit_tab(ut, env, n_units)) hipLaunchKernelGGL((ssk::k_conv32<FUSE, true>), grid, block, 0, st, p, ut);
    else hipLaunchKernelGGL((ssk::k_conv32<FUSE, false>), grid, block, 0, st, p, ssk::UnitTab<false>());
    return hip_err(hipGetLastError());
}

int fill_conv(ssk::ConvParams& p, int* n_cus, const float* spec, const float* rir, const int* rir_len,
                     const int* unit_desc, long long us, int cs, int es, int cap, int n_valid, int out_len,
                     bool need_rir = true) {
    if (!spec || (need_rir && !rir) || !rir_len || !unit_desc) return SS_EINVAL;
    if (n_valid < 0 || out_len <= 0 || n_valid > out_len || n_valid > 3 * ssk::kB) return SS_EINVAL;
    if (es < 1 || cs < 0 || us < 0 || cap < 0) return SS_EINVAL;
    int rc = get_tables(&p.tb, n_cus);
    if (rc) return rc;
    p.spec = reinterpret_cast<const ssk::f32x4*>(spec);
    p.rir = rir;
    p.rir_len = rir_len;
    p.desc = unit_desc;
    p.out = nullptr;
    p.sgram = nullptr;
    p.rir_unit_stride = us;
    p.rir_chan_stride = cs;
    p.rir_elem_stride = es;
    p.rir_cap = cap;
    sslaunch::init_conv_params(p, n_valid, out_len);
    // default on: the two ears of a unit (same window spectrum) share an XCD's L2; SS_HIP_XCD_MAP=0 is the A/B switch
    static const int xcd_map = ab_int("SS_HIP_XCD_MAP", 1);
    p.xcd_map = xcd_map;
#if defined(SS_LADDER)                                     // profiling builds only (scripts/gpu_ladder.sh compiles with -DSS_LADDER)
    static const int dbg = getenv("SS_HIP_DBG") ? atoi(getenv("SS_HIP_DBG")) : 0;
    p.dbg = dbg;
#endif
    return 0;
}


// n_valid: samples from n_valid on are KNOWN to be zero (rows this library rendered itself); len: nothing known
int spectrogram_of_rows(const float* x, float* out, int n_units, int len, int n_valid, int pad_mode, void* stream) {
    if (n_units == 0) return 0;
    if (!x || !out || n_units < 0 || len < 1) return SS_EINVAL;   // any length: the centre padding folds as np.pad does
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
    ssk::SpecParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.x = x;
    p.out = out;
    p.len = len;
    p.pad_mode = pad_mode;
    // large batches: one workgroup walks several groups (tables staged once, next segment prefetched under the math);
    // small batches keep one group per workgroup so that the launch still fills 256 CUs x 2 workgroups
    const sslaunch::FramesPlan pl = sslaunch::plan_frames(sslaunch::Frames::kPooled, n_units, len, n_valid,
                                                          (long long)n_units * sslaunch::groups_of(sslaunch::Frames::kPooled, len) / 2048);
    p.n_frames = pl.n_frames;
    p.t4 = pl.t4;
    p.live = pl.live;
    p.gpw = pl.gpw;
    hipLaunchKernelGGL(ssk::k_spectrogram, dim3(pl.grid), dim3(512), 0,
                       static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}


// ---- length-bucketed RIR bank ---------------------------------------------------------------------------
// buckets[0..n): HOST array; bucket b holds bank entries [first_b, first_b + n_entries_b) as planar rows of cap_b samples
// in an allocation of its own.  Bucket 0 fills the legacy fields of ConvParams, the others p.bk[].
int fill_buckets(ssk::ConvParams& p, const ss_rir_bucket* bk, int n_buckets, bool spectral, int* nbh_max) {
    if (!bk || n_buckets < 1 || n_buckets > ssk::kMaxBuckets) return SS_EINVAL;
    int hb_max = 1;
    for (int b = 0; b < n_buckets; ++b) {
        if (!bk[b].rir || bk[b].cap < 2 || (bk[b].cap & 1) || bk[b].n_entries < 0 || bk[b].first < 0) return SS_EINVAL;
        if (b && bk[b].first < bk[b - 1].first + bk[b - 1].n_entries) return SS_EINVAL;     // ascending, disjoint ranges
        if (spectral && !bk[b].hspec) return SS_EINVAL;
        hb_max = std::max(hb_max, (bk[b].cap + ssk::kB - 1) / ssk::kB);
    }
    if (bk[0].first != 0) return SS_EINVAL;
    p.rir = bk[0].rir;
    p.rir_unit_stride = 2LL * bk[0].cap;
    p.rir_chan_stride = bk[0].cap;
    p.rir_elem_stride = 1;
    p.rir_cap = bk[0].cap;
    p.hspec = spectral ? reinterpret_cast<const ssk::f32x4*>(bk[0].hspec) : nullptr;
    p.h_blocks = spectral ? (bk[0].cap + ssk::kB - 1) / ssk::kB : 0;
    p.n_buckets = n_buckets;
    for (int b = 1; b < n_buckets; ++b)
        p.bk[b - 1] = ssk::BankBucket{bk[b].rir, reinterpret_cast<const ssk::f32x4*>(bk[b].hspec), bk[b].first, bk[b].cap,
                                      (bk[b].cap + ssk::kB - 1) / ssk::kB, 0};
    *nbh_max = hb_max;
    return 0;
}

bool buckets_spectral(const ss_rir_bucket* bk, int n_buckets, int flags) {
    if (!bk || (flags & SS_FLAG_CROSSFADE)) return false;
    for (int b = 0; b < n_buckets; ++b) if (!bk[b].hspec) return false;
    return n_buckets > 0;
}


// ---- length-bucketed bank without time-domain rows: fp32 spectra ("only") or fp16 spectra + scales ("half") --------------
// (include/ss_hip.h "Spectral length buckets").  Everything here is checked on the host before a device is touched.
// *half = the form (every bucket carries scales / none does), *hb_max = the longest bucket's blocks.
int spec_buckets_check(const ss_spec_bucket* bk, int n_buckets, bool* half, int* hb_max) {
    if (!bk || n_buckets < 1 || n_buckets > ssk::kMaxBuckets) return SS_EINVAL;
    const bool h = bk[0].hscale != nullptr;
    int hb = 1;
    for (int b = 0; b < n_buckets; ++b) {
        if (!bk[b].hspec || (bk[b].hscale != nullptr) != h) return SS_EINVAL;                   // one form in every bucket
        if (reinterpret_cast<size_t>(bk[b].hspec) & (h ? 7 : 15)) return SS_EINVAL;             // h16x4 / f32x4 loads
        if (bk[b].cap < 2 || (bk[b].cap & 1) || bk[b].n_entries < 0 || bk[b].first < 0) return SS_EINVAL;
        if (b && bk[b].first < bk[b - 1].first + bk[b - 1].n_entries) return SS_EINVAL;         // ascending, disjoint ranges
        const int blocks = (bk[b].cap + ssk::kB - 1) / ssk::kB;
        if (blocks > 16) return SS_EINVAL;
        hb = std::max(hb, blocks);
    }
    if (bk[0].first != 0) return SS_EINVAL;
    *half = h;
    *hb_max = hb;
    return 0;
}

// bucket 0 into the single-bank fields, the others into p.bk[] (no rows anywhere); the half form's scales into hs
void fill_spec_buckets(ssk::ConvParams& p, ssk::SpecScale<true, true>& hs, const ss_spec_bucket* bk, int n_buckets) {
    p.hspec = static_cast<const ssk::f32x4*>(bk[0].hspec);
    p.h_blocks = (bk[0].cap + ssk::kB - 1) / ssk::kB;
    p.n_buckets = n_buckets;
    hs.hscale = bk[0].hscale;
    for (auto& s : hs.bk) s = nullptr;
    for (int b = 1; b < n_buckets; ++b) {
        p.bk[b - 1] = ssk::BankBucket{nullptr, static_cast<const ssk::f32x4*>(bk[b].hspec), bk[b].first, bk[b].cap,
                                      (bk[b].cap + ssk::kB - 1) / ssk::kB, 0};
        hs.bk[b - 1] = bk[b].hscale;
    }
}

// ---- one launch body behind the observation entries -------------------------------------------------------------------
// A RIR bank in whichever form its holder keeps it: built from the arguments of a C entry, or from a Context (bank_of).
struct Bank {
    const float* rir = nullptr;             // time-domain rows (length buckets that keep rows: bucket 0's)
    long long us = 0;
    int cs = 0, es = 1, cap = 0;
    const void* hspec = nullptr;            // block spectra of the same entries: fp32, or - with hscale - fp16 + a scale per block
    const float* hscale = nullptr;
    int h_blocks = 0;
    const ss_rir_bucket* bk = nullptr;      // length buckets that keep rows (every bucket may carry its fp32 spectra as well) ...
    const ss_spec_bucket* sbk = nullptr;    // ... or hold spectra only, fp32 or half
    int n_buckets = 0;
    bool sbk_rows = false;                  // half `sbk` that also serves rows of 2 or 3 blocks (the *_rows_spec16_buckets entries)
    const void* rir16 = nullptr;            // half-precision time-domain rows [entries][2][cap] + ...
    const float* rscale = nullptr;          // ... one scale per (entry, ear); nothing else is set then but `cap`
    bool rows16_rows = false;               // ... that also serve the fused row kernels (ss_audio_obs_rows_rir16_f32, ss_ctx_set_rir_bank16_rows)
    const ss_rir16_bucket* rbk = nullptr;   // half-precision time-domain rows in length buckets (with n_buckets) ...
    bool rows16_bk = false;                 // ... the form was asked for (rbk may be NULL: refused by render)
};
inline Bank rir16_buckets_bank(const ss_rir16_bucket* rbk, int n_buckets) {
    Bank b;
    b.rbk = rbk; b.n_buckets = n_buckets; b.rows16_bk = true;
    return b;
}
inline Bank rows16_bank(const void* rir16, const float* rscale, int cap, bool fused_rows = false) {
    Bank b;
    b.rir16 = rir16; b.rscale = rscale; b.cap = cap; b.rows16_rows = fused_rows;
    return b;
}
inline Bank rows_bank(const float* rir, long long us, int cs, int es, int cap) {
    Bank b;
    b.rir = rir; b.us = us; b.cs = cs; b.es = es; b.cap = cap;
    return b;
}
inline Bank spec_bank(const void* hspec, int h_blocks, const float* hscale = nullptr) {
    Bank b;
    b.hspec = hspec; b.h_blocks = h_blocks; b.hscale = hscale;
    return b;
}
inline Bank buckets_bank(const ss_rir_bucket* bk, int n_buckets) {
    Bank b = bk && n_buckets >= 1 ? rows_bank(bk[0].rir, 2LL * bk[0].cap, bk[0].cap, 1, bk[0].cap) : Bank();
    b.bk = bk; b.n_buckets = n_buckets;
    return b;
}
inline Bank spec_buckets_bank(const ss_spec_bucket* sbk, int n_buckets, bool half_rows = false) {
    Bank b;
    b.sbk = sbk; b.n_buckets = n_buckets; b.sbk_rows = half_rows;
    return b;
}

// the convolution of whichever form the launch reads: k_conv (time-domain rows), k_conv_spec (fp32 spectra) or its half forms
template <bool FUSE>
int launch_conv_any(const ssk::ConvParams& p, const ssk::SpecScale<true, true>& hs, bool spectral, int n_units, int nb_y, int flags,
                    int n_cus, const LaunchEnv& env) {
    if (!spectral) return launch_conv<FUSE>(sslaunch::Form::kRows, p, n_units, nb_y, flags, n_cus, env);
    return launch_conv<FUSE>(hs.hscale ? sslaunch::Form::kSpec16Buckets : sslaunch::Form::kSpec, p, n_units, nb_y, flags, n_cus, env, false, &hs);
}

// ... and k_obs_blocks / k_obs_rows likewise (sslaunch::rows_form: half buckets whose launch only touches bucket 0 as one allocation)
int launch_rows_any(const ssk::ConvParams& p, const ssk::SpecScale<true, true>& hs, bool spectral, int n_units, int flags, int n_cus,
                    const LaunchEnv& env, const ssk::MelArgs* mel = nullptr) {
    return launch_obs_rows(sslaunch::rows_form(spectral, hs.hscale != nullptr, false, p.n_buckets, flags), p, n_units, flags, n_cus, env,
                           mel, &hs);
}

// One step from bank `b`: the body of every ss_fftconv_binaural_* (want = kConv: the waveform alone), ss_audio_obs_* (kObs: the
// chain of ss_route.hpp - fused one-block, wide, rows, else the convolution into `audiogoal` and k_spectrogram over it) and
// ss_audio_obs_logmel_* entry (the kMel forms: one launch, `mel` set, audiogoal / spectrogram optional), and of the context's step.
// spectral: read the block spectra of a single-allocation bank, not its rows (length buckets decide for themselves: those that
// keep rows when every bucket carries spectra and the step has no cross-fade, spectral buckets always).
// Everything that is refused is refused before a device is touched - this level owns no scratch to fall back on.
int render(const Bank& b, bool spectral, ssroute::Launch want, const float* spec, const int* rir_len, const int* unit_desc,
           float* audiogoal, float* spectrogram, const ssk::MelArgs* mel, int n_units, int n_valid, int out_len, int pad_mode,
           int flags, const LaunchEnv& env) {
    using ssroute::Chain;
    using ssroute::Launch;
    using sslaunch::Form;
    const bool bucketed = b.bk || b.sbk;
    bool half = b.hscale != nullptr;
    int nbh_max = 1;
    if (n_units < 0) return SS_EINVAL;
    const bool rows16 = b.rir16 || b.rscale || b.rows16_bk;
    if (rows16) {                                           // (half rows, one allocation or length buckets: no cross-fade)
        if (b.rows16_bk ? rir16_buckets_check(b.rbk, b.n_buckets, &nbh_max) != 0 : !rows16_bank_ok(b.rir16, b.rscale, b.cap)) return SS_EINVAL;
        if ((flags & SS_FLAG_CROSSFADE) || spectral) return SS_EINVAL;
        // log-mel: one-block rows on both forms, rows of 2 or 3 blocks on one allocation asked for the row kernels
        if (want == Launch::kMelSs2 || (want == Launch::kMelRows && (b.rows16_bk || !b.rows16_rows))) return SS_EINVAL;
        if (!b.rows16_bk) nbh_max = (b.cap + ssk::kB - 1) / ssk::kB;
    } else if (b.sbk) {                                            // (no rows anywhere: a cross-fade has nothing to read)
        if (spec_buckets_check(b.sbk, b.n_buckets, &half, &nbh_max) || (flags & SS_FLAG_CROSSFADE)) return SS_EINVAL;
        spectral = true;
    } else if (b.bk) {
        ssk::ConvParams probe;                              // (the bucket array's own refusals, without the device's tables)
        spectral = buckets_spectral(b.bk, b.n_buckets, flags);
        if (fill_buckets(probe, b.bk, b.n_buckets, spectral, &nbh_max)) return SS_EINVAL;
    } else if (spectral) {
        if (!b.hspec || b.h_blocks < 1) return SS_EINVAL;
        nbh_max = b.h_blocks;
    } else {
        nbh_max = (b.cap + ssk::kB - 1) / ssk::kB;
    }
    if (want != Launch::kConv) {
        if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
        if (out_len < ssk::kNfft / 2 + 1) return SS_EINVAL;
    }
    Chain chain = Chain::kFused;
    int ss2_shape = 0;
    switch (want) {
        case Launch::kConv:
            if (!audiogoal) return SS_EINVAL;
            break;
        case Launch::kObs:
            if (!spectrogram) return SS_EINVAL;
            // half spectral buckets: rows of one partition block (the fused row kernels do not read half bucketed banks)
            // (... but through the entries of their own: Bank::sbk_rows)
            if (b.sbk && half && !b.sbk_rows && (out_len > ssk::kB || t4_of(out_len) > 26)) return SS_EINVAL;
            chain = ssroute::obs_chain(out_len, n_valid, nbh_max, flags, spectral, audiogoal != nullptr, route_switches());
            // half rows: no wide kernel; the row kernels only for a bank bound for them, on the shapes obs_rows_ok gives them
            if (rows16 && chain != Chain::kFused)
                chain = b.rows16_rows && ssroute::obs_rows_ok(out_len, n_valid, nbh_max, flags, false, audiogoal != nullptr) ? Chain::kRows
                                                                                                                            : Chain::kTwo;
            if (chain == Chain::kTwo && !audiogoal) return SS_EINVAL;      // cross-faded long rows hand over through HBM/L2
            break;
        case Launch::kMelOneBlock:
            if (!mel || !ssroute::obs_logmel_shape_ok(out_len, flags)) return SS_EINVAL;
            break;
        case Launch::kMelSs2:
            ss2_shape = ssroute::obs_logmel_ss2_shape(out_len, n_valid, flags, route_switches());
            if (!mel || spectral || bucketed || !ss2_shape) return SS_EINVAL;
            break;
        case Launch::kMelRows:
            if (!mel || (half && bucketed && !b.sbk_rows) || (!spectral && !bucketed && b.cap < 1) ||
                !ssroute::obs_logmel_rows_shape_ok(out_len, n_valid, nbh_max, flags))
                return SS_EINVAL;
            break;
        default:
            return SS_EINVAL;
    }
    ssk::ConvParams p;
    int n_cus = 1;
    const bool rows = (!spectral || b.bk) && !rows16;       // (length buckets that keep rows always describe them)
    int rc = rows ? fill_conv(p, &n_cus, spec, b.rir, rir_len, unit_desc, b.us, b.cs, b.es, b.cap, n_valid, out_len)
                  : fill_conv(p, &n_cus, spec, nullptr, rir_len, unit_desc, 0, 0, 1, 0, n_valid, out_len, false);
    if (rc) return rc;
    ssk::SpecScale<true, true> hs;
    hs.hscale = b.hscale;
    for (auto& sc : hs.bk) sc = nullptr;
    if (b.sbk) fill_spec_buckets(p, hs, b.sbk, b.n_buckets);
    else if (b.bk) rc = fill_buckets(p, b.bk, b.n_buckets, spectral, &nbh_max);
    else if (spectral) { p.hspec = static_cast<const ssk::f32x4*>(b.hspec); p.h_blocks = b.h_blocks; }
    if (rc) return rc;
    p.out = audiogoal;
    const int nb_y = sslaunch::nb_y_of(n_valid);
    if (rows16) {
        ssk::RowScale<true, true> rs{static_cast<const ssk::h16x2*>(b.rir16), b.rscale, {nullptr, nullptr, nullptr}};
        p.rir_cap = b.cap;
        if (b.rows16_bk) fill_rir16_buckets(p, rs, b.rbk, b.n_buckets);
        if (want == Launch::kObs && chain == Chain::kFused) {
            p.pad_mode = pad_mode;
            p.sgram = spectrogram;
            return launch_conv<true>(Form::kRows16, p, n_units, 1, flags, n_cus, env, false, nullptr, &rs);
        }
        if (want == Launch::kObs && chain == Chain::kRows) {
            p.pad_mode = pad_mode;
            p.sgram = spectrogram;
            const ssk::RowScale<true> rs1 = ssdispatch::first_bucket(rs);
            return launch_obs_rows(Form::kRows16, p, n_units, flags, n_cus, env, nullptr, nullptr, &rs1);
        }
        if (want == Launch::kMelOneBlock || want == Launch::kMelRows) {
            p.pad_mode = pad_mode;
            p.sgram = spectrogram;
            if (want == Launch::kMelOneBlock) return launch_conv_mel(Form::kRows16, p, *mel, 0, n_units, flags, env.st, nullptr, &rs);
            const ssk::RowScale<true> rs1 = ssdispatch::first_bucket(rs);
            return launch_obs_rows(Form::kRows16, p, n_units, flags, n_cus, env, mel, nullptr, &rs1);
        }
        rc = launch_conv<false>(Form::kRows16, p, n_units, nb_y, flags, n_cus, env, false, nullptr, &rs);
        if (rc || want == Launch::kConv) return rc;
        return spectrogram_of_rows(audiogoal, spectrogram, n_units, out_len, n_valid, pad_mode, env.st);
    }
    if (want == Launch::kConv) return launch_conv_any<false>(p, hs, spectral, n_units, nb_y, flags, n_cus, env);
    if (want == Launch::kObs && chain == Chain::kTwo) {     // (pad_mode, sgram: as the convolution alone leaves them)
        rc = launch_conv_any<false>(p, hs, spectral, n_units, nb_y, flags, n_cus, env);
        if (rc) return rc;
        return spectrogram_of_rows(audiogoal, spectrogram, n_units, out_len, n_valid, pad_mode, env.st);
    }
    p.pad_mode = pad_mode;
    p.sgram = spectrogram;
    if (want == Launch::kObs) {
        if (chain == Chain::kFused) return launch_conv_any<true>(p, hs, spectral, n_units, 1, flags, n_cus, env);
        if (chain == Chain::kWide) return launch_conv<true>(Form::kRows, p, n_units, 1, flags, n_cus, env, true);
        return launch_rows_any(p, hs, spectral, n_units, flags, n_cus, env);
    }
    // the log-mel forms.  Launches that only touch bucket 0 (one bucket, or SS_FLAG_FIRST_BUCKET) are single-allocation launches
    // on bucket 0's arrays: the single-bank log-mel launchers, loop-free kernels included.
    if (flags & SS_FLAG_FIRST_BUCKET) p.n_buckets = 1;
    if (want == Launch::kMelRows) return launch_rows_any(p, hs, spectral, n_units, flags, n_cus, env, mel);
    const Form form = !spectral ? Form::kRows : half ? Form::kSpec16Buckets : Form::kSpec;
    return launch_conv_mel(form, p, *mel, want == Launch::kMelSs2 ? ss2_shape : 0, n_units, flags, env.st, &hs);
}

// the stateless entries: device pointers only, the whole chip
inline LaunchEnv stateless(void* stream) {
    LaunchEnv env;
    env.st = static_cast<hipStream_t>(stream);
    return env;
}
using ssroute::Launch;

}  // namespace

extern "C" {

int ss_block_len(void) { return ssk::kB; }
int ss_spec_floats(void) { return 2 * ssk::kSpecComplex; }
int ss_version(void) { return 1; }

// Frees the per-(device, stream) scratch k_obs_rows keeps (see get_stash); synchronises the device first.
int ss_release_scratch(void) {
    int cur = 0;
    hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) return hip_err(e);
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = 0;
    for (auto& kv : g_stash) {                                  // every entry's OWN device is synchronised before its free
        if (!kv.second.ptr) continue;
        e = hipSetDevice(kv.first.first);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { rc = hip_err(e); continue; }    // (left allocated: a launch may still be using it)
        (void)hipFree(kv.second.ptr);
        kv.second.ptr = nullptr;
        kv.second.bytes = 0;
    }
    for (auto it = g_stash.begin(); it != g_stash.end();) it = it->second.ptr ? std::next(it) : g_stash.erase(it);
    for (auto& kv : g_sync) {                                   // k_obs_blocks' hand-off areas likewise
        if (!kv.second.tails) continue;
        e = hipSetDevice(kv.first.first);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { rc = hip_err(e); continue; }
        (void)hipFree(kv.second.tails);
        kv.second.tails = nullptr;
    }
    for (auto it = g_sync.begin(); it != g_sync.end();) it = it->second.tails ? std::next(it) : g_sync.erase(it);
    for (auto& kv : g_wave_scratch) {                           // the contexts' waveform scratches (grown again on demand)
        if (!kv.second.ptr) continue;
        e = hipSetDevice(kv.second.dev);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { rc = hip_err(e); continue; }
        (void)hipFree(kv.second.ptr);
        kv.second.ptr = nullptr;
        kv.second.floats = 0;
    }
    for (auto it = g_wave_scratch.begin(); it != g_wave_scratch.end();) it = it->second.ptr ? std::next(it) : g_wave_scratch.erase(it);
    (void)hipSetDevice(cur);
    return rc;
}

// What the rows entries would allocate on their first use for this shape on this stream, now: the device's constant tables,
// k_obs_blocks' hand-off area and k_obs_rows' stash at the largest size a launch of (rir_cap, n_terms) can ask for (one
// workgroup per CU).  Afterwards such launches may be captured on the stream without a warm-up call.
int ss_stream_reserve(void* stream, int out_len, int rir_cap, int n_terms) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (!sslaunch::reserve_args_ok(st != hipStreamPerThread, out_len, rir_cap, n_terms)) return SS_EINVAL;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e);
    bool capturing = false;
    if (stream_capturing(st, &capturing) || capturing) return SS_EINVAL;
    ssk::Tables tb;
    int n_cus = 1;
    int rc = get_tables(&tb, &n_cus);
    if (rc) return rc;
    // (the runtime loads the library's device code on first use: asked for here, not by a first launch inside a capture)
    hipFuncAttributes attr;
    e = hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&ssk::k_sync_next));
    if (e != hipSuccess) return hip_err(e);
    const sslaunch::ObsRowsPlan pr = sslaunch::plan_obs_rows(false, false, false, n_terms == 1 ? SS_FLAG_NO_DISTRACTOR : 0, out_len, 1,
                                                             ssroute::ceil_div(rir_cap, ssk::kB), n_cus, n_cus, 1, launch_switches());
    if (pr.rc) return pr.rc;
    float* stash = nullptr;
    rc = get_stash(st, pr.stash_bytes, &stash);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    SyncBuf* b = nullptr;
    return make_block_sync(dev, st, &b);
}

// The replay epoch word of the stream's hand-off area, after a synchronise of the stream: 0 = no replay yet, -k after replay k
// of captured k_obs_blocks launches (k_sync_next).  For tests and diagnostics.
int ss_stream_replay_epoch(void* stream, int* out) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (!out || st == hipStreamPerThread) return SS_EINVAL;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e);
    const int* word = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const auto it = g_sync.find(std::make_pair(dev, st));
        if (it == g_sync.end() || !it->second.tails) return SS_EINVAL;
        word = it->second.word;
    }
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_err(e);
    return hip_err(hipMemcpy(out, word, sizeof(int), hipMemcpyDeviceToHost));
}

int ss_init(void) {
    ssk::Tables tb;
    return get_tables(&tb);
}

int ss_source_windows_f32(const float* src, const int* win_desc, float* spec_out, int n_windows, void* stream) {
    if (n_windows == 0) return 0;
    if (!src || !win_desc || !spec_out || n_windows < 0) return SS_EINVAL;
    ssk::SrcParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.src = src;
    p.desc = win_desc;
    p.spec = reinterpret_cast<ssk::f32x4*>(spec_out);
    p.desc_stride = 4;
    p.scale = ssk::kWindowScale;
    hipLaunchKernelGGL(ssk::k_source_windows, dim3(n_windows), dim3(ssk::kT), 0,
                       static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}

// window spectra scattered into a pool: desc rows {src_offset, src_len, start, wrap, pool slot}
static int launch_windows_scatter(const float* src, const int* win_desc5, float* pool, int n_windows, hipStream_t st) {
    ssk::SrcParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.src = src;
    p.desc = win_desc5;
    p.spec = reinterpret_cast<ssk::f32x4*>(pool);
    p.desc_stride = 5;
    p.scale = ssk::kWindowScale;
    hipLaunchKernelGGL(ssk::k_source_windows, dim3(n_windows), dim3(ssk::kT), 0, st, p);
    return hip_err(hipGetLastError());
}

int ss_fftconv_binaural_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc,
                            float* out, int n_units, long long rir_unit_stride, int rir_chan_stride,
                            int rir_elem_stride, int rir_cap, int n_valid, int out_len, int flags, void* stream) {
    if (n_units == 0) return 0;
    return render(rows_bank(rir, rir_unit_stride, rir_chan_stride, rir_elem_stride, rir_cap), false, Launch::kConv, spec, rir_len,
                  unit_desc, out, nullptr, nullptr, n_units, n_valid, out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

int ss_spectrogram_f32(const float* x, float* out, int n_units, int len, int pad_mode, void* stream) {
    return spectrogram_of_rows(x, out, n_units, len, len, pad_mode, stream);
}

int ss_logmel_f32(const float* x, float* out, int n_units, int len, int pad_mode, const int* mel_start,
                  const float* mel_w, int n_mels, int max_len, float eps, void* stream) {
    if (n_units == 0) return 0;
    if (!x || !out || !mel_start || !mel_w || n_units < 0 || len < 1) return SS_EINVAL;
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
    if (n_mels < 1 || n_mels > ssk::kMelMaxBands || max_len < 4 || max_len > ssk::kMelMaxLen || (max_len & 3) ||
        n_mels * max_len > ssk::kMelTableFloats || !(eps > 0.f) || (reinterpret_cast<size_t>(mel_w) & 15))
        return SS_EINVAL;
    ssk::MelParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.x = x;
    p.out = out;
    p.start = mel_start;
    p.w = mel_w;
    p.len = len;
    p.n_frames = n_frames_of(len);
    p.pad_mode = pad_mode;
    p.n_mels = n_mels;
    p.max_len = max_len;
    p.eps = eps;
    // (one 111 KB workgroup per CU: ~4 rounds of 256)
    const sslaunch::FramesPlan pl = sslaunch::plan_frames(sslaunch::Frames::kSegments, n_units, len, len,
                                                          (long long)n_units * sslaunch::groups_of(sslaunch::Frames::kSegments, len) / 1024);
    p.gpw = pl.gpw;
    hipLaunchKernelGGL(ssk::k_logmel, dim3(pl.grid), dim3(512), 0, static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}

int ss_gccphat_f32(const float* x, float* out, int n_units, int len, int pad_mode, int max_lag, float eps,
                   void* stream) {
    if (n_units == 0) return 0;
    if (!x || !out || n_units < 0 || len < 1) return SS_EINVAL;
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
    if (max_lag < 1 || max_lag > ssk::kGccMaxLag || !(eps > 0.f)) return SS_EINVAL;
    ssk::GccParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.x = x;
    p.out = out;
    p.len = len;
    p.n_frames = n_frames_of(len);
    p.pad_mode = pad_mode;
    p.max_lag = max_lag;
    p.eps = eps;
    const sslaunch::FramesPlan pl = sslaunch::plan_frames(sslaunch::Frames::kSegments, n_units, len, len,
                                                          (long long)n_units * sslaunch::groups_of(sslaunch::Frames::kSegments, len) / 2048);
    p.gpw = pl.gpw;
    hipLaunchKernelGGL(ssk::k_gccphat, dim3(pl.grid), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}

int ss_audio_features_f32(const float* x, int n_units, int len, int pad_mode, float* spectrogram, float* logmel,
                          const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, float* gccphat,
                          int max_lag, float gcc_eps, void* stream) {
    if (n_units == 0) return 0;
    if (!x || n_units < 0 || len < 1 || (!spectrogram && !logmel && !gccphat)) return SS_EINVAL;
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
    if (logmel && (!mel_start || !mel_w || n_mels < 1 || n_mels > ssk::kFeatMaxMels || max_len < 4 ||
                   max_len > ssk::kFeatMaxLen || (max_len & 3) || n_mels * max_len > ssk::kFeatMelTable || !(mel_eps > 0.f) ||
                   (reinterpret_cast<size_t>(mel_w) & 15)))
        return SS_EINVAL;
    if (gccphat && (max_lag < 1 || max_lag > ssk::kGccMaxLag || !(gcc_eps > 0.f))) return SS_EINVAL;
    ssk::FeatParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.x = x; p.sgram = spectrogram; p.mel = logmel; p.gcc = gccphat;
    p.mel_start = mel_start; p.mel_w = mel_w;
    p.len = len; p.n_frames = n_frames_of(len); p.t4 = t4_of(len); p.pad_mode = pad_mode;
    p.n_mels = logmel ? n_mels : 0; p.max_len = logmel ? max_len : 4; p.max_lag = gccphat ? max_lag : 1;
    p.mel_eps = mel_eps; p.gcc_eps = gcc_eps;
    // two ~80 KiB workgroups per CU: one wave of resident workgroups that share the (unit, group) rounds round-robin (tables
    // staged once per workgroup, the next round's segments prefetched under the current round's math)
    int n_cus = 256;
    { ssk::Tables unused; (void)get_tables(&unused, &n_cus); }
    p.n_units = n_units;
    const dim3 grid(static_cast<unsigned>(sslaunch::features_grid(n_units, len, 2LL * n_cus))), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int which = (logmel ? 1 : 0) | (spectrogram ? 2 : 0) | (gccphat ? 4 : 0);
    switch (which) {
        case 1: hipLaunchKernelGGL((ssk::k_features<true, false, false>), grid, block, 0, st, p); break;
        case 2: hipLaunchKernelGGL((ssk::k_features<false, true, false>), grid, block, 0, st, p); break;
        case 3: hipLaunchKernelGGL((ssk::k_features<true, true, false>), grid, block, 0, st, p); break;
        case 4: hipLaunchKernelGGL((ssk::k_features<false, false, true>), grid, block, 0, st, p); break;
        case 5: hipLaunchKernelGGL((ssk::k_features<true, false, true>), grid, block, 0, st, p); break;
        case 6: hipLaunchKernelGGL((ssk::k_features<false, true, true>), grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL((ssk::k_features<true, true, true>), grid, block, 0, st, p); break;
    }
    return hip_err(hipGetLastError());
}

int ss_audio_obs_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc,
                     float* audiogoal, float* spectrogram, int n_units, long long rir_unit_stride,
                     int rir_chan_stride, int rir_elem_stride, int rir_cap, int n_valid, int out_len,
                     int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    return render(rows_bank(rir, rir_unit_stride, rir_chan_stride, rir_elem_stride, rir_cap), false, Launch::kObs, spec, rir_len,
                  unit_desc, audiogoal, spectrogram, nullptr, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// Log-mel observation in ONE launch, no waveform buffer needed (k_conv<.., MEL>): rows of one partition block only.  Every
// argument is checked before a device is touched - this level owns no scratch to fall back on.
int ss_audio_obs_logmel_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc, float* audiogoal,
                            float* spectrogram, float* logmel, const int* mel_start, const float* mel_w, int n_mels, int max_len,
                            float mel_eps, int n_units, long long rir_unit_stride, int rir_chan_stride, int rir_elem_stride,
                            int rir_cap, int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(rows_bank(rir, rir_unit_stride, rir_chan_stride, rir_elem_stride, rir_cap), false, Launch::kMelOneBlock, spec, rir_len,
                  unit_desc, audiogoal, spectrogram, &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// Log-mel observation of a SoundSpaces 2.0 step in ONE launch (k_conv<.., XFADE, .., WIDE, MEL>), no waveform buffer needed.
// Every argument is checked before a device is touched.
int ss_audio_obs_logmel_ss2_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc, float* audiogoal,
                                float* spectrogram, float* logmel, const int* mel_start, const float* mel_w, int n_mels,
                                int max_len, float mel_eps, int n_units, long long rir_unit_stride, int rir_chan_stride,
                                int rir_elem_stride, int rir_cap, int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(rows_bank(rir, rir_unit_stride, rir_chan_stride, rir_elem_stride, rir_cap), false, Launch::kMelSs2, spec, rir_len,
                  unit_desc, audiogoal, spectrogram, &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// Log-mel observation of rows of 2 or 3 partition blocks in ONE launch (k_obs_blocks<.., MEL> for small steps, else
// k_obs_rows<.., MEL>: launch_obs_rows' own choice, hand-off area and stash).  Every argument is checked before a device is touched.
int ss_audio_obs_logmel_rows_f32(const float* spec, const float* rir, const int* rir_len, const int* unit_desc, float* audiogoal,
                                 float* spectrogram, float* logmel, const int* mel_start, const float* mel_w, int n_mels,
                                 int max_len, float mel_eps, int n_units, long long rir_unit_stride, int rir_chan_stride,
                                 int rir_elem_stride, int rir_cap, int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(rows_bank(rir, rir_unit_stride, rir_chan_stride, rir_elem_stride, rir_cap), false, Launch::kMelRows, spec, rir_len,
                  unit_desc, audiogoal, spectrogram, &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ---- 512-thread FFT core (ss_kernels32.hpp): loop-free rows only; spectra in that core's own register order ----------
int ss_source_windows32_f32(const float* src, const int* win_desc, float* spec_out, int n_windows, void* stream) {
    if (n_windows == 0) return 0;
    if (!src || !win_desc || !spec_out || n_windows < 0) return SS_EINVAL;
    ssk::SrcParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.src = src;
    p.desc = win_desc;
    p.spec = reinterpret_cast<ssk::f32x4*>(spec_out);
    p.desc_stride = 4;
    p.scale = ssk::kWindowScale;
    hipLaunchKernelGGL(ssk::k_source_windows32, dim3(n_windows), dim3(ssk::kT32), 0, static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}

// Rows of ONE block from a time-domain bank of rir_cap <= kB without distractor / cross-fade terms (the loop-free case of
// ss_audio_obs_f32 / ss_fftconv_binaural_f32); spectrogram may be NULL (audiogoal only) or audiogoal may be NULL.
int ss_audio_obs32_f32(const float* spec32, const float* rir, const int* rir_len, const int* unit_desc, float* audiogoal,
                       float* spectrogram, int n_units, long long rir_unit_stride, int rir_chan_stride, int rir_elem_stride,
                       int rir_cap, int n_valid, int out_len, int pad_mode, void* stream) {
    if (n_units == 0) return 0;
    if ((!spectrogram && !audiogoal) || n_units < 0) return SS_EINVAL;
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
    if (n_valid > ssk::kB || rir_cap > ssk::kB || out_len < ssk::kNfft / 2 + 1) return SS_EINVAL;
    ssk::ConvParams p;
    int n_cus = 1;
    int rc = fill_conv(p, &n_cus, spec32, rir, rir_len, unit_desc, rir_unit_stride, rir_chan_stride, rir_elem_stride,
                       rir_cap, n_valid, out_len);
    if (rc) return rc;
    p.pad_mode = pad_mode;
    p.nb_y = 1;
    p.out = audiogoal;
    p.sgram = spectrogram;
    if (spectrogram) {
        if (out_len > ssk::kB || p.t4 > 26) return SS_EINVAL;
        return launch_conv32<true>(p, n_units, stateless(stream));
    }
    return launch_conv32<false>(p, n_units, stateless(stream));
}

int ss_intensity_f32(const float* audiogoal, float* out, int n_units, int len, int num_frame, void* stream) {
    if (n_units == 0) return 0;
    if (!audiogoal || !out || n_units < 0 || len <= 0 || num_frame <= 0) return SS_EINVAL;
    ssk::IntensityParams p;
    p.x = audiogoal;
    p.out = out;
    p.len = len;
    p.num_frame = num_frame;
    hipLaunchKernelGGL(ssk::k_intensity, dim3(n_units), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}


// ---- spectral RIR bank ---------------------------------------------------------------------------------------------
}  // extern "C"
// ss_rir_spectra_f32 for a handful of rows: pinned descriptor blocks (per device), reused behind an event
constexpr int kSmallSpectraWindows = 256;
struct SmallSpectraRing {
    static constexpr int kSlots = 8;
    struct Slot { int* desc = nullptr; hipEvent_t ev = nullptr; } slot[kSlots];
    unsigned next = 0;
};
static std::mutex g_small_mu;
static std::map<int, SmallSpectraRing> g_small_ring;
extern "C" {

int ss_rir_spectra_f32(const float* rir, float* hspec_out, int n_entries, long long rir_unit_stride, int rir_chan_stride,
                       int rir_cap, void* stream) {
    if (n_entries == 0) return 0;
    if (!rir || !hspec_out || n_entries < 0 || rir_cap <= 0 || rir_unit_stride < 0 || rir_chan_stride < 0) return SS_EINVAL;
    const int hb = (rir_cap + ssk::kB - 1) / ssk::kB;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // A HANDFUL of rows (a step's new poses, an eager call's one): descriptors in a small ring of pinned blocks the kernel reads
    // in place - no allocation, no copy, no synchronisation (the general path below does all three per call: ~60 us for one row,
    // which is what an eager call at a new pose paid on top of its file read).  A block is reused after its event has passed.
    if (static_cast<long long>(n_entries) * 2 * hb <= kSmallSpectraWindows &&
        static_cast<long long>(n_entries) * rir_unit_stride < (1LL << 31)) {
        int dev = 0;
        hipError_t e0 = hipGetDevice(&dev);
        if (e0 != hipSuccess) return hip_err(e0);
        std::lock_guard<std::mutex> lk(g_small_mu);
        SmallSpectraRing& ring = g_small_ring[dev];
        SmallSpectraRing::Slot& sl = ring.slot[ring.next++ % SmallSpectraRing::kSlots];
        if (!sl.desc) {
            e0 = hipHostMalloc(reinterpret_cast<void**>(&sl.desc), sizeof(int) * 4 * kSmallSpectraWindows, hipHostMallocDefault);
            if (e0 == hipSuccess) e0 = hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming);
            if (e0 != hipSuccess) { sl.desc = nullptr; (void)hipGetLastError(); }
        } else {
            e0 = hipEventSynchronize(sl.ev);
        }
        if (sl.desc && e0 == hipSuccess) {
            int w = 0;
            for (int r = 0; r < n_entries; ++r)
                for (int c = 0; c < 2; ++c)
                    for (int i = 0; i < hb; ++i, ++w) {
                        const int left = rir_cap - i * ssk::kB;
                        sl.desc[4 * w + 0] = static_cast<int>(r * rir_unit_stride + (long long)c * rir_chan_stride + (long long)i * ssk::kB);
                        sl.desc[4 * w + 1] = left < ssk::kB ? left : ssk::kB;
                        sl.desc[4 * w + 2] = 0;
                        sl.desc[4 * w + 3] = 0;
                    }
            ssk::SrcParams p;
            int rc = get_tables(&p.tb);
            if (rc) return rc;
            p.src = rir;
            p.desc = sl.desc;
            p.spec = reinterpret_cast<ssk::f32x4*>(hspec_out);
            p.desc_stride = 4;
            p.scale = 1.0f;
            hipLaunchKernelGGL(ssk::k_source_windows, dim3(w), dim3(ssk::kT), 0, st, p);
            rc = hip_err(hipGetLastError());
            if (rc == 0) rc = hip_err(hipEventRecord(sl.ev, st));
            return rc;
        }
    }
    // window offsets are int32 words relative to a base pointer: walk the bank in chunks that keep them below 2^31
    long long per = (rir_unit_stride > 0) ? ((1LL << 30) / rir_unit_stride) : n_entries;
    if (per < 1) return SS_EINVAL;
    if (per > 2048) per = 2048;
    std::vector<int> host(static_cast<size_t>(per) * 2 * hb * 4);
    int* dev_desc = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev_desc), host.size() * sizeof(int));
    if (e != hipSuccess) return hip_err(e);
    int rc = 0;
    for (long long r0 = 0; r0 < n_entries && rc == 0; r0 += per) {
        const int cnt = static_cast<int>(n_entries - r0 < per ? n_entries - r0 : per);
        int w = 0;
        for (int r = 0; r < cnt; ++r)
            for (int c = 0; c < 2; ++c)
                for (int i = 0; i < hb; ++i, ++w) {
                    const int left = rir_cap - i * ssk::kB;
                    host[4 * w + 0] = static_cast<int>(r * rir_unit_stride + (long long)c * rir_chan_stride + (long long)i * ssk::kB);
                    host[4 * w + 1] = left < ssk::kB ? left : ssk::kB;       // the block's samples; zero padding beyond
                    host[4 * w + 2] = 0;
                    host[4 * w + 3] = 0;
                }
        e = hipMemcpyAsync(dev_desc, host.data(), sizeof(int) * 4 * static_cast<size_t>(w), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { rc = hip_err(e); break; }
        ssk::SrcParams p;
        rc = get_tables(&p.tb);
        if (rc) break;
        p.src = rir + r0 * rir_unit_stride;
        p.desc = dev_desc;
        p.spec = reinterpret_cast<ssk::f32x4*>(hspec_out) + static_cast<size_t>(r0) * 2 * hb * (ssk::kSpecComplex / 2);
        p.desc_stride = 4;
        p.scale = 1.0f;                                                   // H' = 2 * rFFT, unscaled (S' carries 1/(8M))
        hipLaunchKernelGGL(ssk::k_source_windows, dim3(w), dim3(ssk::kT), 0, st, p);
        rc = hip_err(hipGetLastError());
        if (rc == 0) rc = hip_err(hipStreamSynchronize(st));             // host[] / dev_desc are reused by the next chunk
    }
    (void)hipFree(dev_desc);
    return rc;
}

}  // extern "C"

extern "C" {

int ss_fftconv_binaural_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                                 float* out, int n_units, int h_blocks, int n_valid, int out_len, int flags,
                                 void* stream) {
    if (n_units == 0) return 0;
    return render(spec_bank(hspec, h_blocks), true, Launch::kConv, spec, rir_len, unit_desc, out, nullptr, nullptr, n_units, n_valid,
                  out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

int ss_audio_obs_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                          float* audiogoal, float* spectrogram, int n_units, int h_blocks, int n_valid, int out_len,
                          int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    return render(spec_bank(hspec, h_blocks), true, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr, n_units,
                  n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_logmel_f32 from the spectral bank (k_conv_spec<.., MEL>)
int ss_audio_obs_logmel_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc, float* audiogoal,
                                 float* spectrogram, float* logmel, const int* mel_start, const float* mel_w, int n_mels,
                                 int max_len, float mel_eps, int n_units, int h_blocks, int n_valid, int out_len, int pad_mode,
                                 int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(spec_bank(hspec, h_blocks), true, Launch::kMelOneBlock, spec, rir_len, unit_desc, audiogoal, spectrogram, &m,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

}  // extern "C"

// the arguments the three half entries share (checked before a device is touched): 8-byte loads of four halves
static bool spec16_args_ok(const void* hspec16, const float* hscale, int n_units, int h_blocks, int flags) {
    return hspec16 && hscale && n_units > 0 && h_blocks >= 1 && !(flags & SS_FLAG_CROSSFADE) &&
           !(reinterpret_cast<size_t>(hspec16) & 7);
}

extern "C" {

int ss_fftconv_binaural_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                   const int* unit_desc, float* out, int n_units, int h_blocks, int n_valid, int out_len, int flags,
                                   void* stream) {
    if (n_units == 0) return 0;
    if (!spec16_args_ok(hspec16, hscale, n_units, h_blocks, flags)) return SS_EINVAL;
    return render(spec_bank(hspec16, h_blocks, hscale), true, Launch::kConv, spec, rir_len, unit_desc, out, nullptr, nullptr, n_units,
                  n_valid, out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

// rows of one partition block only (the 16 kHz observation): 257 <= out_len <= kB
int ss_audio_obs_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len, const int* unit_desc,
                            float* audiogoal, float* spectrogram, int n_units, int h_blocks, int n_valid, int out_len, int pad_mode,
                            int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!spec16_args_ok(hspec16, hscale, n_units, h_blocks, flags)) return SS_EINVAL;
    if (out_len > ssk::kB || t4_of(out_len) > 26) return SS_EINVAL;
    return render(spec_bank(hspec16, h_blocks, hscale), true, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

int ss_audio_obs_logmel_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                   const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                   const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int h_blocks, int n_valid,
                                   int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!spec16_args_ok(hspec16, hscale, n_units, h_blocks, flags)) return SS_EINVAL;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(spec_bank(hspec16, h_blocks, hscale), true, Launch::kMelOneBlock, spec, rir_len, unit_desc, audiogoal, spectrogram,
                  &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_logmel_rows_f32 from the spectral bank (k_obs_blocks<true, MEL> / k_obs_rows<true, .., MEL>)
int ss_audio_obs_logmel_rows_spec_f32(const float* spec, const float* hspec, const int* rir_len, const int* unit_desc,
                                      float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                      const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int h_blocks,
                                      int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(spec_bank(hspec, h_blocks), true, Launch::kMelRows, spec, rir_len, unit_desc, audiogoal, spectrogram, &m, n_units,
                  n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ---- half bank, rows of 2 or 3 partition blocks (44.1 / 48 kHz): k_obs_blocks<true, MEL, HALF> / k_obs_rows<true, .., MEL, HALF> ----
// what the two entries refuse on top (the fused row kernels' limits: obs_rows_ok)
static bool spec16_rows_args_ok(const void* hspec16, const float* hscale, int n_units, int h_blocks, int out_len, int flags) {
    return spec16_args_ok(hspec16, hscale, n_units, h_blocks, flags) && h_blocks <= 16 && out_len > ssk::kB && out_len <= 3 * ssk::kB;
}

// ss_audio_obs_spec_f32 for rows of 2 or 3 partition blocks, from a half bank: the same routing (k_obs_blocks while the grid fits
// the chip, k_obs_rows beyond; shapes the fp32 entry hands to the unfused convolution + k_spectrogram go to the half convolution)
int ss_audio_obs_rows_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len, const int* unit_desc,
                                 float* audiogoal, float* spectrogram, int n_units, int h_blocks, int n_valid, int out_len,
                                 int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!spec16_rows_args_ok(hspec16, hscale, n_units, h_blocks, out_len, flags)) return SS_EINVAL;
    return render(spec_bank(hspec16, h_blocks, hscale), true, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_logmel_rows_spec_f32 from a half bank
int ss_audio_obs_logmel_rows_spec16_f32(const float* spec, const void* hspec16, const float* hscale, const int* rir_len,
                                        const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                        const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                        int h_blocks, int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!spec16_rows_args_ok(hspec16, hscale, n_units, h_blocks, out_len, flags)) return SS_EINVAL;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(spec_bank(hspec16, h_blocks, hscale), true, Launch::kMelRows, spec, rir_len, unit_desc, audiogoal, spectrogram, &m,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ---- half-precision time-domain rows: the stateless entries ---------------------------------------------------------------
// ss_fftconv_binaural_f32 on a planar bank of half rows (k_conv<.., HALF>: loop-free or loop kernel, as launch_conv16 decides)
int ss_fftconv_binaural_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                                  float* out, int n_units, int rir_cap, int n_valid, int out_len, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!rows16_bank_ok(rir16, rscale, rir_cap) || (flags & SS_FLAG_CROSSFADE)) return SS_EINVAL;
    return render(rows16_bank(rir16, rscale, rir_cap), false, Launch::kConv, spec, rir_len, unit_desc, out, nullptr, nullptr, n_units,
                  n_valid, out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

// ss_audio_obs_f32's one-launch fused form (the rows the chain calls kFused) from half rows; `audiogoal` may be NULL
int ss_audio_obs_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                           float* audiogoal, float* spectrogram, int n_units, int rir_cap, int n_valid, int out_len, int pad_mode,
                           int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!rows16_bank_ok(rir16, rscale, rir_cap) || (flags & SS_FLAG_CROSSFADE)) return SS_EINVAL;
    if (out_len < ssk::kNfft / 2 + 1 || out_len > ssk::kB || t4_of(out_len) > 26) return SS_EINVAL;
    return render(rows16_bank(rir16, rscale, rir_cap), false, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_rows_f32 from half rows: rows of 2 or 3 partition blocks in one launch (k_obs_blocks / k_obs_rows<.., ROWS16>), the
// shapes obs_rows_ok leaves to two launches (a waveform buffer and one rendered block) through the half convolution + k_spectrogram
int ss_audio_obs_rows_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                                float* audiogoal, float* spectrogram, int n_units, int rir_cap, int n_valid, int out_len, int pad_mode,
                                int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!rows16_bank_ok(rir16, rscale, rir_cap) || (flags & SS_FLAG_CROSSFADE)) return SS_EINVAL;
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB) return SS_EINVAL;
    return render(rows16_bank(rir16, rscale, rir_cap, true), false, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram,
                  nullptr, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// Log-mel observation of one-block rows from half rows in ONE launch (k_conv<.., MEL, HALF>), no waveform buffer needed
int ss_audio_obs_logmel_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len, const int* unit_desc,
                                  float* audiogoal, float* spectrogram, float* logmel, const int* mel_start, const float* mel_w,
                                  int n_mels, int max_len, float mel_eps, int n_units, int rir_cap, int n_valid, int out_len,
                                  int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!rows16_bank_ok(rir16, rscale, rir_cap) || (flags & SS_FLAG_CROSSFADE)) return SS_EINVAL;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(rows16_bank(rir16, rscale, rir_cap), false, Launch::kMelOneBlock, spec, rir_len, unit_desc, audiogoal, spectrogram, &m,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ... of rows of 2 or 3 partition blocks (k_obs_blocks / k_obs_rows<.., MEL, .., ROWS16>: launch_obs_rows' own choice, hand-off
// area and stash)
int ss_audio_obs_logmel_rows_rir16_f32(const float* spec, const void* rir16, const float* rscale, const int* rir_len,
                                       const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                       const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int rir_cap,
                                       int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!rows16_bank_ok(rir16, rscale, rir_cap) || (flags & SS_FLAG_CROSSFADE)) return SS_EINVAL;
    if (out_len <= ssk::kB || out_len > 3 * ssk::kB) return SS_EINVAL;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(rows16_bank(rir16, rscale, rir_cap, true), false, Launch::kMelRows, spec, rir_len, unit_desc, audiogoal, spectrogram,
                  &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ---- half-precision time-domain rows in length buckets: the stateless entries ------------------------------------------------
// ss_fftconv_binaural_rir16_f32 on ss_rir16_bucket[] (k_conv<.., HALF, RBK>; bucket-0 launches: the single-allocation half kernels)
int ss_fftconv_binaural_rir16_buckets_f32(const float* spec, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len,
                                          const int* unit_desc, float* out, int n_units, int n_valid, int out_len, int flags,
                                          void* stream) {
    if (n_units == 0) return 0;
    return render(rir16_buckets_bank(buckets, n_buckets), false, Launch::kConv, spec, rir_len, unit_desc, out, nullptr, nullptr, n_units,
                  n_valid, out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

// ss_audio_obs_rir16_f32 on ss_rir16_bucket[]: the one-launch fused form; `audiogoal` may be NULL
int ss_audio_obs_rir16_buckets_f32(const float* spec, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len,
                                   const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid, int out_len,
                                   int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (out_len < ssk::kNfft / 2 + 1 || out_len > ssk::kB || t4_of(out_len) > 26) return SS_EINVAL;
    return render(rir16_buckets_bank(buckets, n_buckets), false, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_logmel_rir16_f32 on ss_rir16_bucket[]: one-block rows in ONE launch (k_conv<.., MEL, HALF, RBK>; bucket-0 launches:
// the single-allocation half kernels)
int ss_audio_obs_logmel_rir16_buckets_f32(const float* spec, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len,
                                          const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                          const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                          int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(rir16_buckets_bank(buckets, n_buckets), false, Launch::kMelOneBlock, spec, rir_len, unit_desc, audiogoal, spectrogram,
                  &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ---- pose memo: the row copies (k_memo_rows) ---------------------------------------------------------------------------
static bool memo_io_ok(const ss_memo_io* io, int n_io) {
    if (!io || n_io < 1 || n_io > ssk::kMemoArrays) return false;
    for (int a = 0; a < n_io; ++a)
        if (!io[a].out || !io[a].pool || io[a].row_floats < 1 || ((reinterpret_cast<size_t>(io[a].out) | reinterpret_cast<size_t>(io[a].pool)) & 3))
            return false;
    return true;
}

// host_moves: `moves` is a HOST list the launch carries in its kernel arguments, kMemoTabMoves moves at a time (the moves are
// independent of each other: several launches are as good as one); else device-accessible memory the kernel reads in place
static int launch_memo_rows(const ss_memo_io* io, int n_io, const int* moves, bool host_moves, int n_store, int n_fetch, hipStream_t st) {
    ssk::MemoRowsParams p;
    int longest = 1;
    for (int a = 0; a < ssk::kMemoArrays; ++a) {
        const ss_memo_io& x = io[a < n_io ? a : 0];
        p.out[a] = x.out; p.pool[a] = x.pool; p.row_floats[a] = x.row_floats;
        if (x.row_floats > longest) longest = x.row_floats;
    }
    const unsigned gx = static_cast<unsigned>((static_cast<long long>(longest) + ssk::kMemoChunk - 1) / ssk::kMemoChunk);
    const int n = n_store + n_fetch, per = host_moves ? ssk::kMemoTabMoves : 65535;      // (65535: grid.y limit)
    for (int lo = 0; lo < n; lo += per) {
        const int m = n - lo < per ? n - lo : per;
        p.n_store = n_store - lo < 0 ? 0 : (n_store - lo < m ? n_store - lo : m);
        if (host_moves) {
            ssk::MoveTab<true> mt;
            std::memcpy(mt.mv, moves + 2 * static_cast<size_t>(lo), sizeof(int) * 2 * static_cast<size_t>(m));
            p.moves = nullptr;
            hipLaunchKernelGGL(ssk::k_memo_rows<true>, dim3(gx, m, n_io), dim3(256), 0, st, p, mt);
        } else {
            p.moves = moves + 2 * static_cast<size_t>(lo);
            hipLaunchKernelGGL(ssk::k_memo_rows<false>, dim3(gx, m, n_io), dim3(256), 0, st, p, ssk::MoveTab<false>());
        }
    }
    return hip_err(hipGetLastError());
}

int ss_memo_rows_f32(const ss_memo_io* io, int n_io, const int* moves, int n_store, int n_fetch, void* stream) {
    if (n_io < 1 || n_io > ssk::kMemoArrays || n_store < 0 || n_fetch < 0 || n_store > 0x7fffffff - n_fetch) return SS_EINVAL;
    if (n_store + n_fetch == 0) return 0;
    if (!moves || !memo_io_ok(io, n_io)) return SS_EINVAL;
    // the kernel dereferences `moves`: pageable host memory would be a GPU memory fault, not an error code
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, moves) != hipSuccess) { (void)hipGetLastError(); return SS_EINVAL; }
    if (attr.type != hipMemoryTypeHost && attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) return SS_EINVAL;
    return launch_memo_rows(io, n_io, moves, false, n_store, n_fetch, static_cast<hipStream_t>(stream));
}

// ---- context API (include/ss_hip.h): planner + window-spectra cache + descriptor ring inside the library --------------
struct ss_ctx { ssctx::Context c; };

int ss_ctx_create(ss_ctx** out, int sampling_rate, int n_valid, int pad_mode, int wrap_mode, int max_window_sets) {
    if (!out || sampling_rate <= 0 || n_valid < 0 || n_valid > sampling_rate || n_valid > 3 * ssk::kB) return SS_EINVAL;
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return SS_EINVAL;
    ss_ctx* h = new (std::nothrow) ss_ctx();
    if (!h) return SS_EINVAL;
    ssctx::Context& c = h->c;
    c.sr = sampling_rate; c.n_valid = n_valid; c.out_len = sampling_rate; c.pad_mode = pad_mode;
    c.wrap_mode = wrap_mode ? 1 : 0;
    c.kb = ssk::kB; c.spec_floats = 2 * ssk::kSpecComplex;
    c.n_entries = max_window_sets > 0 ? max_window_sets : 256;
    c.stride = n_valid > 0 ? ssctx::ceil_div(n_valid, ssk::kB) : 1;                 // nbh_max (= 1 until a bank is set) + nby - 1
    ssctx::cache_reset(c);
    *out = h;
    return 0;
}

static void ctx_free_device(ssctx::Context& c) {
    if (c.pool) (void)hipFree(c.pool);
    if (c.src_dev) (void)hipFree(c.src_dev);
    if (c.d_desc) (void)hipFree(c.d_desc);
    if (c.d_win) (void)hipFree(c.d_win);
    if (c.h_desc) (void)hipHostFree(c.h_desc);
    if (c.h_win) (void)hipHostFree(c.h_win);
    if (c.ag_scratch) (void)hipFree(c.ag_scratch);
    c.ag_scratch = nullptr; c.ag_cap = 0;
    drop_wave_scratch(&c);
    if (c.ev_made)
        for (int k = 0; k < ssctx::kRing / ssctx::kGroup; ++k) (void)hipEventDestroy(c.ev_done[k]);
    if (c.ev_pace) { (void)hipEventDestroy(c.ev_pace); c.ev_pace = nullptr; }
    if (c.ev_xstream) (void)hipEventDestroy(c.ev_xstream);
    if (c.miss_ev) { (void)hipEventDestroy(static_cast<hipEvent_t>(c.miss_ev)); c.miss_ev = nullptr; }
    c.ev_xstream = nullptr; c.have_last_stream = false;
    if (c.memo_ev_made) {
        for (int l = 0; l < ssctx::kLanes; ++l) (void)hipEventDestroy(c.ev_memo[l]);
        c.memo_ev_made = false;
    }
    if (c.lanes_made) {
        for (int l = 0; l < ssctx::kLanes; ++l) {
            (void)hipStreamSynchronize(c.lane_stream[l]);
            drop_stash(c.lane_stream[l]);                       // k_obs_rows' per-(device, stream) scratch of this lane
            (void)hipEventDestroy(c.ev_lane[l]);
            (void)hipEventDestroy(c.ev_win[l]);
            (void)hipStreamDestroy(c.lane_stream[l]);
        }
        (void)hipEventDestroy(c.ev_in);
        for (int l = 1; l < ssctx::kLanes; ++l)
            for (int k = 0; k < ssctx::kRing / ssctx::kGroup; ++k) (void)hipEventDestroy(c.ev_done_l[l][k]);
        c.lanes_made = false;
    }
    c.pool = nullptr; c.src_dev = nullptr; c.d_desc = nullptr; c.d_win = nullptr; c.h_desc = nullptr; c.h_win = nullptr;
    c.ev_made = false;
}

int ss_ctx_destroy(ss_ctx* h) {
    if (!h) return 0;
    ctx_free_device(h->c);
    delete h;
    return 0;
}

// `clip` is HOST memory unless on_device != 0.  Returns the sound id (>= 0) or a negative error.
int ss_ctx_add_source(ss_ctx* h, const float* clip, int len, int on_device) {
    if (!h || !clip || len <= 0) return SS_EINVAL;
    ssctx::Context& c = h->c;
    const size_t need = c.src_used + static_cast<size_t>(len);
    if (need > c.src_cap) {                                    // grow the flat bank (rare: once per new sound at most)
        size_t cap = c.src_cap ? c.src_cap : (1u << 20);
        while (cap < need) cap *= 2;
        float* nb = nullptr;
        hipError_t e = hipMalloc(&nb, cap * sizeof(float));
        if (e != hipSuccess) return hip_err(e);
        if (c.src_used) {
            e = hipDeviceSynchronize();                        // launches that read the old bank
            if (e == hipSuccess) e = hipMemcpy(nb, c.src_dev, c.src_used * sizeof(float), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { (void)hipFree(nb); return hip_err(e); }
        }
        if (c.src_dev) (void)hipFree(c.src_dev);
        c.src_dev = nb;
        c.src_cap = cap;
    }
    hipError_t e = hipMemcpy(c.src_dev + c.src_used, clip, static_cast<size_t>(len) * sizeof(float),
                             on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_err(e);
    c.src_off.push_back(static_cast<int>(c.src_used));
    c.src_len.push_back(len);
    c.src_used = need;
    return static_cast<int>(c.src_len.size()) - 1;
}

// planning-only registration (tests of the planner on machines without a GPU): lengths only, no device memory
int ss_ctx_add_source_len(ss_ctx* h, int len) {
    if (!h || len <= 0) return SS_EINVAL;
    ssctx::Context& c = h->c;
    c.src_off.push_back(static_cast<int>(c.src_used));
    c.src_len.push_back(len);
    c.src_used += static_cast<size_t>(len);
    return static_cast<int>(c.src_len.size()) - 1;
}

int ss_ctx_set_rir_bank(ss_ctx* h, const float* rir, const int* rir_len, long long unit_stride, int chan_stride,
                        int elem_stride, int rir_cap) {
    if (!h || rir_cap < 0 || elem_stride < 1 || chan_stride < 0 || unit_stride < 0) return SS_EINVAL;
    ssctx::Context& c = h->c;
    const int nbh_old = c.rir_cap > 0 ? ssctx::ceil_div(c.rir_cap, c.kb) : 1;
    const int nbh_new = rir_cap > 0 ? ssctx::ceil_div(rir_cap, c.kb) : 1;
    c.rir = rir; c.rir_len = rir_len; c.rir_us = unit_stride; c.rir_cs = chan_stride; c.rir_es = elem_stride;
    c.rir_cap = rir_cap;
    c.rir16 = nullptr; c.rscale = nullptr;                     // (half rows, ss_ctx_set_rir_bank16: replaced like any other bank)
    c.rir16_buckets.clear();                                   // (... in length buckets, ss_ctx_set_rir16_buckets: likewise)
    // the spectral form described the PREVIOUS bank (its entries, its capacity): back to the time-domain kernels until
    // ss_ctx_set_rir_spectra is called for this one (a swapped / grown bank kept rendering the old spectra)
    c.hspec = nullptr;
    c.hscale = nullptr;
    c.h_blocks = 0;
    c.buckets.clear();
    c.spec_buckets.clear();
    if (nbh_new != nbh_old) {                                  // the set of partition offsets per key changes
        const int nby = c.n_valid > 0 ? ssctx::ceil_div(c.n_valid, c.kb) : 1;
        c.stride = nbh_new + nby - 1;
        ssctx::cache_reset(c);
        if (c.pool) {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_err(e);
            (void)hipFree(c.pool);
            c.pool = nullptr;
            c.pool_entries = 0;
        }
    }
    return 0;
}

// Spectral form of the bank set by ss_ctx_set_rir_bank (same entries, same rir_len): steps without a cross-fade then
// run k_conv_spec.  hspec = NULL switches back to the time-domain kernels.
int ss_ctx_set_rir_spectra(ss_ctx* h, const float* hspec, int h_blocks) {
    if (!h || (hspec && h_blocks < 1)) return SS_EINVAL;
    ssctx::Context& c = h->c;
    if (hspec && h_blocks != (c.rir_cap > 0 ? ssctx::ceil_div(c.rir_cap, c.kb) : 1)) return SS_EINVAL;
    if (hspec && (c.hscale || !c.spec_buckets.empty() || c.rir16 || !c.rir16_buckets.empty())) return SS_EINVAL;     // a half bank (ss_ctx_set_rir_spectra16) or spectral buckets are bound: one form at a time
    c.hspec = hspec;
    c.hscale = nullptr;
    c.h_blocks = hspec ? h_blocks : 0;
    return 0;
}

// Half form of a SPECTRAL-ONLY bank (ss_ctx_set_rir_bank(ctx, NULL, rir_len, 0, 0, 1, rir_cap) first): fp16 block spectra and
// their scales (include/ss_hip.h).  Steps run k_conv_spec<.., HALF>, which serves rows of one partition block: a context whose
// rows are longer, a bank that keeps time-domain rows or buckets, and a context with fp32 spectra bound are refused.
// hspec16 = NULL unbinds.
int ss_ctx_set_rir_spectra16(ss_ctx* h, const void* hspec16, const float* hscale, int h_blocks) {
    if (!h) return SS_EINVAL;
    ssctx::Context& c = h->c;
    if (!hspec16) {
        if (c.hscale) { c.hspec = nullptr; c.hscale = nullptr; c.h_blocks = 0; }
        return 0;
    }
    if (!hscale || h_blocks < 1 || (reinterpret_cast<size_t>(hspec16) & 7)) return SS_EINVAL;
    if (c.out_len > c.kb || c.rir || c.rir16 || !c.rir16_buckets.empty() || !c.buckets.empty() || !c.spec_buckets.empty() || !c.rir_len || (c.hspec && !c.hscale)) return SS_EINVAL;
    if (h_blocks != (c.rir_cap > 0 ? ssctx::ceil_div(c.rir_cap, c.kb) : 1)) return SS_EINVAL;
    c.hspec = static_cast<const float*>(hspec16);              // (read as halves wherever hscale is set)
    c.hscale = hscale;
    c.h_blocks = h_blocks;
    return 0;
}

// The same binding for contexts whose rows have 2 or 3 partition blocks (44.1 / 48 kHz): steps then go to
// ss_audio_obs_rows_spec16_f32 / ss_audio_obs_logmel_rows_spec16_f32 (k_obs_blocks / k_obs_rows <.., HALF>), waveform-only steps
// to ss_fftconv_binaural_spec16_f32.  Same preconditions otherwise; hspec16 = NULL unbinds.
int ss_ctx_set_rir_spectra16_rows(ss_ctx* h, const void* hspec16, const float* hscale, int h_blocks) {
    if (!h) return SS_EINVAL;
    ssctx::Context& c = h->c;
    if (!hspec16) {
        if (c.hscale) { c.hspec = nullptr; c.hscale = nullptr; c.h_blocks = 0; }
        return 0;
    }
    if (!hscale || h_blocks < 1 || h_blocks > 16 || (reinterpret_cast<size_t>(hspec16) & 7)) return SS_EINVAL;
    if (c.out_len <= c.kb || c.out_len > 3 * c.kb) return SS_EINVAL;
    if (c.rir || c.rir16 || !c.rir16_buckets.empty() || !c.buckets.empty() || !c.spec_buckets.empty() || !c.rir_len || (c.hspec && !c.hscale)) return SS_EINVAL;
    if (h_blocks != (c.rir_cap > 0 ? ssctx::ceil_div(c.rir_cap, c.kb) : 1)) return SS_EINVAL;
    c.hspec = static_cast<const float*>(hspec16);              // (read as halves wherever hscale is set)
    c.hscale = hscale;
    c.h_blocks = h_blocks;
    return 0;
}

// Half-precision time-domain rows as the context's bank (include/ss_hip.h "Half-precision time-domain rows"): replaces whatever
// bank was bound (rows, spectra, buckets), rir16 = NULL unbinds.  One-block rows take the fused half kernels, longer ones the half
// convolution + k_spectrogram, log-mel steps the waveform scratch; a cross-faded step is refused (ss_route.hpp, Bank::rows16).
int ss_ctx_set_rir_bank16(ss_ctx* h, const void* rir16, const float* rscale, const int* rir_len, int rir_cap) {
    if (!h) return SS_EINVAL;
    if (!rir16) {
        h->c.rir16 = nullptr; h->c.rscale = nullptr; h->c.rir16_rows = false;
        return 0;
    }
    if (!rir_len || !rows16_bank_ok(rir16, rscale, rir_cap)) return SS_EINVAL;
    const int rc = ss_ctx_set_rir_bank(h, nullptr, rir_len, 0, 0, 1, rir_cap);      // (window keys, pool, every other form: as for any new bank)
    if (rc) return rc;
    h->c.rir16 = rir16;
    h->c.rir16_rows = false;                                   // (ss_ctx_set_rir_bank16_rows sets it behind this call)
    h->c.rscale = rscale;
    return 0;
}

// ... bound for the fused row kernels as well: ss_ctx_set_rir_bank16 plus the route field (ss_route.hpp, Bank::rows16_rows)
int ss_ctx_set_rir_bank16_rows(ss_ctx* h, const void* rir16, const float* rscale, const int* rir_len, int rir_cap) {
    const int rc = ss_ctx_set_rir_bank16(h, rir16, rscale, rir_len, rir_cap);
    if (rc) return rc;
    h->c.rir16_rows = rir16 != nullptr;
    return 0;
}

int ss_ctx_plan(ss_ctx* h, const ss_units* units, int n, int* unit_desc_out, int* flags_out, int* n_new_windows_out,
                int* new_windows_out, int new_windows_cap) {
    if (!h || !unit_desc_out) return SS_EINVAL;
    ssctx::PlanResult res;
    int rc = ssctx::plan_units(h->c, units, n, unit_desc_out, &res);
    if (rc) return rc;
    h->c.plan_only_keys = true;       // keys in the cache whose spectra nobody computes, a tick without a ring slot: the
                                      // next ss_ctx_observe starts from an empty cache (after a device synchronise)
    if (flags_out) *flags_out = res.flags;
    if (n_new_windows_out) *n_new_windows_out = res.n_new_windows;
    if (new_windows_out) {
        const int k = res.n_new_windows < new_windows_cap ? res.n_new_windows : new_windows_cap;
        std::memcpy(new_windows_out, h->c.new_win.data(), sizeof(int) * 5 * static_cast<size_t>(k));
    }
    return 0;
}

int ss_ctx_ring_stats(ss_ctx* h, long long* out4) {
    if (!h || !out4) return SS_EINVAL;
    out4[0] = h->c.ring.n_records; out4[1] = h->c.ring.n_waits;
    out4[2] = h->c.pace.n_records; out4[3] = h->c.pace.n_waits;
    return 0;
}

int ss_ctx_stats(ss_ctx* h, long long* out8) {
    if (!h || !out8) return SS_EINVAL;
    const ssctx::Context& c = h->c;
    out8[0] = c.hits; out8[1] = c.misses; out8[2] = c.evictions; out8[3] = c.grows;
    out8[4] = c.n_entries; out8[5] = static_cast<long long>(c.map.size()); out8[6] = c.stride; out8[7] = c.tick;
    return 0;
}

static int ctx_ensure_ring(ssctx::Context& c, int n, int n_win, hipStream_t st) {
    hipError_t e;
    if (!c.ev_made) {
        for (int k = 0; k < ssctx::kRing / ssctx::kGroup; ++k) {
            e = hipEventCreateWithFlags(&c.ev_done[k], hipEventDisableTiming);
            if (e != hipSuccess) return hip_err(e);
        }
        e = hipEventCreateWithFlags(&c.ev_pace, hipEventDisableTiming);
        if (e != hipSuccess) return hip_err(e);
        c.ev_made = true;
    }
    if (n > c.ring_cap) {
        e = hipDeviceSynchronize();                            // slots of the old ring may still be read
        if (e != hipSuccess) return hip_err(e);
        int cap = c.ring_cap ? c.ring_cap : 256;
        while (cap < n) cap *= 2;
        if (c.h_desc) (void)hipHostFree(c.h_desc);
        if (c.d_desc) (void)hipFree(c.d_desc);
        c.h_desc = nullptr; c.d_desc = nullptr; c.ring_cap = 0;
        const size_t bytes = sizeof(int) * 8 * static_cast<size_t>(cap) * ssctx::kRing;
        e = hipHostMalloc(reinterpret_cast<void**>(&c.h_desc), bytes, hipHostMallocDefault);
        if (e != hipSuccess) return hip_err(e);
        e = hipMalloc(reinterpret_cast<void**>(&c.d_desc), bytes);
        if (e != hipSuccess) return hip_err(e);
        c.ring_cap = cap;
    }
    if (n_win > c.win_cap) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_err(e);
        int cap = c.win_cap ? c.win_cap : 256;
        while (cap < n_win) cap *= 2;
        if (c.h_win) (void)hipHostFree(c.h_win);
        if (c.d_win) (void)hipFree(c.d_win);
        c.h_win = nullptr; c.d_win = nullptr; c.win_cap = 0;
        const size_t bytes = sizeof(int) * 5 * static_cast<size_t>(cap) * ssctx::kRing;
        e = hipHostMalloc(reinterpret_cast<void**>(&c.h_win), bytes, hipHostMallocDefault);
        if (e != hipSuccess) return hip_err(e);
        e = hipMalloc(reinterpret_cast<void**>(&c.d_win), bytes);
        if (e != hipSuccess) return hip_err(e);
        c.win_cap = cap;
    }
    (void)st;
    return 0;
}

static int ctx_ensure_pool(ssctx::Context& c, hipStream_t st) {
    if (c.pool && c.pool_entries >= c.n_entries) return 0;
    const size_t per_entry = static_cast<size_t>(c.stride) * c.spec_floats * sizeof(float);
    float* np = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&np), per_entry * static_cast<size_t>(c.n_entries));
    if (e != hipSuccess) return hip_err(e);
    if (c.pool) {                                              // grown: keep the spectra already computed
        e = hipMemcpyAsync(np, c.pool, per_entry * static_cast<size_t>(c.pool_entries), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipDeviceSynchronize();       // earlier launches (any stream) still read the old pool
        if (e != hipSuccess) { (void)hipFree(np); return hip_err(e); }
        (void)hipFree(c.pool);
    }
    c.pool = np;
    c.pool_entries = c.n_entries;
    return 0;
}

// What is bound to the context: as the routing sees it (ss_route.hpp) ...
static ssroute::Bank route_bank_of(const ssctx::Context& c) {
    ssroute::Bank b;
    b.rows = c.rir != nullptr;
    b.spectra = c.hspec != nullptr;
    b.half = c.hscale != nullptr;
    b.buckets = !c.buckets.empty();
    b.buckets_spectra = b.buckets && buckets_spectral(c.buckets.data(), static_cast<int>(c.buckets.size()), 0);
    b.spec_buckets = !c.spec_buckets.empty();
    b.spec_buckets_half = b.spec_buckets && c.spec_buckets[0].hscale != nullptr;
    b.spec_buckets_half_rows = b.spec_buckets_half && c.spec_buckets_rows;
    b.rir_cap = c.rir_cap;
    b.h_blocks = c.h_blocks;
    b.rows16 = c.rir16 != nullptr;
    b.rows16_rows = b.rows16 && c.rir16_rows;
    b.rows16_buckets = !c.rir16_buckets.empty();
    return b;
}

// ... and as the launches read it
static Bank bank_of(const ssctx::Context& c) {
    if (!c.spec_buckets.empty()) return spec_buckets_bank(c.spec_buckets.data(), static_cast<int>(c.spec_buckets.size()), c.spec_buckets_rows);
    if (!c.buckets.empty()) return buckets_bank(c.buckets.data(), static_cast<int>(c.buckets.size()));
    if (c.rir16) return rows16_bank(c.rir16, c.rscale, c.rir_cap, c.rir16_rows);
    if (!c.rir16_buckets.empty()) return rir16_buckets_bank(c.rir16_buckets.data(), static_cast<int>(c.rir16_buckets.size()));
    Bank b = rows_bank(c.rir, c.rir_us, c.rir_cs, c.rir_es, c.rir_cap);
    b.hspec = c.hspec; b.hscale = c.hscale; b.h_blocks = c.h_blocks;
    return b;
}

// One step: plan the units (host), compute the missing source-window spectra, render.  `units` are HOST arrays.
// audiogoal / spectrogram are DEVICE buffers [n,2,sr] / [n,65,T4,2]; either may be NULL (not both).
// `lane` >= 0: the step runs on internal stream `lane` of the overlap mode (stream == c.lane_stream[lane])
// `mel` != NULL (then audiogoal == NULL): a log-mel step without a waveform buffer (ss_ctx_observe_features) - the log-mel form
// of the fused kernels where it serves the step, else this step's route into the context's waveform scratch followed by
// ss_audio_features_f32 on the same stream.
static int ctx_observe_on(ss_ctx* h, const ss_units* units, int n, float* audiogoal, float* spectrogram, void* stream,
                          int lane, const ss_features* mel = nullptr) {
    ssctx::Context& c = h->c;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    SS_PROF_BEGIN();
    if (c.plan_only_keys) {                                    // ss_ctx_plan was used on this context: its keys claim
        // spectra that were never computed, and its ticks took no ring slot (the eviction guard of the overlap mode counts
        // ticks as ring slots) - start from an empty cache, and only once nothing in flight reads the pool (a
        // reset under two lanes let lane A's k_source_windows write slots lane B was still reading)
        e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_err(e);
        ssctx::cache_reset(c);
        c.plan_only_keys = false;
    }
    // The window-spectra pool is shared by every step: a step on a NEW stream reads spectra the previous stream wrote
    // (cache hits) and may overwrite slots it still reads (evictions).  One event orders the new stream behind everything
    // the old one has been given so far.
    if (lane >= 0) {
        // overlap mode: the lanes only need each other's WINDOW SPECTRA (a cache hit on lane B of a key lane A computed);
        // evictions cannot touch a slot a step in flight reads (guard of a full ring of ticks, ss_context.hpp)
        for (int o = 0; o < c.n_lanes; ++o) {
            if (o == lane || c.win_seen[lane][o] >= c.win_seq[o]) continue;
            e = hipStreamWaitEvent(st, c.ev_win[o], 0);
            if (e != hipSuccess) return hip_err(e);
            c.win_seen[lane][o] = c.win_seq[o];
        }
    } else if (c.have_last_stream && st != c.last_stream) {
        if (!c.ev_xstream) {
            e = hipEventCreateWithFlags(&c.ev_xstream, hipEventDisableTiming);
            if (e != hipSuccess) return hip_err(e);
        }
        e = hipEventRecord(c.ev_xstream, c.last_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, c.ev_xstream, 0);
        if (e != hipSuccess) return hip_err(e);
    }
    SS_PROF_MARK(1);                                           // cross-lane / cross-stream waits
    int rc = ctx_ensure_ring(c, n, 0, st);
    if (rc) return rc;
    // Ring slots are released in GROUPS: one completion event per kGroup consecutive steps (recorded after the group's
    // last launch, waited for - on the host - before the group's first slot is written again, a full ring later).  An
    // event record per step puts a marker packet between every two launches (measured: 2.6-3 us of a 27-us step).
    // An event exists only for groups whose slots the device read: descriptors read in place by a kernel without a unit
    // table, a descriptor upload, a window upload.  A group of unit-table steps that upload nothing records no event and
    // its next round waits for none (c.ring, ss_ring.hpp: the flag per group says whether its event holds a record of the
    // group's last round - a never-recorded or stale event is not consulted).  A caller that changes streams inside a
    // group closes it on the old stream and starts the next group.
    // Overlap mode (lane >= 0) stays as it was: every lane records its share of every group and every group is waited for.
    if (lane < 0 && c.ring.must_close_before(c.ring_k, st == c.group_stream)) {
        const int og = c.ring.open_group;
        if (c.ring.close_early()) {                            // (also a group a failed step left open)
            e = hipEventRecord(c.ev_done[og], c.group_stream);
            if (e != hipSuccess) return hip_err(e);
        }
        c.ring_k = c.ring.next_slot();
    }
    const int k = c.ring_k, g = k / ssctx::kGroup;
    if (lane < 0) {
        if (c.ring.begin(k)) {
            e = hipEventSynchronize(c.ev_done[g]);             // every launch that read the group's slots has finished
            if (e != hipSuccess) return hip_err(e);
        }
        if (k % ssctx::kGroup == 0) c.group_stream = st;
    } else if (k % ssctx::kGroup == 0) {
        e = hipEventSynchronize(c.ev_done[g]);
        for (int l = 1; l < c.n_lanes && e == hipSuccess; ++l) e = hipEventSynchronize(c.ev_done_l[l][g]);   // ... on every lane
        if (e != hipSuccess) return hip_err(e);
        ++c.ring.n_waits;
    }
    // Small steps: the kernels read the unit descriptors straight from the pinned ring slot (one 32-byte scalar load per
    // workgroup over the host link) - an upload between two launches on the stream costs a blit kernel plus a barrier on
    // either side of it (measured: ~15 us of idle GPU per 25-us step).  Large steps (several descriptors per workgroup,
    // long kernels) keep the upload.
    static const bool force_copy = ab_flag("SS_HIP_DESC_COPY");
    const bool direct = !force_copy && n <= ssctx::kDirectDescUnits;
    int* hd = c.h_desc + static_cast<size_t>(k) * c.ring_cap * 8;
    int* dd = direct ? hd : c.d_desc + static_cast<size_t>(k) * c.ring_cap * 8;
    ssctx::PlanResult res;
    SS_PROF_MARK(2);                                           // ring slot: group event synchronise
    rc = ssctx::plan_units(c, units, n, hd, &res);
    if (rc) return rc;                                         // (refused before the cache or the ring was touched)
    // the step's route, decided once (ss_route.hpp): which launch body, from the rows or the spectra, into whose buffers
    ssroute::Wants wants;
    wants.waveform = audiogoal != nullptr; wants.spectrogram = spectrogram != nullptr; wants.mel = mel != nullptr;
    const ssroute::Route route = ssroute::route_step(route_bank_of(c), c.out_len, c.n_valid, c.policy, n, res.flags, wants, route_switches());
    // a spectral-only bank cannot serve a step whose route reads the time-domain rows (a cross-fade): refused before any upload
    // or launch, the plan's keys given back
    if (route.refused) {
        ssctx::cache_rollback(c);
        return SS_EINVAL;
    }
    SS_PROF_MARK(3);                                           // planner
    c.ring_k = (k + 1) % ssctx::kRing;                         // the slot is taken from here on, whatever happens next
    // The slot's group is released by an event recorded behind the group's last launch (overlap mode: behind each lane's
    // last launch of the group); a step that fails after this point must still record it, or the group's next round
    // would be checked against a stale event.
    bool slot_read = true;                                     // until the launch has reported the unit-table route
    auto close_slot = [&]() -> int {
        hipError_t ee = hipSuccess;
        if (lane >= 0) {
            if (k % ssctx::kGroup >= ssctx::kGroup - c.n_lanes) {
                ee = hipEventRecord(lane == 0 ? c.ev_done[g] : c.ev_done_l[lane][g], st);
                ++c.ring.n_records;
            }
        } else if (c.ring.end(k, slot_read)) {
            ee = hipEventRecord(c.ev_done[g], st);
            c.pace.ring_event();
        } else {
            // no ring event behind this step: the host's run-ahead is bounded by the pace event instead (ss_ring.hpp), one record
            // per kRing such steps, waited for one period later
            bool wait_first = false;
            if (c.pace.step(&wait_first)) {
                if (wait_first) ee = hipEventSynchronize(c.ev_pace);
                if (ee == hipSuccess) ee = hipEventRecord(c.ev_pace, st);
            }
        }
        return hip_err(ee);
    };
    // ... and take the keys of this plan out of the cache again as long as their spectra have not been computed
    auto fail = [&](int code) { ssctx::cache_rollback(c); (void)close_slot(); return code; };
    rc = ctx_ensure_pool(c, st);
    if (rc) return fail(rc);
    if (res.n_new_windows > 0) {
        rc = ctx_ensure_ring(c, n, res.n_new_windows, st);
        if (rc) return fail(rc);
        int* hw = c.h_win + static_cast<size_t>(k) * c.win_cap * 5;
        int* dw = c.d_win + static_cast<size_t>(k) * c.win_cap * 5;
        std::memcpy(hw, c.new_win.data(), sizeof(int) * 5 * static_cast<size_t>(res.n_new_windows));
        e = hipMemcpyAsync(dw, hw, sizeof(int) * 5 * static_cast<size_t>(res.n_new_windows), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(hip_err(e));
        rc = launch_windows_scatter(c.src_dev, dw, c.pool, res.n_new_windows, st);
        if (rc) return fail(rc);
        if (lane >= 0) {                                       // the other lane's next step may hit these keys
            e = hipEventRecord(c.ev_win[lane], st);
            if (e != hipSuccess) return fail(hip_err(e));
            ++c.win_seq[lane];
        }
    }
    c.new_entries.clear();                                     // their spectra are on the stream: the keys are good
    c.last_stream = st;
    c.have_last_stream = true;
    if (!direct) {
        e = hipMemcpyAsync(dd, hd, sizeof(int) * 8 * static_cast<size_t>(n), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(hip_err(e));
    }
    // log-mel without a waveform buffer, on the shapes no log-mel form serves: the step renders into the context's own waveform
    // scratch and the feature kernel runs over it
    if (route.wave_scratch) {
        rc = get_wave_scratch(&c, lane < 0 ? 0 : lane, st, static_cast<size_t>(n) * 2 * c.out_len, &audiogoal);
        if (rc) return fail(rc);
    }
    if (route.handover) {                                      // cross-faded / very long rows hand over through memory (the context's own buffer)
        const size_t need = static_cast<size_t>(n) * 2 * c.out_len;
        if (need > c.ag_cap) {
            e = hipDeviceSynchronize();
            if (e != hipSuccess) return fail(hip_err(e));
            if (c.ag_scratch) (void)hipFree(c.ag_scratch);
            c.ag_scratch = nullptr; c.ag_cap = 0;
            e = hipMalloc(reinterpret_cast<void**>(&c.ag_scratch), need * sizeof(float));
            if (e != hipSuccess) return fail(hip_err(e));
            c.ag_cap = need;
        }
        audiogoal = c.ag_scratch;
    }
    static const bool no_tab = ab_flag("SS_HIP_NO_UNIT_TAB");
    SS_PROF_MARK(4);                                           // new windows (upload + k_source_windows), descriptor upload
    bool tab_taken = false;
    LaunchEnv env;
    env.st = st;
    env.host_desc = no_tab ? nullptr : hd;                     // (see fill_unit_tab)
    env.share = c.chip_share > 0 ? c.chip_share : c.n_lanes;
    env.tab_taken = &tab_taken;
    ssk::MelArgs m{};
    if (mel) m = ssk::MelArgs{mel->logmel, mel->mel_start, mel->mel_w, mel->n_mels, mel->max_len, mel->mel_eps};
    rc = render(bank_of(c), route.spectral, route.launch, c.pool, c.rir_len, dd, audiogoal, spectrogram,
                mel && !route.wave_scratch ? &m : nullptr, n, c.n_valid, c.out_len, c.pad_mode, res.flags, env);
    // what the device may read from this step's ring slot after the call: descriptors in place (no unit table), the source of
    // their upload, the source of the window upload
    slot_read = !direct || res.n_new_windows > 0 || !tab_taken;
    SS_PROF_MARK(5);                                           // the launch entry (unit table + hipLaunchKernel)
    if (!rc && route.wave_scratch)                             // scratch route: the features of the waveform just rendered
        rc = ss_audio_features_f32(audiogoal, n, c.out_len, c.pad_mode, nullptr, mel->logmel, mel->mel_start, mel->mel_w,
                                   mel->n_mels, mel->max_len, mel->mel_eps, nullptr, 1, 1.f, stream);
    if (rc) return fail(rc);
    // (overlap mode: a group's ticks alternate between the lanes; each lane records its half after ITS last tick)
    rc = close_slot();
    SS_PROF_MARK(6);                                           // group event record
    return rc;
}

// ---- overlap mode -------------------------------------------------------------------------------------------------
int ss_ctx_set_overlap(ss_ctx* h, int n_streams) {
    if (!h || n_streams < 1 || n_streams > ssctx::kLanes) return SS_EINVAL;
    ssctx::Context& c = h->c;
    hipError_t e = hipDeviceSynchronize();                     // a clean cut between the two regimes
    if (e != hipSuccess) return hip_err(e);
    if (n_streams > 1 && !c.lanes_made) {
        for (int l = 0; l < ssctx::kLanes; ++l) {
            e = hipStreamCreateWithFlags(&c.lane_stream[l], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c.ev_lane[l], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c.ev_win[l], hipEventDisableTiming);
            if (e != hipSuccess) return hip_err(e);
        }
        e = hipEventCreateWithFlags(&c.ev_in, hipEventDisableTiming);
        if (e != hipSuccess) return hip_err(e);
        for (int k = 0; k < ssctx::kRing / ssctx::kGroup; ++k) {
            for (int l = 1; l < ssctx::kLanes; ++l) {
                e = hipEventCreateWithFlags(&c.ev_done_l[l][k], hipEventDisableTiming);
                if (e != hipSuccess) return hip_err(e);
            }
        }
        c.lanes_made = true;
    }
    c.n_lanes = n_streams;
    c.lane_next = 0;
    c.ring_k = 0;                                              // groups start afresh (everything has completed)
    c.ring.reset();
    c.pace.reset();
    c.have_last_stream = false;
    for (int l = 0; l < ssctx::kLanes; ++l) { c.lane_dirty[l] = false; c.lane_joined[l] = false; c.lane_join_valid[l] = false; for (int o = 0; o < ssctx::kLanes; ++o) c.win_seen[l][o] = c.win_seq[o]; }
    return 0;
}

int ss_ctx_set_spectral_policy(ss_ctx* h, int max_units) {
    if (!h || max_units < 0) return SS_EINVAL;
    h->c.policy.spectral_max_units = max_units;
    return 0;
}

int ss_ctx_set_logmel_policy(ss_ctx* h, int min_units, int max_units) {
    if (!h || min_units < 0 || max_units < 0) return SS_EINVAL;
    h->c.policy.mel_fused_min = min_units;
    h->c.policy.mel_fused_max = max_units;
    return 0;
}

int ss_ctx_set_logmel_rows_policy(ss_ctx* h, int min_units, int max_units) {
    if (!h || min_units < 0 || max_units < 0) return SS_EINVAL;
    h->c.policy.mel_rows_min = min_units;
    h->c.policy.mel_rows_max = max_units;
    return 0;
}

int ss_ctx_set_logmel_ss2_policy(ss_ctx* h, int min_units, int max_units) {
    if (!h || min_units < 0 || max_units < 0) return SS_EINVAL;
    h->c.policy.mel_ss2_min = min_units;
    h->c.policy.mel_ss2_max = max_units;
    return 0;
}

int ss_ctx_set_logmel_buckets_policy(ss_ctx* h, int min_units, int max_units) {
    if (!h || min_units < 0 || max_units < 0) return SS_EINVAL;
    h->c.policy.mel_bk_min = min_units;
    h->c.policy.mel_bk_max = max_units;
    return 0;
}

int ss_ctx_set_logmel_rir16_policy(ss_ctx* h, int min_units, int max_units) {
    if (!h || min_units < 0 || max_units < 0) return SS_EINVAL;
    h->c.policy.mel_r16_min = min_units;
    h->c.policy.mel_r16_max = max_units;
    return 0;
}

size_t ss_ctx_wave_scratch_bytes(const ss_ctx* h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    size_t bytes = 0;
    for (const auto& kv : g_wave_scratch)
        if (kv.first.first == &h->c && kv.second.ptr) bytes += kv.second.floats * sizeof(float);
    return bytes;
}

int ss_ctx_set_chip_share(ss_ctx* h, int n_sources) {
    if (!h || n_sources < 0 || n_sources > 8) return SS_EINVAL;
    h->c.chip_share = n_sources;
    return 0;
}

int ss_ctx_join(ss_ctx* h, void* stream) {
    if (!h) return SS_EINVAL;
    ssctx::Context& c = h->c;
    if (c.n_lanes <= 1) return 0;                              // single-stream mode: the caller's stream IS the work's stream
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int l = 0; l < c.n_lanes; ++l) {
        // a lane with nothing issued since its last join: its event still stands for "everything on the lane" - a join from
        // ANOTHER stream waits for that record, the stream that joined last has nothing left to wait for
        if (!c.lane_dirty[l] && (!c.lane_joined[l] || (c.lane_join_valid[l] && c.lane_join_stream[l] == st))) continue;
        hipError_t e = c.lane_dirty[l] ? hipEventRecord(c.ev_lane[l], c.lane_stream[l]) : hipSuccess;
        if (e == hipSuccess) e = hipStreamWaitEvent(st, c.ev_lane[l], 0);
        if (e != hipSuccess) return hip_err(e);
        c.lane_dirty[l] = false;
        c.lane_joined[l] = true;
        c.lane_join_valid[l] = true;
        c.lane_join_stream[l] = st;
    }
    return 0;
}

// Overlap mode: work on `st` that REWRITES bank rows (the in-call loaders' scatter) goes behind every step issued so far - steps
// in flight on the lanes may still read the entries (write after read).  The lanes' join state is left alone.
static int order_behind_lanes(ssctx::Context& c, hipStream_t st) {
    if (c.n_lanes <= 1) return 0;
    for (int l = 0; l < c.n_lanes; ++l) {
        if (!c.lane_dirty[l] && !c.lane_joined[l]) continue;
        hipError_t e = c.lane_dirty[l] ? hipEventRecord(c.ev_lane[l], c.lane_stream[l]) : hipSuccess;
        if (e == hipSuccess) e = hipStreamWaitEvent(st, c.ev_lane[l], 0);
        if (e != hipSuccess) return hip_err(e);
        if (c.lane_dirty[l]) {                                 // the record now covers the lane's work: a later join re-uses it
            c.lane_dirty[l] = false;
            c.lane_joined[l] = true;
            c.lane_join_valid[l] = false;                      // (no stream has JOINED: every join still waits)
        }
    }
    return 0;
}

static int ctx_features_on(ss_ctx* h, int n, const float* audiogoal, float* spectrogram, const ss_features* f, void* stream) {
    if (!f) return 0;
    const ssctx::Context& c = h->c;
    return ss_audio_features_f32(audiogoal, n, c.out_len, c.pad_mode, spectrogram, f->logmel, f->mel_start, f->mel_w, f->n_mels,
                                 f->max_len, f->mel_eps, f->gccphat, f->max_lag, f->gcc_eps, stream);
}

// A step with extension features: k_features has every frame's spectrum of both ears in registers anyway, so the pooled
// spectrogram comes from IT (+4.7 us per 256 units) and the convolution launch drops its fused STFT phase (-7 us per round of
// 256 rows): the waveform is the hand-over either way (the features need it in memory).
static bool features_take_spectrogram(const ss_features* f, const float* audiogoal, const float* spectrogram) {
    static const bool off = ab_flag("SS_HIP_FEAT_KEEP_FUSED");       // (A/B builds only)
    return !off && f && audiogoal && spectrogram;
}

static int ctx_observe_any(ss_ctx* h, const ss_units* units, int n, float* audiogoal, float* spectrogram, const ss_features* f,
                           void* stream) {
    if (!h || n < 0 || (!audiogoal && !spectrogram && !(f && f->logmel))) return SS_EINVAL;
    if (f && !f->logmel && !f->gccphat) return SS_EINVAL;
    // without a waveform buffer: log-mel (and the pooled spectrogram) only - GCC-PHAT reads both ears' waveform
    const bool mel_only = f && !audiogoal;
    if (mel_only && (f->gccphat || !mel_args_ok(f->logmel, f->mel_start, f->mel_w, f->n_mels, f->max_len, f->mel_eps)))
        return SS_EINVAL;
    if (n == 0) return 0;
    ssctx::Context& c = h->c;
    if ((!c.rir && !c.hspec && !c.rir16 && c.rir16_buckets.empty() && c.buckets.empty() && c.spec_buckets.empty()) || !c.rir_len || !c.src_dev) return SS_EINVAL;
    const bool sg_late = features_take_spectrogram(f, audiogoal, spectrogram);
    if (c.n_lanes <= 1) {
        if (mel_only) return ctx_observe_on(h, units, n, nullptr, spectrogram, stream, -1, f);
        const int rc = ctx_observe_on(h, units, n, audiogoal, sg_late ? nullptr : spectrogram, stream, -1);
        return rc ? rc : ctx_features_on(h, n, audiogoal, sg_late ? spectrogram : nullptr, f, stream);
    }
    // overlap mode: this step goes to the next internal stream, behind whatever the caller's stream holds right now (the
    // consumers of the output rows it overwrites, uploads of RIR rows it reads); the caller's stream sees the result after
    // ss_ctx_join.  Consecutive steps run on different streams: the head of step k+1 (descriptor + row loads, HBM latency,
    // nothing to compute) overlaps the tail of step k (STFT, no memory traffic).
    const int lane = c.ring_k % c.n_lanes;                     // tick parity: a refused call does not shift the lanes
    SS_PROF_BEGIN();
    // The fence costs an event record + a stream wait (measured: 4.6 us of the call's 10.8 us of host time at 16-32 envs, where
    // the host IS the step's bound) and a barrier packet in front of the lane's launch.  A caller's stream that has nothing
    // pending - a trainer that has just read its actions back, a vector env between two policy steps - needs none.
    static const bool always_fence = ab_flag("SS_HIP_ALWAYS_FENCE");        // (A/B builds only)
    //  a stream being captured into a graph must not be QUERIED - that is an illegal operation which invalidates
    // the capture: ask the capture status first and go straight to the fence in that case.  Single-threaded use of `stream` is
    // assumed between the query and the lane's launch (include/ss_hip.h, ss_ctx_set_overlap).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (!always_fence && hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusActive;                    // cannot tell: do not query, fence
    }
    hipError_t e = (always_fence || cap != hipStreamCaptureStatusNone) ? hipErrorNotReady
                                                                       : hipStreamQuery(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        // work pending (hipErrorNotReady: the only answer that is cleared here - a genuine sticky error stays for the fence's
        // own calls and the launch check to report): order the lane behind the caller's stream
        if (!always_fence && cap == hipStreamCaptureStatusNone && e == hipErrorNotReady) (void)hipGetLastError();
        e = hipEventRecord(c.ev_in, static_cast<hipStream_t>(stream));
        if (e == hipSuccess) e = hipStreamWaitEvent(c.lane_stream[lane], c.ev_in, 0);
    }
    if (e != hipSuccess) return hip_err(e);
    SS_PROF_MARK(0);                                           // input fence: caller's stream -> lane
    SS_PROF_CALL();
    c.lane_dirty[lane] = true;
    if (mel_only) return ctx_observe_on(h, units, n, nullptr, spectrogram, c.lane_stream[lane], lane, f);
    const int rc = ctx_observe_on(h, units, n, audiogoal, sg_late ? nullptr : spectrogram, c.lane_stream[lane], lane);
    return rc ? rc : ctx_features_on(h, n, audiogoal, sg_late ? spectrogram : nullptr, f, c.lane_stream[lane]);
}

#if defined(SS_AB)
int ss_ab_host_profile(double* ns_out8, long long* calls_out) {
    for (int i = 0; i < 8; ++i) { ns_out8[i] = g_prof_ns[i]; g_prof_ns[i] = 0; }
    *calls_out = g_prof_calls; g_prof_calls = 0;
    return 0;
}
#endif

int ss_ctx_observe(ss_ctx* h, const ss_units* units, int n, float* audiogoal, float* spectrogram, void* stream) {
    return ctx_observe_any(h, units, n, audiogoal, spectrogram, nullptr, stream);
}

int ss_ctx_observe_features(ss_ctx* h, const ss_units* units, int n, float* audiogoal, float* spectrogram, const ss_features* f,
                            void* stream) {
    if (!f) return SS_EINVAL;
    return ctx_observe_any(h, units, n, audiogoal, spectrogram, f, stream);
}


}  // extern "C"
// hold (pose memo): envs served from the memo this step - silent units, no RIR looked up, never a miss; advance = false: leave
// audio_index alone (sims_advance does pass 2 once the step is certain to go ahead)
static int sims_to_units(ss_ctx* h, const ss_sim_columns* sc, int n, int* w, int* miss_out, int* n_miss,
                         const unsigned char* hold = nullptr, bool advance = true);
static void sims_advance(ss_ctx* h, const ss_sim_columns* sc, int n, const int* w);
extern "C" {

// One step from the simulators' state columns (see include/ss_hip.h): the per-step numpy of ss_amd/vector.py in C++.
int ss_ctx_sims_units(ss_ctx* h, const ss_sim_columns* sc, int n, int* units_out, int* miss_out, int* n_miss) {
    if (!units_out) return SS_EINVAL;
    return sims_to_units(h, sc, n, units_out, miss_out, n_miss);
}

int ss_ctx_observe_sims(ss_ctx* h, const ss_sim_columns* sc, int n, float* audiogoal, float* spectrogram, int* miss_out,
                        int* n_miss, void* stream) {
    if (!h || n < 0) return SS_EINVAL;
    std::vector<int>& w = h->c.sim_scratch;
    w.resize(static_cast<size_t>(n) * 5 + 1);
    const int rc = sims_to_units(h, sc, n, w.data(), miss_out, n_miss);
    if (rc != 0 || n == 0 || *n_miss) return rc;
    ss_units u;
    std::memset(&u, 0, sizeof u);
    u.sound = w.data(); u.t0 = u.sound + n; u.rir = u.t0 + n;
    if (sc->dis_sound) { u.dis_sound = u.rir + n; u.dis_rir = u.dis_sound + n; }
    return ss_ctx_observe(h, &u, n, audiogoal, spectrogram, stream);
}

// ---- pose memo on the column path (ss_memo.hpp) ---------------------------------------------------------------------
int ss_ctx_memo_enable(ss_ctx* h, int n_envs) {
    if (!h || n_envs < 0) return SS_EINVAL;
    ssctx::Context& c = h->c;
    c.memo.reset(n_envs);
    c.memo_on = n_envs > 0;
    c.memo_outputs = 0;
    if (!c.memo_on) { c.memo = ssmemo::Memo(); std::vector<int>().swap(c.memo_moves); }
    return 0;
}

int ss_ctx_memo_reset(ss_ctx* h) {
    if (!h || !h->c.memo_on) return SS_EINVAL;
    h->c.memo.clear();
    h->c.memo_outputs = 0;
    return 0;
}

int ss_ctx_memo_stats(ss_ctx* h, long long* out4) {
    if (!h || !out4 || !h->c.memo_on) return SS_EINVAL;
    const ssmemo::Memo& m = h->c.memo;
    out4[0] = m.hits; out4[1] = m.misses; out4[2] = m.in_use; out4[3] = m.dropped;
    return 0;
}

}  // extern "C"

// The host half of a memo step up to the point of no return: memo plan (who is held), unit columns with the hold mask, RIR
// misses.  Changes nothing.  *need_rows / *n_miss say whether the step may go ahead.
static int memo_plan_step(ss_ctx* h, const ss_sim_columns* sc, int n, int pool_rows, int* w, int* miss_out, int* n_miss,
                          int* need_rows) {
    if (!h || !sc || !n_miss || !need_rows || !h->c.memo_on || n != h->c.memo.n_envs() || pool_rows < 0 || sc->dis_sound ||
        sc->dis_src)
        return SS_EINVAL;
    ssmemo::Memo& m = h->c.memo;
    *n_miss = 0; *need_rows = 0;
    const int need = m.plan(sc->scene, sc->sound, sc->src, sc->recv, sc->rot, n, pool_rows);
    if (need < 0) return SS_EINVAL;
    const int rc = sims_to_units(h, sc, n, w, miss_out, n_miss, m.hold.data(), false);
    if (rc) return rc;
    *need_rows = need;
    return 0;
}

// ... and past it: audio_index advances for the envs that were rendered, the memo takes the step's entries.  -> moves
static void memo_commit_step(ss_ctx* h, const ss_sim_columns* sc, int n, const int* w, int* moves, int* n_store, int* n_fetch) {
    sims_advance(h, sc, n, w);
    h->c.memo.commit(sc->scene, sc->sound, moves, n_store, n_fetch);
}

extern "C" {

int ss_ctx_sims_memo_plan(ss_ctx* h, const ss_sim_columns* sc, int n, int pool_rows, int* units_out, unsigned char* hold_out,
                          int* moves_out, int* n_store, int* n_fetch, int* miss_out, int* n_miss, int* need_rows) {
    if (!units_out || !hold_out || !moves_out || !n_store || !n_fetch) return SS_EINVAL;
    const int rc = memo_plan_step(h, sc, n, pool_rows, units_out, miss_out, n_miss, need_rows);
    if (rc) return rc;
    *n_store = *n_fetch = 0;
    std::memcpy(hold_out, h->c.memo.hold.data(), static_cast<size_t>(n));
    if (*n_miss || *need_rows) return 0;
    memo_commit_step(h, sc, n, units_out, moves_out, n_store, n_fetch);
    return 0;
}

int ss_ctx_observe_sims_memo(ss_ctx* h, const ss_sim_columns* sc, int n, float* audiogoal, float* spectrogram,
                             const ss_memo_pool* pool, int* miss_out, int* n_miss, int* need_rows, void* stream) {
    if (!h || !pool || pool->rows < 0 || (!audiogoal && !spectrogram) || !audiogoal != !pool->audiogoal ||
        !spectrogram != !pool->spectrogram)
        return SS_EINVAL;
    ssctx::Context& c = h->c;
    const int outputs = (audiogoal ? 1 : 0) | (spectrogram ? 2 : 0);
    if (c.memo_on && c.memo_outputs && outputs != c.memo_outputs) return SS_EINVAL;
    ss_memo_io io[2];
    int n_io = 0;
    const int t4 = t4_of(c.out_len);
    if (spectrogram) io[n_io++] = ss_memo_io{spectrogram, pool->spectrogram, ssk::kBins4 * t4 * 2, 0};
    if (audiogoal) io[n_io++] = ss_memo_io{audiogoal, pool->audiogoal, 2 * c.out_len, 0};
    if (!memo_io_ok(io, n_io)) return SS_EINVAL;
    std::vector<int>& w = c.sim_scratch;
    w.resize(static_cast<size_t>(n < 0 ? 0 : n) * 5 + 1);
    int rc = memo_plan_step(h, sc, n, pool->rows, w.data(), miss_out, n_miss, need_rows);
    if (rc != 0 || *n_miss || *need_rows) return rc;                      // refused or reported: nothing launched, nothing committed
    ss_units u;
    std::memset(&u, 0, sizeof u);
    u.sound = w.data(); u.t0 = u.sound + n; u.rir = u.t0 + n;
    rc = ss_ctx_observe(h, &u, n, audiogoal, spectrogram, stream);       // held envs are silent units
    if (rc) return rc;                                                    // (a step that failed commits nothing either)
    c.memo_moves.resize(static_cast<size_t>(n) * 2);
    int n_store = 0, n_fetch = 0;
    memo_commit_step(h, sc, n, w.data(), c.memo_moves.data(), &n_store, &n_fetch);
    c.memo_outputs = outputs;
    // the row copies go right behind the step's launches, on the stream that carries them: the caller's, or in overlap mode the
    // lane the step was given - there behind the other lanes' latest copies as well (the pools are shared by the lanes; the
    // renders stay unordered), which takes stream waits, no join and no host wait.  The moves travel in the kernel arguments:
    // nothing of the step's ring slot is read.
    hipStream_t st = c.n_lanes > 1 ? c.last_stream : static_cast<hipStream_t>(stream);
    int lane = -1;
    for (int l = 0; l < c.n_lanes && c.n_lanes > 1; ++l)
        if (c.lane_stream[l] == st) lane = l;
    hipError_t e = hipSuccess;
    if (lane >= 0) {
        if (!c.memo_ev_made) {
            for (int l = 0; l < ssctx::kLanes && e == hipSuccess; ++l) e = hipEventCreateWithFlags(&c.ev_memo[l], hipEventDisableTiming);
            if (e != hipSuccess) return hip_err(e);
            c.memo_ev_made = true;
        }
        for (int o = 0; o < ssctx::kLanes; ++o) {
            if (o == lane || c.memo_seen[lane][o] >= c.memo_seq[o]) continue;
            e = hipStreamWaitEvent(st, c.ev_memo[o], 0);
            if (e != hipSuccess) return hip_err(e);
            c.memo_seen[lane][o] = c.memo_seq[o];
        }
    }
    rc = launch_memo_rows(io, n_io, c.memo_moves.data(), true, n_store, n_fetch, st);
    if (rc) return rc;
    if (lane >= 0) {
        e = hipEventRecord(c.ev_memo[lane], st);
        if (e != hipSuccess) return hip_err(e);
        ++c.memo_seq[lane];
    }
    return 0;
}

}  // extern "C"

static int sims_to_units(ss_ctx* h, const ss_sim_columns* sc, int n, int* w, int* miss_out, int* n_miss,
                         const unsigned char* hold, bool advance) {
    if (!h || !sc || n < 0 || !n_miss || !sc->sound || !sc->audio_index || !sc->step_count || !sc->duration || !sc->recv ||
        !sc->src || !sc->rot || !sc->scene || !sc->index_flat || !sc->index_off || !sc->index_dim || sc->azimuths < 1 ||
        360 % sc->azimuths || (!sc->dis_sound != !sc->dis_src))
        return SS_EINVAL;
    ssctx::Context& c = h->c;
    *n_miss = 0;
    if (n == 0) return 0;
    const bool dis = sc->dis_sound != nullptr;
    const int n_src = static_cast<int>(c.src_len.size()), step = 360 / sc->azimuths;
    int* sound = w; int* t0 = sound + n; int* rir = t0 + n; int* dsound = rir + n; int* drir = dsound + n;
    auto lookup = [&](int i, long long node_src) -> int {
        const long long scn = sc->scene[i];
        if (scn < 0 || scn >= sc->n_scenes) return -1;
        const long long dim = sc->index_dim[scn], r = sc->recv[i];
        if (r < 0 || r >= dim || node_src < 0 || node_src >= dim) return -1;
        const int base = sc->index_flat[sc->index_off[scn] + r * dim + node_src];
        if (base < 0) return -1;
        long long az = (-sc->rot[i]) % 360;
        if (az < 0) az += 360;
        return base + static_cast<int>(az / step);
    };
    int misses = 0;
    for (int i = 0; i < n; ++i) {                              // pass 1: everything except the audio_index advance
        const long long s = sc->sound[i];
        const bool silent = s < 0 || s >= n_src || sc->step_count[i] > sc->duration[i] || (hold && hold[i]);
        sound[i] = silent ? 0 : static_cast<int>(s);
        dsound[i] = 0; drir[i] = -1;
        if (silent) { rir[i] = -1; t0[i] = 0; continue; }
        const int len = c.src_len[sound[i]];
        t0[i] = len == c.sr ? 0 : static_cast<int>(sc->audio_index[i]) * c.sr;
        rir[i] = lookup(i, sc->src[i]);
        bool miss = rir[i] < 0;
        if (dis) {
            const long long ds = sc->dis_sound[i];
            if (ds >= 0 && ds < n_src) {
                dsound[i] = static_cast<int>(ds);
                drir[i] = lookup(i, sc->dis_src[i]);
                miss = miss || drir[i] < 0;
            }
        }
        if (miss && miss_out && misses < n) miss_out[misses] = i;
        misses += miss;
    }
    if (misses) { *n_miss = misses; return 0; }
    if (advance) sims_advance(h, sc, n, w);
    return 0;
}

static void sims_advance(ss_ctx* h, const ss_sim_columns* sc, int n, const int* w) {
    const ssctx::Context& c = h->c;
    const int* sound = w; const int* rir = w + 2 * static_cast<size_t>(n);
    for (int i = 0; i < n; ++i) {                              // pass 2: simulator.py:634-635
        if (rir[i] < 0) continue;
        const int len = c.src_len[sound[i]];
        if (len != c.sr && len >= c.sr) sc->audio_index[i] = (sc->audio_index[i] + 1) % (len / c.sr);
    }
}

// ---- request records of a multi-process vector env (ss_amd/deferred.py) -> unit columns ------------------------------
static long long find_key(const long long* keys, const long long* vals, int n, long long q) {
    if (!keys || n <= 0) return -1;
    const long long* p = std::lower_bound(keys, keys + n, q);
    return (p != keys + n && *p == q) ? vals[p - keys] : -1;
}

static int requests_to_units(ss_ctx* h, const long long* recs, int n, const ss_request_tables* tb, int* w, int* miss_out,
                             int* n_miss) {
    if (!h || !recs || !tb || n < 0 || !n_miss || tb->n_sounds < 0 || tb->n_tables < 0 || tb->n_pairs < 0) return SS_EINVAL;
    ssctx::Context& c = h->c;
    *n_miss = 0;
    const int n_src = static_cast<int>(c.src_len.size());
    int* sound = w; int* t0 = sound + n; int* rir = t0 + n; int* dsound = rir + n; int* drir = dsound + n;
    int misses = 0;
    auto slot_of = [&](long long table, long long recv, long long src) -> int {
        if (recv < 0 || src < 0 || recv >= (1 << 20) || src >= (1 << 20)) return -1;
        const long long s = find_key(tb->pair_keys, tb->pair_slots, tb->n_pairs, (table << 40) | (recv << 20) | src);
        if (s < 0 || (tb->stale && s < tb->n_slots && tb->stale[s])) return -1;
        if (tb->last_used && s < tb->n_slots) tb->last_used[s] = tb->tick;      // the caller's LRU clock
        return static_cast<int>(s);
    };
    for (int i = 0; i < n; ++i) {
        const long long* r = recs + static_cast<size_t>(i) * SS_REQ_WORDS;
        sound[i] = 0; t0[i] = 0; rir[i] = -1; dsound[i] = 0; drir[i] = -1;
        if (r[0] != 0) continue;                               // silent (simulator.py:610-612)
        const long long sid = find_key(tb->sound_keys, tb->sound_ids, tb->n_sounds, r[1]);
        const long long tid = find_key(tb->table_keys, tb->table_ids, tb->n_tables, r[3]);
        bool miss = sid < 0 || sid >= n_src || tid < 0 || r[2] < 0 || r[2] > 0x7fffffffLL;
        if (!miss) {
            sound[i] = static_cast<int>(sid);
            t0[i] = static_cast<int>(r[2]);
            rir[i] = slot_of(tid, r[4], r[5]);
            miss = rir[i] < 0;
            if (r[6] >= 0) {                                   // distractor (simulator.py:649-664): whole clip, own RIR
                const long long did = find_key(tb->sound_keys, tb->sound_ids, tb->n_sounds, r[6]);
                if (did < 0 || did >= n_src) miss = true;
                else {
                    dsound[i] = static_cast<int>(did);
                    drir[i] = slot_of(tid, r[4], r[7]);
                    miss = miss || drir[i] < 0;
                }
            }
        }
        if (miss && miss_out && misses < n) miss_out[misses] = i;
        misses += miss;
    }
    *n_miss = misses;
    return 0;
}

extern "C" {

int ss_ctx_requests_units(ss_ctx* h, const long long* recs, int n, const ss_request_tables* tb, int* units_out, int* miss_out,
                          int* n_miss) {
    if (!units_out) return SS_EINVAL;
    return requests_to_units(h, recs, n, tb, units_out, miss_out, n_miss);
}

int ss_ctx_observe_requests(ss_ctx* h, const long long* recs, int n, const ss_request_tables* tb, float* audiogoal,
                            float* spectrogram, int* miss_out, int* n_miss, void* stream) {
    if (!h || n < 0) return SS_EINVAL;
    std::vector<int>& w = h->c.sim_scratch;
    w.resize(static_cast<size_t>(n) * 5 + 1);
    const int rc = requests_to_units(h, recs, n, tb, w.data(), miss_out, n_miss);
    if (rc != 0 || n == 0 || *n_miss) return rc;
    ss_units u;
    std::memset(&u, 0, sizeof u);
    u.sound = w.data(); u.t0 = u.sound + n; u.rir = u.t0 + n;
    bool any_dis = false;
    for (int i = 0; i < n && !any_dis; ++i) any_dis = u.rir[n + n + i] >= 0;     // dis_rir column
    if (any_dis) { u.dis_sound = u.rir + n; u.dis_rir = u.dis_sound + n; }
    return ss_ctx_observe(h, &u, n, audiogoal, spectrogram, stream);
}

// k files -> k bank entries of the lent store (ss_miss_loader): entries off the free stack, then - with the recency arrays lent -
// the least recently used occupied ones (never one stamped with `tick`); files read into the pinned block, ONE scatter launch,
// the new rows' block spectra when `spectral`; loaded_slot / loaded_frames / evicted_slot report.  1 = not served, nothing changed.
// A third bank kind beside "rows" and "spectral-only": half-precision time-domain rows in ONE allocation (ss_ctx_set_rir_bank16 /
// _rows).  Served when the loader lends no rows (bank == NULL), a pinned block for the rows' maxima (stage_max) and the bound
// capacity; never spectral.  Same books; the one launch is k_scatter_rows16_max on the context's halves and scales.
static bool loader_rows16(const ssctx::Context& c, const ss_miss_loader* ld) {
    return c.rir16 && c.rscale && ld && !ld->bank && ld->stage_max && ld->cap == c.rir_cap;
}

static int loader_load_paths(ssctx::Context& c, ss_miss_loader* ld, const char* const* cp, int k, long long* last_used, long long tick,
                             int n_slots, bool spectral, hipStream_t st) {
    const int hb = (ld->cap + ssk::kB - 1) / ssk::kB;
    if (k <= 0 || k > ld->stage_rows || k > ld->loaded_cap) return 1;
    // a spectral-only bank (no rows: ld->bank == NULL) takes its block spectra straight from the staged rows (k_stage_spectra)
    const bool rows16 = loader_rows16(c, ld);
    if (rows16 && spectral) return 1;
    const bool spec_only = !ld->bank && !rows16;
    if (spec_only && (!spectral || c.rir)) return 1;
    if (spectral && ((!spec_only && !ld->stage_desc) || c.h_blocks != hb || !c.hspec)) return 1;
    // entries: free ones first, then - if the caller lent its recency arrays - the least recently used occupied ones
    std::vector<int> victims;
    if (k > ld->n_free) {
        const int r = k - ld->n_free;
        if (!ld->used || !ld->use_seq || !ld->evicted_slot || !last_used || r > ld->evict_cap) return 1;
        std::vector<int> cand;
        for (int sl = 0; sl < n_slots; ++sl)
            if (ld->used[sl] && last_used[sl] < tick) cand.push_back(sl);     // (never a row this step resolves to)
        if (static_cast<int>(cand.size()) < r) return 1;       // the caller's own path raises its "store too small" there
        auto older = [&](int a, int b) {
            return last_used[a] != last_used[b] ? last_used[a] < last_used[b] : ld->use_seq[a] < ld->use_seq[b];
        };
        std::partial_sort(cand.begin(), cand.begin() + r, cand.end(), older);
        victims.assign(cand.begin(), cand.begin() + r);
    }
    std::vector<int> take(k);                                  // the entries the k new rows go to, in order
    for (int i = 0; i < k; ++i)
        take[i] = i < ld->n_free ? ld->free_slots[ld->n_free - 1 - i] : victims[i - ld->n_free];
    if (spectral && !spec_only) {                              // (window offsets are int32 words from the bank's base)
        for (int i = 0; i < k; ++i)
            if ((static_cast<long long>(take[i]) + 1) * ld->bank_unit_stride >= (1LL << 31)) return 1;
    }
    if (c.miss_ev) {                                           // the staging block's previous scatter has run
        if (hipEventSynchronize(static_cast<hipEvent_t>(c.miss_ev)) != hipSuccess) return 1;
    } else {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return 1; }
        c.miss_ev = ev;
    }
    std::vector<int> kept(k), frames(k), status(k);
    sswav::read_many(cp, k, ld->stage, 2LL * ld->cap, ld->cap, ld->keep, false, kept.data(), frames.data(), status.data(),
                     ld->threads > 0 ? ld->threads : 1, rows16 ? ld->stage_max : nullptr);
    for (int i = 0; i < k; ++i)
        if (status[i] != sswav::kOk && status[i] != sswav::kEmpty) return 1;     // scipy's semantics are the caller's reader's
#if !defined(SS_AB_NO_LOADER_LANE_ORDER)                       // (A/B builds: tests/test_wav_loader.py's write-after-read case fails without)
    if (order_behind_lanes(c, st)) return 1;                   // (overlap mode: steps in flight may read the entries rewritten below)
#endif
    // ---- commit
    for (size_t i = 0; i < victims.size(); ++i) ld->evicted_slot[i] = victims[i];
    ld->n_evicted = static_cast<int>(victims.size());
    const int from_free = k < ld->n_free ? k : ld->n_free;
    ld->n_free -= from_free;
    for (int i = 0; i < k; ++i) {
        const int slot = take[i];
        ld->stage_slot[i] = slot;
        ld->stage_len[i] = kept[i];
        ld->host_len[slot] = kept[i];
        ld->clipped[slot] = kept[i] < frames[i];
        if (ld->spec_stale) ld->spec_stale[slot] = 1;
        ld->loaded_slot[i] = slot; ld->loaded_frames[i] = frames[i];
        if (last_used && slot < n_slots) last_used[slot] = tick;
    }
    ld->n_loaded = k;
    int rc = 0;
    if (rows16) {                                              // staged rows + their maxima -> halves, scales, lengths: one launch
        rc = ss_bank_scatter_rows16_max_f32(ld->stage, 2LL * ld->cap, ld->stage_slot, ld->stage_len, ld->stage_max, k,
                                            const_cast<void*>(c.rir16), const_cast<float*>(c.rscale), ld->cap, ld->dev_len, st);
    } else if (spec_only) {                                    // staged rows -> block spectra + lengths, one launch
        // (a half bank, ss_ctx_set_rir_spectra16, through the half staging kernel: never fp32 spectra into its buffer)
        rc = c.hscale ? ss_bank_scatter_spectra16_f32(ld->stage, 2LL * ld->cap, 0, ld->stage_slot, ld->stage_len, k,
                                                      const_cast<float*>(c.hspec), const_cast<float*>(c.hscale), hb, ld->dev_len, st)
                      : ss_bank_scatter_spectra_f32(ld->stage, 2LL * ld->cap, 0, ld->stage_slot, ld->stage_len, k,
                                                    const_cast<float*>(c.hspec), hb, ld->dev_len, st);
        if (rc == 0 && ld->spec_stale)
            for (int i = 0; i < k; ++i) ld->spec_stale[ld->stage_slot[i]] = 0;
    } else {
        rc = ss_bank_scatter_rows_f32(ld->stage, 2LL * ld->cap, ld->stage_slot, ld->stage_len, k, ld->bank, ld->bank_unit_stride,
                                      ld->bank_chan_stride, ld->cap, ld->dev_len, st);
    }
    if (rc == 0 && spectral && !spec_only) {
        // the new rows' block spectra H'_i = 2 rFFT(block i), straight into the spectral bank (scatter form of k_source_windows;
        // the descriptors are read from the pinned block in place)
        int w = 0;
        for (int i = 0; i < k; ++i)
            for (int ch = 0; ch < 2; ++ch)
                for (int b = 0; b < hb; ++b, ++w) {
                    const int slot = ld->stage_slot[i], left = ld->cap - b * ssk::kB;
                    int* d = ld->stage_desc + 5 * w;
                    d[0] = static_cast<int>(slot * ld->bank_unit_stride + static_cast<long long>(ch) * ld->bank_chan_stride + static_cast<long long>(b) * ssk::kB);
                    d[1] = left < ssk::kB ? left : ssk::kB;
                    d[2] = 0; d[3] = 0;
                    d[4] = (slot * 2 + ch) * hb + b;
                }
        ssk::SrcParams sp;
        rc = get_tables(&sp.tb);
        if (rc == 0) {
            sp.src = ld->bank;
            sp.desc = ld->stage_desc;
            sp.spec = reinterpret_cast<ssk::f32x4*>(const_cast<float*>(c.hspec));
            sp.desc_stride = 5;
            sp.scale = 1.0f;
            hipLaunchKernelGGL(ssk::k_source_windows, dim3(w), dim3(ssk::kT), 0, st, sp);
            rc = hip_err(hipGetLastError());
        }
        if (rc == 0 && ld->spec_stale)
            for (int i = 0; i < k; ++i) ld->spec_stale[ld->stage_slot[i]] = 0;
    }
    if (rc == 0) rc = hip_err(hipEventRecord(static_cast<hipEvent_t>(c.miss_ev), st));
    return rc;
}

// The miss path inside the call (include/ss_hip.h: ss_miss_loader).  Returns 1 = "not for the fast path" (nothing was changed).
static int serve_pose_misses(ss_ctx* h, const long long* recs, int n, ss_request_tables* tb, ss_miss_loader* ld, const int* miss,
                             int n_miss, hipStream_t st, bool spectral) {
    ssctx::Context& c = h->c;
    const int hb = (ld && ld->cap > 0) ? (ld->cap + ssk::kB - 1) / ssk::kB : 1;
    const bool spec_only = ld && !ld->bank && !c.rir && c.hspec && spectral;       // spectral-only bank: no rows, no descriptors
    const bool rows16 = loader_rows16(c, ld) && !spectral;                        // half-precision time-domain rows
    if (spectral && (!ld || (!spec_only && !ld->stage_desc) || c.h_blocks != hb)) return 1;
    if (!ld || !ld->table_dirs || !ld->pair_keys || !ld->pair_slots || !ld->free_slots || (!ld->bank && !spec_only && !rows16) || !ld->dev_len ||
        !ld->host_len || !ld->clipped || !ld->stage || !ld->stage_slot || !ld->stage_len || !ld->loaded_key || !ld->loaded_slot ||
        !ld->loaded_frames || ld->cap < 2 || (ld->cap & 1) || tb->pair_keys != ld->pair_keys || tb->pair_slots != ld->pair_slots)
        return 1;
    const int n_src = static_cast<int>(c.src_len.size());
    std::vector<long long> keys;
    auto want = [&](long long tid, long long recv, long long src) -> bool {      // false: not serviceable here
        if (recv < 0 || src < 0 || recv >= (1 << 20) || src >= (1 << 20) || tid >= ld->n_table_dirs || !ld->table_dirs[tid]) return false;
        const long long key = (tid << 40) | (recv << 20) | src;
        const long long s = find_key(tb->pair_keys, tb->pair_slots, tb->n_pairs, key);
        if (s >= 0) return !(tb->stale && s < tb->n_slots && tb->stale[s]);      // resident (a stale row is the caller's reload)
        keys.push_back(key);
        return true;
    };
    for (int k = 0; k < n_miss; ++k) {
        const long long* r = recs + static_cast<size_t>(miss[k]) * SS_REQ_WORDS;
        const long long sid = find_key(tb->sound_keys, tb->sound_ids, tb->n_sounds, r[1]);
        const long long tid = find_key(tb->table_keys, tb->table_ids, tb->n_tables, r[3]);
        if (sid < 0 || sid >= n_src || tid < 0 || r[2] < 0 || r[2] > 0x7fffffffLL) return 1;
        if (!want(tid, r[4], r[5])) return 1;
        if (r[6] >= 0) {
            const long long did = find_key(tb->sound_keys, tb->sound_ids, tb->n_sounds, r[6]);
            if (did < 0 || did >= n_src || !want(tid, r[4], r[7])) return 1;
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const int k = static_cast<int>(keys.size());
    if (k == 0 || k > ld->stage_rows || k > ld->loaded_cap || tb->n_pairs + k > ld->pair_cap) return 1;
    int rc = 0;
    {
        std::vector<std::string> paths(k);
        std::vector<const char*> cp(k);
        for (int i = 0; i < k; ++i) {
            const long long key = keys[i];
            paths[i] = std::string(ld->table_dirs[key >> 40]) + "/" + std::to_string((key >> 20) & 0xFFFFF) + "_" +
                       std::to_string(key & 0xFFFFF) + ".wav";                   // simulator.py:615-616
            cp[i] = paths[i].c_str();
        }
        const int rc_l = loader_load_paths(c, ld, cp.data(), k, tb->last_used, tb->tick, tb->n_slots, spectral, st);
        if (rc_l == 1) return 1;
        for (int i = 0; i < k; ++i) ld->loaded_key[i] = keys[i];
        if (ld->n_evicted) {                                   // the evicted entries' pairs leave the sorted arrays (one compacting pass)
            std::vector<char> gone(static_cast<size_t>(tb->n_slots), 0);
            for (int i = 0; i < ld->n_evicted; ++i) gone[ld->evicted_slot[i]] = 1;
            int o = 0;
            for (int i = 0; i < tb->n_pairs; ++i) {
                const long long sl = ld->pair_slots[i];
                if (sl >= 0 && sl < tb->n_slots && gone[sl]) continue;
                ld->pair_keys[o] = ld->pair_keys[i]; ld->pair_slots[o] = ld->pair_slots[i]; ++o;
            }
            tb->n_pairs = o;
        }
        rc = rc_l;
    }
    // the sorted pair arrays, in place (keys ascending: merged from the back)
    {
        int i = tb->n_pairs - 1, j = k - 1, o = tb->n_pairs + k - 1;
        while (j >= 0) {
            if (i >= 0 && ld->pair_keys[i] > keys[j]) { ld->pair_keys[o] = ld->pair_keys[i]; ld->pair_slots[o] = ld->pair_slots[i]; --i; }
            else { ld->pair_keys[o] = keys[j]; ld->pair_slots[o] = ld->loaded_slot[j]; --j; }
            --o;
        }
        tb->n_pairs += k;
    }
    return rc;                                                 // (< 0: the rows are booked, the launch failed: the caller sees the error)
}

int ss_ctx_load_rir_files(ss_ctx* h, ss_miss_loader* ld, const char* const* paths, int k, long long* last_used, long long tick,
                          int n_slots, void* stream) {
    if (!h || !ld || !paths || k < 0) return SS_EINVAL;
    ld->n_loaded = 0; ld->n_evicted = 0;
    if (k == 0) return 0;
    ssctx::Context& c = h->c;
    if (!c.rir16_buckets.empty()) return 1;                    // half rows in length buckets: not served here
    const bool rows16 = loader_rows16(c, ld);                  // half rows, one allocation: the one-pass scatter (see loader_load_paths)
    if (c.rir16 && !rows16) return 1;                          // ... without stage_max / with another capacity: the caller's own path
    const bool spec_only = !ld->bank && !c.rir && c.hspec && c.buckets.empty();     // spectral-only bank (see loader_load_paths)
    if (!ld->free_slots || (!ld->bank && !spec_only && !rows16) || !ld->dev_len || !ld->host_len || !ld->clipped || !ld->stage || !ld->stage_slot ||
        !ld->stage_len || !ld->loaded_slot || !ld->loaded_frames || ld->cap < 2 || (ld->cap & 1) || c.rir != ld->bank)
        return 1;
    // (rows of a store that keeps the spectral form get their block spectra right away: whichever form the next launch reads)
    return loader_load_paths(c, ld, paths, k, last_used, tick, n_slots, c.hspec != nullptr, static_cast<hipStream_t>(stream));
}

int ss_ctx_observe_requests_load(ss_ctx* h, const long long* recs, int n, ss_request_tables* tb, ss_miss_loader* ld, float* audiogoal,
                                 float* spectrogram, int* miss_out, int* n_miss, void* stream) {
    if (!h || n < 0 || !tb) return SS_EINVAL;
    if (ld) { ld->n_loaded = 0; ld->n_evicted = 0; }
    std::vector<int>& w = h->c.sim_scratch;
    w.resize(static_cast<size_t>(n) * 5 + 1);
    int rc = requests_to_units(h, recs, n, tb, w.data(), miss_out, n_miss);
    if (rc != 0 || n == 0) return rc;
    if (*n_miss) {
        ssctx::Context& c = h->c;
        // a launch that reads the SPECTRAL rows needs the new rows' block spectra first (built behind the scatter)
        bool any_dis = false;
        for (int i = 0; i < n && !any_dis; ++i) any_dis = recs[static_cast<size_t>(i) * SS_REQ_WORDS] == 0 && recs[static_cast<size_t>(i) * SS_REQ_WORDS + 6] >= 0;
        const bool spectral = c.hspec && !(c.policy.spectral_max_units > 0 && c.rir && c.out_len <= ssk::kB && n > c.policy.spectral_max_units && !any_dis);
        // (half rows: served through loader_rows16's form of the struct; otherwise, and in length buckets, the misses are reported)
        if (!ld || !miss_out || c.rir != ld->bank || (c.rir16 && !loader_rows16(c, ld)) || !c.rir16_buckets.empty()) return 0;
        std::vector<int> miss(miss_out, miss_out + (*n_miss < n ? *n_miss : n));
        rc = serve_pose_misses(h, recs, n, tb, ld, miss.data(), static_cast<int>(miss.size()), static_cast<hipStream_t>(stream), spectral);
        if (rc == 1) return 0;                                 // reported as ss_ctx_observe_requests reports it
        if (rc) return rc;
        rc = requests_to_units(h, recs, n, tb, w.data(), miss_out, n_miss);
        if (rc != 0 || *n_miss) return rc;
    }
    ss_units u;
    std::memset(&u, 0, sizeof u);
    u.sound = w.data(); u.t0 = u.sound + n; u.rir = u.t0 + n;
    bool any_dis = false;
    for (int i = 0; i < n && !any_dis; ++i) any_dis = u.rir[n + n + i] >= 0;
    if (any_dis) { u.dis_sound = u.rir + n; u.dis_rir = u.dis_sound + n; }
    return ss_ctx_observe(h, &u, n, audiogoal, spectrogram, stream);
}

}  // extern "C"

extern "C" {

int ss_fftconv_binaural_buckets_f32(const float* spec, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len,
                                    const int* unit_desc, float* out, int n_units, int n_valid, int out_len, int flags,
                                    void* stream) {
    if (n_units == 0) return 0;
    return render(buckets_bank(buckets, n_buckets), false, Launch::kConv, spec, rir_len, unit_desc, out, nullptr, nullptr, n_units,
                  n_valid, out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

int ss_audio_obs_buckets_f32(const float* spec, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len,
                             const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid,
                             int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    return render(buckets_bank(buckets, n_buckets), false, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// Log-mel observation from a length-bucketed bank in ONE launch, no waveform buffer needed: the log-mel forms of the kernels
// ss_audio_obs_buckets_f32 launches for the same shape (k_conv / k_conv_spec <loop, MEL> for one-block rows, k_obs_blocks /
// k_obs_rows <.., BUCKETS, MEL> for rows of 2 or 3 blocks).  Launches that only touch bucket 0 (one bucket, or
// SS_FLAG_FIRST_BUCKET) are single-allocation launches on bucket 0's arrays: the existing log-mel launchers, loop-free kernels
// included.  Every argument is checked before a device is touched.
int ss_audio_obs_logmel_buckets_f32(const float* spec, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len,
                                    const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel, const int* mel_start,
                                    const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units, int n_valid, int out_len,
                                    int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(buckets_bank(buckets, n_buckets), false, out_len <= ssk::kB ? Launch::kMelOneBlock : Launch::kMelRows, spec, rir_len,
                  unit_desc, audiogoal, spectrogram, &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// The context's bank as length buckets (replaces ss_ctx_set_rir_bank + ss_ctx_set_rir_spectra for such banks; borrowed
// device pointers, the array itself is copied).  Steps whose units all sit in bucket 0 keep the loop-free kernels.
int ss_ctx_set_rir_buckets(ss_ctx* h, const ss_rir_bucket* buckets, int n_buckets, const int* rir_len) {
    if (!h || !buckets || !rir_len || n_buckets < 1 || n_buckets > ssk::kMaxBuckets) return SS_EINVAL;
    ssk::ConvParams probe;
    int hb_max = 1;
    for (auto& b : probe.bk) b = ssk::BankBucket{nullptr, nullptr, 0x7fffffff, 0, 0, 0};
    int rc = fill_buckets(probe, buckets, n_buckets, false, &hb_max);
    if (rc) return rc;
    ssctx::Context& c = h->c;
    const int nbh_old = c.rir_cap > 0 ? ssctx::ceil_div(c.rir_cap, c.kb) : 1;
    c.buckets.assign(buckets, buckets + n_buckets);
    c.spec_buckets.clear();
    c.rir = buckets[0].rir; c.rir_len = rir_len; c.rir_us = 2LL * buckets[0].cap; c.rir_cs = buckets[0].cap; c.rir_es = 1;
    c.rir16 = nullptr; c.rscale = nullptr; c.rir16_buckets.clear();
    c.rir_cap = hb_max * c.kb;                                 // planning depth: the longest bucket's blocks
    c.hspec = nullptr; c.hscale = nullptr; c.h_blocks = 0;
    if (hb_max != nbh_old) {                                   // the set of partition offsets per key changes
        const int nby = c.n_valid > 0 ? ssctx::ceil_div(c.n_valid, c.kb) : 1;
        c.stride = hb_max + nby - 1;
        ssctx::cache_reset(c);
        if (c.pool) {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_err(e);
            (void)hipFree(c.pool);
            c.pool = nullptr;
            c.pool_entries = 0;
        }
    }
    return 0;
}

}  // extern "C"

extern "C" {

int ss_fftconv_binaural_spec_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                         const int* unit_desc, float* out, int n_units, int n_valid, int out_len, int flags,
                                         void* stream) {
    if (n_units == 0) return 0;
    return render(spec_buckets_bank(buckets, n_buckets), true, Launch::kConv, spec, rir_len, unit_desc, out, nullptr, nullptr, n_units,
                  n_valid, out_len, SS_PAD_REFLECT, flags, stateless(stream));
}

int ss_audio_obs_spec_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                  const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid, int out_len,
                                  int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    return render(spec_buckets_bank(buckets, n_buckets), true, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram, nullptr,
                  n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_logmel_buckets_f32 on spectral length buckets.  fp32: the log-mel forms of the kernels
// ss_audio_obs_spec_buckets_f32 launches (k_conv_spec<loop, MEL>; k_obs_blocks / k_obs_rows <true, .., BUCKETS, MEL>).  Half:
// one-block rows, k_conv_spec<.., MEL, HALF, HBK>.  Bucket-0 launches: the single-allocation log-mel launchers, as above.
int ss_audio_obs_logmel_spec_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                         const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                         const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps, int n_units,
                                         int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(spec_buckets_bank(buckets, n_buckets), true, out_len <= ssk::kB ? Launch::kMelOneBlock : Launch::kMelRows, spec,
                  rir_len, unit_desc, audiogoal, spectrogram, &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ---- half spectral length buckets, rows of 2 or 3 partition blocks (44.1 / 48 kHz): k_obs_blocks<true, MEL, HALF, HBK> /
// k_obs_rows<true, false, BUCKETS, MEL, HALF> ----
// what the two entries refuse on top of render(): anything but the half form, rows the fused row kernels do not serve
static bool spec16_buckets_rows_args_ok(const ss_spec_bucket* buckets, int n_buckets, int n_units, int n_valid, int out_len, int pad_mode,
                                        int flags) {
    bool half = false;
    int hb_max = 1;
    if (n_units < 0 || spec_buckets_check(buckets, n_buckets, &half, &hb_max) || !half || (flags & SS_FLAG_CROSSFADE)) return false;
    if (pad_mode != SS_PAD_REFLECT && pad_mode != SS_PAD_CONSTANT) return false;
    return out_len > ssk::kB && out_len <= 3 * ssk::kB && n_valid >= 0 && n_valid <= out_len;
}

// ss_audio_obs_rows_spec16_f32 on half spectral length buckets: the same routing (k_obs_blocks while the grid fits the chip,
// k_obs_rows beyond; shapes the fp32 entry hands to the unfused convolution + k_spectrogram go to the half convolution).
// Launches that only touch bucket 0 (one bucket, or SS_FLAG_FIRST_BUCKET) are single-allocation launches on bucket 0's arrays.
int ss_audio_obs_rows_spec16_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                         const int* unit_desc, float* audiogoal, float* spectrogram, int n_units, int n_valid,
                                         int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!spectrogram || !spec16_buckets_rows_args_ok(buckets, n_buckets, n_units, n_valid, out_len, pad_mode, flags)) return SS_EINVAL;
    return render(spec_buckets_bank(buckets, n_buckets, true), true, Launch::kObs, spec, rir_len, unit_desc, audiogoal, spectrogram,
                  nullptr, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

// ss_audio_obs_logmel_rows_spec16_f32 on half spectral length buckets
int ss_audio_obs_logmel_rows_spec16_buckets_f32(const float* spec, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len,
                                                const int* unit_desc, float* audiogoal, float* spectrogram, float* logmel,
                                                const int* mel_start, const float* mel_w, int n_mels, int max_len, float mel_eps,
                                                int n_units, int n_valid, int out_len, int pad_mode, int flags, void* stream) {
    if (n_units == 0) return 0;
    if (!spec16_buckets_rows_args_ok(buckets, n_buckets, n_units, n_valid, out_len, pad_mode, flags)) return SS_EINVAL;
    if (!mel_args_ok(logmel, mel_start, mel_w, n_mels, max_len, mel_eps)) return SS_EINVAL;
    const ssk::MelArgs m{logmel, mel_start, mel_w, n_mels, max_len, mel_eps};
    return render(spec_buckets_bank(buckets, n_buckets, true), true, Launch::kMelRows, spec, rir_len, unit_desc, audiogoal, spectrogram,
                  &m, n_units, n_valid, out_len, pad_mode, flags, stateless(stream));
}

static int ctx_bind_spec_buckets(ss_ctx* h, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len, bool rows);

// The context's bank as spectral length buckets: replaces any earlier binding (rows, spectra of either form, ss_rir_bucket
// buckets); the descriptor array is copied, the device pointers are borrowed.  Planning depth as ss_ctx_set_rir_buckets.
int ss_ctx_set_rir_spec_buckets(ss_ctx* h, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len) {
    return ctx_bind_spec_buckets(h, buckets, n_buckets, rir_len, false);
}

// ... HALF buckets on a context whose rows are 2 or 3 partition blocks (kB < sampling_rate <= 3 kB): spectrogram steps go to
// ss_audio_obs_rows_spec16_buckets_f32, log-mel steps inside ss_ctx_set_logmel_buckets_policy's range to
// ss_audio_obs_logmel_rows_spec16_buckets_f32, waveform-only steps to ss_fftconv_binaural_spec_buckets_f32.  Same preconditions
// otherwise; refused on a context of one-block rows and for fp32 buckets.
int ss_ctx_set_rir_spec_buckets_rows(ss_ctx* h, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len) {
    return ctx_bind_spec_buckets(h, buckets, n_buckets, rir_len, true);
}

// Half-precision time-domain rows in length buckets as the context's bank: replaces any earlier binding (ss_ctx_set_rir_bank clears
// every form and resets keys and pool where the depth changes), buckets = NULL unbinds.  Planning depth: the deepest bucket's blocks.
int ss_ctx_set_rir16_buckets(ss_ctx* h, const ss_rir16_bucket* buckets, int n_buckets, const int* rir_len) {
    if (!h) return SS_EINVAL;
    if (!buckets) {
        h->c.rir16_buckets.clear();
        return 0;
    }
    int hb_max = 1;
    if (!rir_len || rir16_buckets_check(buckets, n_buckets, &hb_max)) return SS_EINVAL;
    const int rc = ss_ctx_set_rir_bank(h, nullptr, rir_len, 0, 0, 1, hb_max * h->c.kb);
    if (rc) return rc;
    h->c.rir16_buckets.assign(buckets, buckets + n_buckets);
    return 0;
}

static int ctx_bind_spec_buckets(ss_ctx* h, const ss_spec_bucket* buckets, int n_buckets, const int* rir_len, bool rows) {
    bool half = false;
    int hb_max = 1;
    if (!h || !rir_len || spec_buckets_check(buckets, n_buckets, &half, &hb_max)) return SS_EINVAL;
    ssctx::Context& c = h->c;
    if (rows) {
        if (!half || c.out_len <= c.kb || c.out_len > 3 * c.kb) return SS_EINVAL;
    } else if (half && c.out_len > c.kb) return SS_EINVAL;     // (ss_audio_obs_spec_buckets_f32: half serves one-block rows)
    const int nbh_old = c.rir_cap > 0 ? ssctx::ceil_div(c.rir_cap, c.kb) : 1;
    c.spec_buckets.assign(buckets, buckets + n_buckets);
    c.spec_buckets_rows = rows;
    c.buckets.clear();
    c.rir = nullptr; c.rir_len = rir_len; c.rir_us = 0; c.rir_cs = 0; c.rir_es = 1;
    c.rir16 = nullptr; c.rscale = nullptr; c.rir16_buckets.clear();
    c.rir_cap = hb_max * c.kb;                                 // planning depth: the longest bucket's blocks
    c.hspec = nullptr; c.hscale = nullptr; c.h_blocks = 0;
    if (hb_max != nbh_old) {                                   // the set of partition offsets per key changes
        const int nby = c.n_valid > 0 ? ssctx::ceil_div(c.n_valid, c.kb) : 1;
        c.stride = hb_max + nby - 1;
        ssctx::cache_reset(c);
        if (c.pool) {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_err(e);
            (void)hipFree(c.pool);
            c.pool = nullptr;
            c.pool_entries = 0;
        }
    }
    return 0;
}

}  // extern "C"

// ---- RIR files -> staging rows (host only; see ss_wavio.hpp) ------------------------------------------------------
extern "C" int ss_wav_read_rirs_f32(const char* const* paths, int n, float* dst, long long row_stride, int cap, int keep,
                                    int planar, int* kept_out, int* frames_out, int* status_out, int n_threads) {
    if (n == 0) return 0;
    if (!paths || !dst || !kept_out || !frames_out || !status_out || n < 0 || cap < 1 || row_stride < 2LL * cap) return SS_EINVAL;
    sswav::read_many(paths, n, dst, row_stride, cap, keep, planar != 0, kept_out, frames_out, status_out, n_threads);
    return 0;
}

// ... with the maxima of |v| over each row's kept frames, per ear, taken on the reader's thread (wav layout only)
extern "C" int ss_wav_read_rirs_max_f32(const char* const* paths, int n, float* dst, long long row_stride, int cap, int keep,
                                        int* kept_out, int* frames_out, int* status_out, int n_threads, float* max_out) {
    if (n == 0) return 0;
    if (!paths || !dst || !kept_out || !frames_out || !status_out || !max_out || n < 0 || cap < 1 || row_stride < 2LL * cap)
        return SS_EINVAL;
    sswav::read_many(paths, n, dst, row_stride, cap, keep, false, kept_out, frames_out, status_out, n_threads, max_out);
    return 0;
}

// Staged rows (wav layout, pinned host or device memory) -> planar bank rows + their lengths, one launch (k_scatter_rows)
extern "C" int ss_bank_scatter_rows_f32(const float* staged, long long staged_row_stride, const int* slots, const int* lens,
                                        int n, float* bank, long long unit_stride, int chan_stride, int cap, int* bank_len,
                                        void* stream) {
    if (n == 0) return 0;
    if (!staged || !slots || !lens || !bank || n < 0 || cap <= 0 || unit_stride <= 0 || chan_stride <= 0 ||
        staged_row_stride < 2LL * cap) return SS_EINVAL;
    // the kernel dereferences all three inputs: pageable host memory here would be a GPU memory fault (the process dies), not
    // an error code - refuse anything the runtime does not know as device-accessible (pinned / registered host, device, managed)
    for (const void* ptr : {static_cast<const void*>(staged), static_cast<const void*>(slots), static_cast<const void*>(lens)}) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) { (void)hipGetLastError(); return SS_EINVAL; }
        if (attr.type != hipMemoryTypeHost && attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) return SS_EINVAL;
    }
    ssk::ScatterRowsParams p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.bank = bank; p.bank_len = bank_len;
    p.staged_stride = staged_row_stride; p.unit_stride = unit_stride; p.chan_stride = chan_stride; p.cap = cap;
    for (int lo = 0; lo < n; lo += 65535) {                    // (grid.y limit)
        const int m = n - lo < 65535 ? n - lo : 65535;
        ssk::ScatterRowsParams q = p;
        q.staged += static_cast<size_t>(lo) * staged_row_stride; q.slots += lo; q.lens += lo;
        hipLaunchKernelGGL(ssk::k_scatter_rows, dim3((cap + 511) / 512, m), dim3(256), 0, static_cast<hipStream_t>(stream), q);
    }
    return hip_err(hipGetLastError());
}

// the kernel dereferences these: pageable host memory would be a GPU memory fault (the process dies), not an error code -
// refuse anything the runtime does not know as device-accessible (pinned / registered host, device, managed)
static bool device_accessible(const void* ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// Staged rows (wav or planar layout, pinned host or device memory) -> block spectra of a spectral-only bank + its lengths, one
// launch (k_stage_spectra).  Both staging forms are accepted; which is faster depends on the number of rows: a workgroup that
// pulls its 128 KiB block over the host link waits at the link's latency, which a handful of rows hides and dozens do not
// (profiles/r7, one sequential run, noisy: 1 row pulled 123 us against 130 us copied first, 32 rows 487 against 368 us per 128-env
// miss step).  The Python
// stores pull blocks of <= RirStore.spectra_pull_rows rows and copy larger ones; the in-call loaders pull (their steps load few).
extern "C" int ss_bank_scatter_spectra_f32(const float* staged, long long staged_row_stride, int planar, const int* slots,
                                           const int* lens, int n, float* hspec, int h_blocks, int* bank_len, void* stream) {
    if (n == 0) return 0;
    if (!staged || !slots || !lens || !hspec || n < 0 || h_blocks < 1 || staged_row_stride < 2) return SS_EINVAL;
    // 8-byte loads: pairs of frames (planar: of one ear, the second ear half a row further) or both ears of a frame (wav)
    if ((reinterpret_cast<size_t>(staged) & 7) || (staged_row_stride & (planar ? 3 : 1))) return SS_EINVAL;
    for (const void* ptr : {static_cast<const void*>(staged), static_cast<const void*>(slots), static_cast<const void*>(lens)})
        if (!device_accessible(ptr)) return SS_EINVAL;
    ssk::StageSpecParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    const long long frames = staged_row_stride / 2, hb_frames = static_cast<long long>(h_blocks) * ssk::kB;
    p.staged = staged; p.slots = slots; p.lens = lens; p.hspec = reinterpret_cast<ssk::f32x4*>(hspec); p.bank_len = bank_len;
    p.staged_stride = staged_row_stride; p.planar = planar ? 1 : 0; p.h_blocks = h_blocks;
    p.cap = static_cast<int>(std::min(frames, hb_frames));
    p.hscale = nullptr; p.ear_off = 0; p.slot0 = 0; p.pair_loads = 1;
    for (int lo = 0; lo < n; lo += 65535) {                    // (grid.y limit)
        const int m = n - lo < 65535 ? n - lo : 65535;
        ssk::StageSpecParams q = p;
        q.staged += static_cast<size_t>(lo) * staged_row_stride; q.slots += lo; q.lens += lo;
        hipLaunchKernelGGL(ssk::k_stage_spectra, dim3(h_blocks, m), dim3(ssk::kT), 0, static_cast<hipStream_t>(stream), q);
    }
    return hip_err(hipGetLastError());
}

// The same staging, into a HALF bank (k_stage_spectra16): fp16 block spectra [entries][2][h_blocks][ss_spec_floats()] and one
// fp32 scale per (entry, ear, block), quantised from the very values the fp32 entry stores.
extern "C" int ss_bank_scatter_spectra16_f32(const float* staged, long long staged_row_stride, int planar, const int* slots,
                                             const int* lens, int n, void* hspec16, float* hscale, int h_blocks, int* bank_len,
                                             void* stream) {
    if (n == 0) return 0;
    if (!staged || !slots || !lens || !hspec16 || !hscale || n < 0 || h_blocks < 1 || staged_row_stride < 2) return SS_EINVAL;
    if ((reinterpret_cast<size_t>(staged) & 7) || (staged_row_stride & (planar ? 3 : 1)) || (reinterpret_cast<size_t>(hspec16) & 7))
        return SS_EINVAL;
    for (const void* ptr : {static_cast<const void*>(staged), static_cast<const void*>(slots), static_cast<const void*>(lens)})
        if (!device_accessible(ptr)) return SS_EINVAL;
    ssk::StageSpecParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    const long long frames = staged_row_stride / 2, hb_frames = static_cast<long long>(h_blocks) * ssk::kB;
    p.staged = staged; p.slots = slots; p.lens = lens; p.hspec = static_cast<ssk::f32x4*>(hspec16); p.bank_len = bank_len;
    p.staged_stride = staged_row_stride; p.planar = planar ? 1 : 0; p.h_blocks = h_blocks;
    p.cap = static_cast<int>(std::min(frames, hb_frames));
    p.hscale = hscale; p.ear_off = staged_row_stride >> 1; p.slot0 = 0; p.pair_loads = 1;
    for (int lo = 0; lo < n; lo += 65535) {                    // (grid.y limit)
        const int m = n - lo < 65535 ? n - lo : 65535;
        ssk::StageSpecParams q = p;
        q.staged += static_cast<size_t>(lo) * staged_row_stride; q.slots += lo; q.lens += lo;
        hipLaunchKernelGGL(ssk::k_stage_spectra16, dim3(h_blocks, m), dim3(ssk::kT), 0, static_cast<hipStream_t>(stream), q);
    }
    return hip_err(hipGetLastError());
}

// A planar device bank ([n][2][rir_cap]-like rows, zero beyond each entry's length) -> its half form, entry r to entry r: the same
// kernel with the bank as its staging block (rows of rir_cap frames, the second ear rir_chan_stride floats behind the first)
extern "C" int ss_rir_spectra16_f32(const float* rir, void* hspec16_out, float* hscale_out, int n_entries, long long rir_unit_stride,
                                    int rir_chan_stride, int rir_cap, void* stream) {
    if (n_entries == 0) return 0;
    if (!rir || !hspec16_out || !hscale_out || n_entries < 0 || rir_cap <= 0 || rir_unit_stride < 0 || rir_chan_stride < 0) return SS_EINVAL;
    if (reinterpret_cast<size_t>(hspec16_out) & 7) return SS_EINVAL;
    ssk::StageSpecParams p;
    int rc = get_tables(&p.tb);
    if (rc) return rc;
    p.staged = rir; p.slots = nullptr; p.lens = nullptr; p.hspec = static_cast<ssk::f32x4*>(hspec16_out); p.bank_len = nullptr;
    p.staged_stride = rir_unit_stride; p.planar = 1; p.h_blocks = (rir_cap + ssk::kB - 1) / ssk::kB;
    p.cap = rir_cap;
    p.hscale = hscale_out; p.ear_off = rir_chan_stride; p.slot0 = 0;
    p.pair_loads = !(reinterpret_cast<size_t>(rir) & 7) && !(rir_unit_stride & 1) && !(rir_chan_stride & 1);
    for (int lo = 0; lo < n_entries; lo += 65535) {            // (grid.y limit)
        const int m = n_entries - lo < 65535 ? n_entries - lo : 65535;
        ssk::StageSpecParams q = p;
        q.staged += static_cast<size_t>(lo) * rir_unit_stride; q.slot0 = lo;
        hipLaunchKernelGGL(ssk::k_stage_spectra16, dim3(p.h_blocks, m), dim3(ssk::kT), 0, static_cast<hipStream_t>(stream), q);
    }
    return hip_err(hipGetLastError());
}

extern "C" int ss_rows_gather_f32(const float* const* src, const int* n_floats, int n, float* dst, long long row_stride,
                                  int row_floats, int n_threads) {
    if (n == 0) return 0;
    if (!src || !n_floats || !dst || n < 0 || row_floats < 0 || row_stride < row_floats) return SS_EINVAL;
    sswav::gather_rows(src, n_floats, n, dst, row_stride, row_floats, n_threads);
    return 0;
}

// ---- half-precision time-domain rows: the producers -----------------------------------------------------------------------
// A planar fp32 device bank -> its half form, entry r to entry r (k_rows_half: one workgroup per (entry, ear))
extern "C" int ss_rir_rows16_f32(const float* rir, void* rir16_out, float* rscale_out, int n_entries, long long rir_unit_stride,
                                 int rir_chan_stride, int rir_cap, void* stream) {
    if (n_entries == 0) return 0;
    if (!rir || n_entries < 0 || rir_unit_stride < 0 || rir_chan_stride < 0 || !rows16_bank_ok(rir16_out, rscale_out, rir_cap))
        return SS_EINVAL;
    ssk::RowsHalfParams p;
    p.rir = rir; p.rir16 = static_cast<ssk::h16x2*>(rir16_out); p.rscale = rscale_out;
    p.unit_stride = rir_unit_stride; p.chan_stride = rir_chan_stride; p.cap = rir_cap;
    for (int lo = 0; lo < n_entries; lo += 65535) {            // (grid.y limit)
        const int m = n_entries - lo < 65535 ? n_entries - lo : 65535;
        ssk::RowsHalfParams q = p;
        q.rir += static_cast<size_t>(lo) * rir_unit_stride;
        q.rir16 += static_cast<size_t>(lo) * rir_cap;          // (2 ears x cap / 2 pairs per entry)
        q.rscale += static_cast<size_t>(lo) * 2;
        hipLaunchKernelGGL(ssk::k_rows_half, dim3(2, m), dim3(256), 0, static_cast<hipStream_t>(stream), q);
    }
    return hip_err(hipGetLastError());
}

// Staged rows (wav layout, pinned host or device memory) -> halves + scales of a half-rows bank + their lengths, one launch
// (k_scatter_rows16); the staging contract of ss_bank_scatter_rows_f32
extern "C" int ss_bank_scatter_rows16_f32(const float* staged, long long staged_row_stride, const int* slots, const int* lens, int n,
                                          void* rir16, float* rscale, int cap, int* bank_len, void* stream) {
    if (n == 0) return 0;
    if (!staged || !slots || !lens || n < 0 || !rows16_bank_ok(rir16, rscale, cap) || staged_row_stride < 2LL * cap) return SS_EINVAL;
    if ((reinterpret_cast<size_t>(staged) & 7) || (staged_row_stride & 1)) return SS_EINVAL;      // a frame is one 8-byte load
    for (const void* ptr : {static_cast<const void*>(staged), static_cast<const void*>(slots), static_cast<const void*>(lens)})
        if (!device_accessible(ptr)) return SS_EINVAL;
    ssk::ScatterRows16Params p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.rir16 = static_cast<ssk::h16x2*>(rir16); p.rscale = rscale;
    p.bank_len = bank_len; p.staged_stride = staged_row_stride; p.cap = cap;
    hipLaunchKernelGGL(ssk::k_scatter_rows16, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return hip_err(hipGetLastError());
}

// The same hop in one pass over each row, the rows' maxima given (k_scatter_rows16_max; ss_wav_read_rirs_max_f32 supplies them)
extern "C" int ss_bank_scatter_rows16_max_f32(const float* staged, long long staged_row_stride, const int* slots, const int* lens,
                                              const float* row_max, int n, void* rir16, float* rscale, int cap, int* bank_len,
                                              void* stream) {
    if (n == 0) return 0;
    if (!staged || !slots || !lens || !row_max || n < 0 || !rows16_bank_ok(rir16, rscale, cap) || staged_row_stride < 2LL * cap)
        return SS_EINVAL;
    if ((reinterpret_cast<size_t>(staged) & 7) || (staged_row_stride & 1) || (reinterpret_cast<size_t>(row_max) & 3)) return SS_EINVAL;
    for (const void* ptr : {static_cast<const void*>(staged), static_cast<const void*>(slots), static_cast<const void*>(lens),
                            static_cast<const void*>(row_max)})
        if (!device_accessible(ptr)) return SS_EINVAL;
    ssk::ScatterRows16MaxParams p;
    p.staged = staged; p.slots = slots; p.lens = lens; p.row_max = row_max; p.rir16 = static_cast<ssk::h16x2*>(rir16); p.rscale = rscale;
    p.bank_len = bank_len; p.staged_stride = staged_row_stride; p.cap = cap;
    for (int lo = 0; lo < n; lo += 65535) {                    // (grid.y limit)
        const int m = n - lo < 65535 ? n - lo : 65535;
        ssk::ScatterRows16MaxParams q = p;
        q.staged += static_cast<size_t>(lo) * staged_row_stride; q.slots += lo; q.lens += lo; q.row_max += 2 * static_cast<size_t>(lo);
        hipLaunchKernelGGL(ssk::k_scatter_rows16_max, dim3((cap + 511) / 512, m), dim3(256), 0, static_cast<hipStream_t>(stream), q);
    }
    return hip_err(hipGetLastError());
}
