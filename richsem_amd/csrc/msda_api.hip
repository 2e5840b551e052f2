// msda_api.hip -- the C ABI of librichsem_msda.so (declared in include/richsem_msda.h).
//
// Host side of the drop-in for the reference's ms_deform_attn_cuda_forward / _backward
// (reference models/richsem/ops/src/cuda/ms_deform_attn_cuda.cu:20-80, 83-153): argument checks,
// launch geometry, zero-fill of the accumulated output, kernel selection.  No torch types.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "msda_host.h"
#include "msda_direct.h"
#include "msda_levelsum.h"
#include "msda_roles.h"
#include "msda_prep.h"
#include "msda_band.h"
#include "msda_rps.h"
#include "msda_tiled.h"

namespace {
thread_local char g_err[512] = "";
}

// ---- the host layer of msda_host.h: every non-zero return of the library goes through one of these -----------------------------
namespace msda {

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int arg_fail(int code, const char *entry)
{
    const char *what = code == MSDA_ERR_NULL_POINTER ? "null pointer argument"
                     : code == MSDA_ERR_BAD_DIMS     ? "dimension out of the supported range (see include/richsem_msda.h)"
                     : code == MSDA_ERR_MISALIGNED   ? "pointer not aligned as required"
                     : code == MSDA_ERR_TOO_LARGE    ? "problem too large for 32-bit indexing"
                     : code == MSDA_ERR_NO_DEVICE    ? "no device to run on"
                     : code == MSDA_ERR_BAD_OPTION   ? "option value not among the accepted ones"
                                                     : "error";
    return fail(code, "%s: %s", entry, what);
}

int hip_fail(hipError_t e, const char *what, const char *tag)
{
    snprintf(g_err, sizeof(g_err), "%s%s: %s (hipError %d)", what, tag, hipGetErrorString(e), (int)e);
    return (int)e;
}

int launched(const char *what, const char *tag)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MSDA_OK : hip_fail(e, what, tag);
}

hipError_t set_lds_limit(const void *fn, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> granted;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = granted[std::make_pair(dev, fn)];
    if (have >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

}  // namespace msda

namespace {

using msda::aligned;
using msda::fail;
using msda::hip_fail;
using msda::launched;

struct Problem {
    int N, S, M, D, L, Lq, P;
    std::vector<int64_t> shapes, lsi;  // host mirrors
};

std::atomic<int> g_fwd_variant{0}, g_bwd_variant{0}, g_bwd_cpl{0}, g_levelsum{1}, g_fwd_prep_fused{1}, g_bwd_split{1}, g_bwd_dd_roles{1}, g_bwd_dd_roles_calls{0};

// The options a call's path depends on, read ONCE -- `Options{}` at the start of the exported call -- and passed down: a msda_set_option
// from another thread in the middle of a call cannot give a call that follows neither the old value nor the new.
struct Options {
    int fwd_variant = g_fwd_variant.load(), fwd_prep_fused = g_fwd_prep_fused.load(), bwd_variant = g_bwd_variant.load(), bwd_cpl = g_bwd_cpl.load(),
        levelsum = g_levelsum.load(), bwd_split = g_bwd_split.load(), bwd_dd_roles = g_bwd_dd_roles.load();
};

// ---- launch profiler: pre-created event pairs, one per logged call -----------------------------
struct ProfileSlot {
    hipEvent_t start, stop;
    msda_profile_record rec;
};
std::mutex g_prof_mutex;
std::vector<ProfileSlot> g_prof_slots;
int g_prof_used = 0;
std::atomic<bool> g_prof_on{false};
std::atomic<int> g_prof_filter{0};      // 0: every call is bracketed; else only calls of (kind + 1) * 16 + variant (option "profile_filter")

// RAII bracket around the main kernel launch of one call
struct ProfileScope {
    ProfileSlot *slot = nullptr;
    hipStream_t stream;
    ProfileScope(int kind, int variant, int dtype_bytes, const Problem &pb, hipStream_t st) : stream(st)
    {
        if (!g_prof_on.load(std::memory_order_relaxed)) return;
        // (an event pair is two more packets on the stream -- ~4 us of a call's time on MI355X: a caller that times a whole step brackets
        // only the kernel it wants the duration of)
        const int f = g_prof_filter.load(std::memory_order_relaxed);
        if (f && f != (kind + 1) * 16 + variant) return;
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        if (g_prof_used >= (int)g_prof_slots.size()) return;
        slot = &g_prof_slots[g_prof_used++];
        slot->rec = msda_profile_record{kind, variant, dtype_bytes, pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, 0.f};
        (void)hipEventRecord(slot->start, stream);
    }
    // the call turned out not to run this variant: give the slot back (only the newest slot can be returned)
    void cancel()
    {
        if (!slot) return;
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        if (g_prof_used > 0 && slot == &g_prof_slots[g_prof_used - 1]) --g_prof_used;
        else slot->rec.variant = -1;
        slot = nullptr;
    }
    ~ProfileScope()
    {
        if (slot) (void)hipEventRecord(slot->stop, stream);
    }
};

// ---- one path of a call: bracket it for the profiler, launch, map the error ------------------------------------------------------------
// launch() returns the hipError_t of its launches and hip_fail's words about it.  An ATTEMPT may answer hipErrorNotSupported -- its plan does
// not apply, or no workspace can be had right now --: the profile record is given back and the call goes on to the next path (kNextPath).
struct Launched {
    hipError_t e;
    const char *what = "", *tag = "";
};
constexpr int kNextPath = 1 << 30;
enum class Attempt { kNo, kRecordStaysOnError, kRecordBackOnError };
template <typename Launch>
int run_path(int kind, int prof_variant, int dtype_bytes, Attempt attempt, const Problem &pb, hipStream_t stream, Launch launch)
{
    ProfileScope prof(kind, prof_variant, dtype_bytes, pb, stream);
    const Launched l = launch();
    const bool refused = attempt != Attempt::kNo && l.e == hipErrorNotSupported;
    if (refused || (attempt == Attempt::kRecordBackOnError && l.e != hipSuccess)) prof.cancel();
    if (l.e == hipSuccess) return MSDA_OK;
    return refused ? kNextPath : hip_fail(l.e, l.what, l.tag);
}


// ---- locality monitor -----------------------------------------------------------------------------------
// The LDS-window FORWARD kernel wins only while most sampling points fall into the window of their query's region; the share
// that does not ("general share") is a property of the DATA (how far the network's offsets reach).  Measured on MI355X
// (tools/locality_sweep2.sh, call E; profiles/r02_locality.md): the window forward -- which finishes the points that miss
// their window per point, after the item -- beats the direct forward up to a share of ~8 % (sigma ~4.5 px).  In automatic mode
// the library therefore lets the window forward kernel count its general points now and then (one atomic per wave), brings the
// count back with an asynchronous copy + event on the caller's stream, and reads it on a LATER call once the event has completed
// -- no call ever waits.  Nothing is probed while the stream is being captured into a graph.  (The backward needs no monitor: the
// routed kernels of msda_rps.h cost the same wherever the points fall.)
constexpr float kFwdShareMax = 0.08f;
constexpr unsigned kProbeWarmCalls = 2, kProbeEvery = 64;   // per (shape, sampling_loc buffer)
constexpr int kMaxDevices = 64;
std::atomic<int> g_monitor_on{1};
std::atomic<int> g_last_share_ppm{-1};

struct MonitorEntry {
    unsigned calls = 0, next_probe = 0, probes = 0;
    float share = 0.f;
    bool known = false;
};
constexpr int kProbeSlots = 8;   // probes in flight at once (the layers of a step call back to back)
struct ProbeSlot {
    hipEvent_t done = nullptr;
    bool pending = false;
    uint64_t key = 0;
    double points = 0;
};
struct Monitor {
    std::mutex mu;
    unsigned *dev = nullptr, *host = nullptr;   // kProbeSlots counters on the device, their pinned host copies
    ProbeSlot slot[kProbeSlots];
    int held = -1;                               // slot of the probe being launched (between choose_fwd and finish_probe)
    std::unordered_map<uint64_t, MonitorEntry> table;
};
Monitor g_monitors[kMaxDevices];

// What a verdict is keyed by: the problem's shape AND the sampling_loc buffer.  How far the offsets reach is a property of a
// LAYER's weights; the layers of a network call with the same shapes but each with its own sampling_loc tensor, which a
// steady-state training step finds at the same address every time (caching allocator) -- and the backward call of a layer
// is handed the very tensor its forward call saw.  A pointer never seen before simply starts a new entry.
uint64_t problem_key(const int N, const int S, const int M, const int L, const int P, const int64_t *shapes, const void *loc = nullptr)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix(N); mix(S); mix(M); mix(L); mix(P);
    for (int l = 0; l < 2 * L; ++l) mix((uint64_t)shapes[l]);
    mix((uint64_t)reinterpret_cast<uintptr_t>(loc));
    return h;
}
constexpr size_t kMonitorMaxEntries = 512;   // (sampling_loc addresses that keep changing: forget and start over)

// under mo.mu: fold the finished probes into their entries
void monitor_poll(Monitor &mo)
{
    for (int i = 0; i < kProbeSlots; ++i) {
        ProbeSlot &ps = mo.slot[i];
        if (!ps.pending || hipEventQuery(ps.done) != hipSuccess) continue;
        ps.pending = false;
        MonitorEntry &en = mo.table[ps.key];
        const float s = (float)((double)mo.host[i] / ps.points);
        // the warm-up probes of a key keep their worst; later ones track slowly
        en.share = !en.known ? s : (en.probes <= kProbeWarmCalls ? (s > en.share ? s : en.share) : 0.5f * (en.share + s));
        en.known = true;
        g_last_share_ppm = (int)(s * 1e6f);
    }
}

Monitor *monitor_for_current_device()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
    return &g_monitors[dev];
}

bool capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    return cap != hipStreamCaptureStatusNone;
}

// Forward, automatic mode, window kernels applicable.  Returns the variant to run (1 direct, 2 window) and, through
// *probe, the device counter the window kernel should add its general points to (or null).  With *probe set the caller
// MUST call monitor_finish_probe after its launch.  The monitor's mutex is held from here to monitor_finish_probe.
int monitor_choose_fwd(Monitor *mo, uint64_t key, hipStream_t stream, unsigned **probe)
{
    *probe = nullptr;
    if (!mo || !g_monitor_on.load()) return 2;
    const bool in_capture = capturing(stream);
    mo->mu.lock();
    if (!in_capture) monitor_poll(*mo);   // (querying an event is not allowed while a capture is under way)
    if (mo->table.size() > kMonitorMaxEntries) mo->table.clear();
    MonitorEntry &en = mo->table[key];
    const unsigned call = en.calls++;
    int free_slot = -1;
    bool mine_in_flight = false;
    for (int i = 0; i < kProbeSlots; ++i) {
        if (!mo->slot[i].pending && free_slot < 0) free_slot = i;
        mine_in_flight = mine_in_flight || (mo->slot[i].pending && mo->slot[i].key == key);
    }
    bool want = free_slot >= 0 && !mine_in_flight && !in_capture && call >= en.next_probe;
    if (want && !mo->dev) {   // first probe on this device
        bool ok = hipMalloc(reinterpret_cast<void **>(&mo->dev), kProbeSlots * sizeof(unsigned)) == hipSuccess &&
                  hipHostMalloc(reinterpret_cast<void **>(&mo->host), kProbeSlots * sizeof(unsigned), hipHostMallocDefault) == hipSuccess;
        for (int i = 0; ok && i < kProbeSlots; ++i) ok = hipEventCreateWithFlags(&mo->slot[i].done, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            mo->dev = nullptr;
            want = false;
        }
    }
    if (want && hipMemsetAsync(mo->dev + free_slot, 0, sizeof(unsigned), stream) != hipSuccess) want = false;
    if (want) {
        *probe = mo->dev + free_slot;
        en.next_probe = call + (en.probes < kProbeWarmCalls ? 1 : kProbeEvery);
        ++en.probes;
        mo->slot[free_slot].key = key;
        mo->held = free_slot;
        return 2;   // a probe IS a window-kernel call; the lock stays held
    }
    const int variant = en.known && en.share > kFwdShareMax ? 1 : 2;
    mo->mu.unlock();
    return variant;
}

void monitor_finish_probe(Monitor *mo, double points, hipStream_t stream, bool launched)
{
    const int i = mo->held;
    mo->held = -1;
    if (i >= 0 && launched &&
        hipMemcpyAsync(mo->host + i, mo->dev + i, sizeof(unsigned), hipMemcpyDeviceToHost, stream) == hipSuccess &&
        hipEventRecord(mo->slot[i].done, stream) == hipSuccess) {
        mo->slot[i].pending = true;
        mo->slot[i].points = points;
    }
    mo->mu.unlock();
}

// The forward variant a call runs where a window kernel applies: what was asked for, or in automatic mode (0) the monitor's choice
// together with the probe the window kernel is to count into.
struct FwdChoice {
    int variant;
    Monitor *mo = nullptr;
    unsigned *probe = nullptr;
};
FwdChoice choose_window_fwd(int asked, const Problem &pb, const void *loc, hipStream_t stream)
{
    FwdChoice ch{asked};
    if (asked == 0) {
        ch.mo = monitor_for_current_device();
        ch.variant = monitor_choose_fwd(ch.mo, problem_key(pb.N, pb.S, pb.M, pb.L, pb.P, pb.shapes.data(), loc), stream, &ch.probe);
    }
    return ch;
}

// Argument checks shared by forward and backward.  Mirrors the reference's preconditions
// (ms_deform_attn_cuda.cu:28-52) and adds the bounds the kernels rely on.
int check_problem(Problem &pb, const int64_t *shapes_dev, const int64_t *lsi_dev, const int64_t *shapes_host,
                  const int64_t *lsi_host, int im2col_step, hipStream_t stream)
{
    if (pb.N <= 0 || pb.S <= 0 || pb.M <= 0 || pb.D <= 0 || pb.L <= 0 || pb.Lq <= 0 || pb.P <= 0)
        return fail(MSDA_ERR_BAD_DIMS, "non-positive dimension (N=%d S=%d M=%d D=%d L=%d Lq=%d P=%d)", pb.N, pb.S,
                    pb.M, pb.D, pb.L, pb.Lq, pb.P);
    if (im2col_step <= 0) return fail(MSDA_ERR_IM2COL_STEP, "im2col_step(%d) must be positive", im2col_step);
    const int step = pb.N < im2col_step ? pb.N : im2col_step;
    if (pb.N % step != 0) return fail(MSDA_ERR_IM2COL_STEP, "batch(%d) must divide im2col_step(%d)", pb.N, step);

    const int64_t lim = (int64_t)1 << 31;
    const int64_t n_value = (int64_t)pb.N * pb.S * pb.M * pb.D;
    const int64_t n_out = (int64_t)pb.N * pb.Lq * pb.M * pb.D;
    const int64_t n_loc = (int64_t)pb.N * pb.Lq * pb.M * pb.L * pb.P * 2;
    if (n_value >= lim || n_out >= lim || n_loc >= lim)
        return fail(MSDA_ERR_TOO_LARGE, "tensor with >= 2^31 elements (value %lld, out %lld, loc %lld)",
                    (long long)n_value, (long long)n_out, (long long)n_loc);

    pb.shapes.resize(2 * (size_t)pb.L);
    pb.lsi.resize((size_t)pb.L);
    if (shapes_host && lsi_host) {
        memcpy(pb.shapes.data(), shapes_host, sizeof(int64_t) * 2 * pb.L);
        memcpy(pb.lsi.data(), lsi_host, sizeof(int64_t) * pb.L);
    } else {  // slow path: synchronises the stream
        hipError_t e = hipMemcpyAsync(pb.shapes.data(), shapes_dev, sizeof(int64_t) * 2 * pb.L, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pb.lsi.data(), lsi_dev, sizeof(int64_t) * pb.L, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "copying spatial_shapes / level_start_index to the host");
    }
    int64_t total = 0;
    for (int l = 0; l < pb.L; ++l) {
        const int64_t H = pb.shapes[2 * l], W = pb.shapes[2 * l + 1], st = pb.lsi[l];
        if (H <= 0 || W <= 0 || H >= lim || W >= lim || H * W > pb.S)
            return fail(MSDA_ERR_BAD_DIMS, "level %d: bad spatial shape (%lld, %lld)", l, (long long)H, (long long)W);
        if (st < 0 || st + H * W > pb.S)
            return fail(MSDA_ERR_BAD_DIMS, "level %d: level_start_index %lld + %lld*%lld exceeds S=%d", l, (long long)st,
                        (long long)H, (long long)W, pb.S);
        total += H * W;
    }
    if (total != pb.S)
        return fail(MSDA_ERR_BAD_DIMS, "sum of H*W over levels (%lld) != S (%d)", (long long)total, pb.S);
    return MSDA_OK;
}

// The checked problem of ONE exported call: msda_forward_*, msda_backward_* and msda_forward_prep_* each run this exactly once per call; nothing
// else calls check_problem.  Error text reset, null pointers (`non_null`), check_problem, alignment (`ptrs_aligned`; `misaligned`: its refusal).
struct LevelTables { const int64_t *shapes, *lsi, *shapes_host, *lsi_host; };
int misaligned_fail(const char *which) { return fail(MSDA_ERR_MISALIGNED, "misaligned pointer (%s)", which); }
int checked_problem(Problem &pb, bool non_null, const LevelTables &lt, int im2col_step, hipStream_t stream, bool ptrs_aligned,
                    const char *misaligned)
{
    g_err[0] = 0;
    if (!non_null) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (int rc = check_problem(pb, lt.shapes, lt.lsi, lt.shapes_host, lt.lsi_host, im2col_step, stream)) return rc;
    return ptrs_aligned ? MSDA_OK : misaligned_fail(misaligned);
}

int floor_log2(int x)
{
    int r = 0;
    while ((1 << (r + 1)) <= x) ++r;
    return r;
}

// Channels per lane for the direct kernels: the widest access of at most max_channels elements of TV that D and every data
// pointer allow.
template <typename TV>
int pick_channels(int D, int max_channels, std::initializer_list<const void *> ptrs)
{
    int c = max_channels;
    for (; c > 1; c >>= 1) {
        if (D % c == 0 && aligned(sizeof(TV) * c, ptrs)) break;
    }
    return c;
}
// the direct kernels' widest: 16 B of f32 / f64, four channels (8 B) of bf16
template <typename TV>
constexpr int kMaxChannels = sizeof(TV) == 8 ? 2 : 4;

msda::DirectGeom direct_geom(const Problem &pb, int C)
{
    msda::DirectGeom g{};
    g.N = pb.N; g.S = pb.S; g.M = pb.M; g.D = pb.D; g.L = pb.L; g.Lq = pb.Lq; g.P = pb.P;
    const int lanes = (pb.D + C - 1) / C;
    int G = msda::kMinGroup;
    while (G < lanes && G < msda::kWave) G <<= 1;
    g.G = G;
    g.logG = floor_log2(G);
    g.nchunks = (lanes + G - 1) / G;
    // queries per block: whole passes of the block's lane groups; few passes when Lq is small (decoder calls) so that
    // the grid still fills 256 CUs several times over, more passes (amortising the level table) when Lq is large
    const int per_iter = msda::kDirectWaves * (msda::kWave / G);
    const int slots = msda::kXcds * ((pb.N * pb.M + msda::kXcds - 1) / msda::kXcds);
    const int want_tiles = (4096 + slots - 1) / slots;
    int passes = pb.Lq / (per_iter * want_tiles);
    passes = passes < 1 ? 1 : (passes > 8 ? 8 : passes);
    g.qtile = per_iter * passes;
    g.ntiles = (pb.Lq + g.qtile - 1) / g.qtile;
    const int LP = pb.L * pb.P;
    g.pbatch = LP < msda::kPointBatch ? LP : msda::kPointBatch;
    return g;
}

int direct_grid(const msda::DirectGeom &g)
{
    const int pairs = g.N * g.M;
    return msda::kXcds * ((pairs + msda::kXcds - 1) / msda::kXcds) * g.ntiles;
}

// bit mask of all L levels
inline unsigned all_levels_mask(int L) { return L >= 32 ? ~0u : (1u << L) - 1; }

// do the levels tile [0, S) in order, without gap or overlap?  (check_problem only bounds them)
bool levels_tile(const Problem &pb)
{
    bool tile = true;
    for (int64_t l = 0, pre = 0; l < pb.L; ++l) {
        tile = tile && pb.lsi[l] == pre;
        pre += pb.shapes[2 * l] * pb.shapes[2 * l + 1];
    }
    return tile;
}

// The direct kernels (msda_direct.h) are instantiated with 1, 2 and -- for 4-byte compute types -- 4 channels per lane: calls
// launch(std::integral_constant<int, CC>) for the C picked (pick_channels never gives an 8-byte type more than 2).
template <typename T, typename Launch>
void with_channels(int C, Launch launch)
{
    switch (C) {
        case 4: launch(std::integral_constant<int, (sizeof(T) == 4 ? 4 : 2)>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        default: launch(std::integral_constant<int, 1>{}); break;
    }
}

// large calls: more waves per SIMD, shallower per-wave pipeline (see fwd_direct_kernel)
inline bool many_items(const Problem &pb) { return (int64_t)pb.N * pb.Lq * pb.M >= 65536; }

// ---- library-owned device memory, per (device, stream): calls on one stream are ordered, so they can share it; calls on
// different streams cannot.  Nothing is allocated while the stream is being captured.
struct Workspace {
    float *gv32 = nullptr;   // bf16 backward: fp32 accumulation buffer for grad_value (rounded to bf16 once)
    size_t gv32_cap = 0;
    unsigned *rps_bins = nullptr;            // routed backward: queue heads (32 words), then one 64-bit (records | runs) counter per
    size_t rps_bins_n = 0;                   // bin on a 128-byte line of its own (rps_bins_words); capacity in bins
    uint2 *rps_runs = nullptr;               // [cap] the bins' run tables (nbins x max_runs)
    size_t rps_runs_cap = 0;
    msda::RpsRec *rps_entries = nullptr;     // [cap] routed records
    size_t rps_entries_cap = 0;
    bool rps_dirty = false;                  // a failed launch may have left the bin counters non-zero
    // Buffers outgrown by a later, larger call are RETIRED, not freed: a HIP graph captured earlier on this stream holds their raw
    // addresses (kernel arguments), and a replay after a hipFree would read and write freed memory.  They live until the process ends;
    // growth is geometric (x 1.5), so the retired total stays below twice the live size.
    std::vector<void *> retired;
    void retire(void *p) { if (p) retired.push_back(p); }
};
std::mutex g_ws_mu;
std::map<std::pair<int, hipStream_t>, Workspace> g_ws;

// Under g_ws_mu, the one place a workspace is allocated: make `ptr` a buffer of `need` elements of `elem_bytes` (+ `extra_bytes` behind them)
// at least.  Nothing while the stream is being captured, the old buffer retired, the new one half as large again as needed (+ `pad`
// elements).  false, with the runtime's error cleared, when there is no buffer to be had: the caller falls back or refuses.
template <typename E>
bool grow_buffer(Workspace &ws, hipStream_t stream, E *&ptr, size_t &cap, size_t need, size_t pad, size_t elem_bytes, size_t extra_bytes = 0)
{
    if (cap >= need) return true;
    if (capturing(stream)) return false;
    ws.retire(ptr);
    ptr = nullptr;
    cap = 0;
    const size_t want = need + need / 2 + pad;
    if (hipMalloc(reinterpret_cast<void **>(&ptr), want * elem_bytes + extra_bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    cap = want;
    return true;
}

int g_cu_count[kMaxDevices] = {0};

int cu_count()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    if (!g_cu_count[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        g_cu_count[dev] = n;
    }
    return g_cu_count[dev];
}

// ---- routed pixel-stationary backward (msda_rps.h) ---------------------------------------------------------------------------
// The bin counters are zero between calls (the tile kernel zeroes a bin's counter when it has consumed the bin), so that no call has to clear
// them first: they are cleared when allocated and after a launch error.
struct RpsBuffers { unsigned *bins; uint2 *runs; msda::RpsRec *entries; size_t entries_cap; };
constexpr size_t rps_bins_words(size_t n_bins) { return 32 + (size_t)msda::kRpsPad * n_bins + 8; }

bool rps_workspace(hipStream_t stream, size_t n_bins, size_t n_runs, size_t n_entries, RpsBuffers &out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(g_ws_mu);
    Workspace &ws = g_ws[std::make_pair(dev, stream)];
    // in this order: allocate -> mark dirty -> clear
    if (ws.rps_bins_n < n_bins) {
        if (!grow_buffer(ws, stream, ws.rps_bins, ws.rps_bins_n, n_bins, 64, msda::kRpsPad * sizeof(unsigned), rps_bins_words(0) * sizeof(unsigned)))
            return false;
        ws.rps_dirty = true;
    }
    if (ws.rps_dirty) {
        if (capturing(stream)) return false;      // (a call being captured neither allocates nor clears)
        if (hipMemsetAsync(ws.rps_bins, 0, rps_bins_words(ws.rps_bins_n) * sizeof(unsigned), stream) != hipSuccess) { (void)hipGetLastError(); return false; }
        ws.rps_dirty = false;
    }
    if (!grow_buffer(ws, stream, ws.rps_runs, ws.rps_runs_cap, n_runs, 1024, sizeof(uint2))) return false;
    if (!grow_buffer(ws, stream, ws.rps_entries, ws.rps_entries_cap, n_entries, 0, sizeof(msda::RpsRec), msda::kRpsDummyBytes)) return false;      // (+ the tile kernel's scratch lines)
    out = RpsBuffers{ws.rps_bins, ws.rps_runs, ws.rps_entries, ws.rps_entries_cap};
    return true;
}

void rps_mark_dirty(hipStream_t stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> lock(g_ws_mu);
    g_ws[std::make_pair(dev, stream)].rps_dirty = true;
}

// returns hipErrorNotSupported when the plan does not apply or no workspace can be had right now.
// TV = bf16_t: grad_acc is an fp32 image of grad_value for the levels accumulated with atomics (rounded at the end).
template <typename TV>
hipError_t launch_bwd_rps(const Problem &pb, const TV *value, const float *loc, const float *aw, const TV *grad_out,
                          TV *grad_value, float *grad_acc, float *grad_loc, float *grad_aw, hipStream_t stream)
{
    msda::RpsPlan pl = msda::plan_rps(pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data());
    if (!pl.ok) return hipErrorNotSupported;
    // rows: 16 B (fp32) / 8 B (bf16) per lane access
    if (!aligned(sizeof(TV) * 4, {value, grad_out, grad_value}) || !aligned(16, {grad_acc}) || !aligned(8, {grad_loc, loc})) return hipErrorNotSupported;
    if ((int64_t)pb.N * pb.Lq * pb.M * msda::kRpsD * (int64_t)sizeof(TV) > (int64_t)0xFFFFFFFF) return hipErrorNotSupported;      // (the tile kernel addresses grad_out rows by 32-bit byte offsets)
    RpsBuffers ws;
    const size_t n_runs = (size_t)pl.g.nbins * (size_t)pl.g.max_runs;
    if (n_runs * sizeof(uint2) > ((size_t)256 << 20)) return hipErrorNotSupported;      // (run tables of a quarter GB: not a shape this path is for)
    if (!rps_workspace(stream, (size_t)pl.g.nbins, n_runs, pl.max_entries, ws)) return hipErrorNotSupported;
    pl.g.ctr = ws.bins;
    pl.g.bin_state = reinterpret_cast<unsigned long long *>(ws.bins + 32);   // (line-aligned; one per 128-B line)
    pl.g.runs = ws.runs;
    pl.g.entries_cap = (unsigned)std::min<size_t>(ws.entries_cap, 0xFFFFFFFFu);
    pl.g.entries = ws.entries;
    pl.g.dummy = reinterpret_cast<float *>(ws.entries + ws.entries_cap);
    pl.g.stamps = msda::tiled_options().stamps;
    auto kern = pl.g.stamps ? (pb.P == 4 ? &msda::rps_tile_kernel<true, TV, true> : &msda::rps_tile_kernel<false, TV, true>)
                            : (pb.P == 4 ? &msda::rps_tile_kernel<true, TV> : &msda::rps_tile_kernel<false, TV>);
    hipError_t e = msda::set_lds_limit(reinterpret_cast<const void *>(kern), sizeof(msda::RpsLds));
    if (e != hipSuccess) return e;
    // route passes: a workgroup (8 waves; 16 where the plan asks for them) per block of queries of an (image, head)
    const int qpw = pb.P <= 4 ? 16 : (pb.P <= 8 ? 8 : (pb.P <= 16 ? 4 : (pb.P <= 32 ? 2 : 1)));
    const int qpb = qpw * (pl.g.route_threads / msda::kWave);
    const int64_t r_items = (int64_t)pb.N * pb.M * ((pb.Lq + qpb - 1) / qpb);
    const int route_wgs = pl.g.route_threads > 512 ? 1 : msda::rps_options().route_wgs.load();      // (16 waves at 102 registers: one workgroup per CU)
    const int rgrid = (int)std::max<int64_t>(1, std::min<int64_t>(r_items, (int64_t)route_wgs * cu_count()));
    {
        // (the reference's models all have L = P = 4: that instance has both as compile-time constants; the stage stamps live in an
        // instance of their own)
        using RouteFn = void (*)(const float *, const float *, float *, float *, float *, const msda::RpsGeom);
        const bool big = pl.g.route_threads > 512, lp4 = pb.L == 4 && pb.P == 4;
        RouteFn route;
        if (pl.g.stamps)
            route = big ? &msda::rps_route_kernel<msda::kRpsRouteThreadsMax, 0, 0, true>
                        : (lp4 ? &msda::rps_route_kernel<512, 4, 4, true> : &msda::rps_route_kernel<512, 0, 0, true>);
        else if (lp4)
            route = big ? &msda::rps_route_kernel<msda::kRpsRouteThreadsMax, 4, 4> : &msda::rps_route_kernel<512, 4, 4>;
        else
            route = big ? &msda::rps_route_kernel<msda::kRpsRouteThreadsMax> : &msda::rps_route_kernel<512>;
        hipLaunchKernelGGL(route, dim3(rgrid), dim3(pl.g.route_threads), (size_t)pl.g.lut_n * sizeof(unsigned), stream, loc, aw, grad_acc,
                           grad_loc, grad_aw, pl.g);
    }
    const int grid = (cu_count() / msda::kXcds) * msda::kXcds;   // persistent: one workgroup per CU (its LDS is most of a CU's)
    hipLaunchKernelGGL(kern, dim3(grid > 0 ? grid : 8), dim3(msda::kRpsThreads), sizeof(msda::RpsLds), stream, value, grad_out,
                       grad_value, grad_acc, grad_loc, grad_aw, pl.g);
    if constexpr (!std::is_same<TV, float>::value)      // (every level has rows in the fp32 image: the tiles' shared first rows / columns at least)
        hipLaunchKernelGGL(msda::rps_round_kernel, dim3(256), dim3(256), 0, stream, grad_acc, grad_value, pl.g);
    e = hipGetLastError();
    if (e != hipSuccess) rps_mark_dirty(stream);
    return e;
}

// ---- row-band backward (msda_band.h): decoder-shaped calls, D = 32, one launch ------------------------------------------------------
// returns hipErrorNotSupported when the plan does not apply.  TV = bf16_t: grad_acc is an fp32 image of grad_value for the slabbed levels.
template <typename TV>
hipError_t launch_bwd_band(const Problem &pb, const TV *value, const float *loc, const float *aw, const TV *grad_out, TV *grad_value,
                           float *grad_acc, float *grad_loc, float *grad_aw, hipStream_t stream)
{
    msda::BandPlan pl = msda::plan_band(pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data());
    if (!pl.ok) return hipErrorNotSupported;
    pl.g.stamps = msda::tiled_options().stamps;
    // rows: 16 B (fp32) / 8 B (bf16) per lane access
    if (!aligned(8, {grad_loc, loc}) || !aligned(sizeof(TV) * 4, {value, grad_out, grad_value}) || !aligned(16, {grad_acc})) return hipErrorNotSupported;
    if (pl.atomic_levels && !grad_acc) return hipErrorNotSupported;
    hipError_t e;
    if (pl.atomic_levels)      // the levels several workgroups add to: zero in every image
        hipLaunchKernelGGL(msda::band_zero_kernel, dim3(128), dim3(256), 0, stream, grad_acc, pl.g, pl.atomic_levels);
    auto kern = &msda::bwd_band_kernel<TV>;
    e = msda::set_lds_limit(reinterpret_cast<const void *>(kern), pl.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(msda::band_grid(pl.g)), dim3(msda::kBandThreads), pl.lds_bytes, stream, value, loc, aw, grad_out, grad_value,
                       grad_acc, grad_loc, grad_aw, pl.g);
    if constexpr (!std::is_same<TV, float>::value) {
        if (pl.atomic_levels) hipLaunchKernelGGL(msda::band_round_kernel, dim3(256), dim3(256), 0, stream, grad_acc, grad_value, pl.g, pl.atomic_levels);
    }
    return hipGetLastError();
}

// The split kernels (msda_direct.h: fwd_split_kernel / bwd_split_kernel) apply at D = 32 with 16-byte (fp32) / 8-byte (bf16) rows, L*P a
// multiple of 4 up to 32; they are the automatic choice for calls of fewer than 65536 (query, head) items.
inline bool split_fits(const Problem &pb, int C) { return pb.D == 32 && C == 4 && (pb.L * pb.P) % msda::kSplitGroups == 0 && pb.L * pb.P / msda::kSplitGroups <= msda::kSplitMaxPts; }
inline bool split_small(const Problem &pb) { return (int64_t)pb.N * pb.Lq * pb.M < 65536; }
inline dim3 split_grid(const Problem &pb) { return dim3((unsigned)(((int64_t)pb.N * pb.Lq * pb.M * 32 + msda::kDirectThreads - 1) / msda::kDirectThreads)); }

template <typename TV>
hipError_t launch_fwd_split(const Problem &pb, const TV *value, const int64_t *shapes, const int64_t *lsi, const float *loc, const float *aw,
                            TV *out, const msda::DirectGeom &g, hipStream_t stream)
{
    const size_t lds = sizeof(msda::LevelGeom) * pb.L;
    auto kern = pb.L * pb.P == 16 ? &msda::fwd_split_kernel<TV, 4> : &msda::fwd_split_kernel<TV, 0>;
    hipLaunchKernelGGL(kern, split_grid(pb), dim3(msda::kDirectThreads), lds, stream, value, shapes, lsi, loc, aw, out, g);
    return hipGetLastError();
}

template <typename TV>
hipError_t launch_bwd_split(const Problem &pb, const TV *value, const int64_t *shapes, const int64_t *lsi, const float *loc, const float *aw,
                            const TV *grad_out, float *grad_loc, float *grad_aw, const msda::DirectGeom &g, hipStream_t stream)
{
    const size_t lds = sizeof(msda::LevelGeom) * pb.L;
    auto kern = pb.L * pb.P == 16 ? &msda::bwd_split_kernel<TV, 4> : &msda::bwd_split_kernel<TV, 0>;
    hipLaunchKernelGGL(kern, split_grid(pb), dim3(msda::kDirectThreads), lds, stream, value, shapes, lsi, loc, aw, grad_out, grad_loc, grad_aw, g);
    return hipGetLastError();
}

// ---- level-sum and split workgroups in one launch (msda_roles.h): decoder-shaped calls, fp32 storage, P = 4 ----------------------------
// returns hipErrorNotSupported when windows of this launch's size cannot take every level (the call then takes two launches).
hipError_t launch_bwd_dd_roles(const Problem &pb, const float *value, const int64_t *shapes, const int64_t *lsi, const float *loc,
                               const float *aw, const float *grad_out, float *grad_value, float *grad_loc, float *grad_aw,
                               const msda::DirectGeom &g, hipStream_t stream)
{
    msda::LevelSumGeom lg;
    size_t window = 0;
    if (msda::plan_levelsum(pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data(), lg, window, msda::kDdRolesLdsKb) !=
        all_levels_mask(pb.L))
        return hipErrorNotSupported;
    const msda::DdRoles r = msda::plan_dd_roles<msda::kDdRolesThreads>((int64_t)pb.N * pb.Lq * pb.M);
    const uint64_t grid = (uint64_t)r.sp_first + (uint64_t)msda::levelsum_grid(lg);
    if (grid > 0x7fffffffu) return hipErrorNotSupported;
    const size_t lds = msda::dd_roles_lds_bytes(pb.L, window);
    auto kern = &msda::bwd_dd_roles_kernel<float, msda::kDdRolesThreads>;
    hipError_t e = msda::set_lds_limit(reinterpret_cast<const void *>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(msda::kDdRolesThreads), lds, stream, value, shapes, lsi, loc, aw, grad_out, grad_value,
                       grad_loc, grad_aw, lg, g, r);
    return hipGetLastError();
}

// ---- level-sum backward (msda_levelsum.h): grad_value of the levels of `lg`, summed in LDS windows -----------------------------------------
// *at_lds_limit: the error returned is the refusal of the kernel's LDS size, not of its launch
template <typename TV>
hipError_t launch_bwd_levelsum(const Problem &pb, const float *loc, const float *aw, const TV *grad_out, TV *grad_value,
                               const msda::LevelSumGeom &lg, size_t lds, hipStream_t stream, bool *at_lds_limit)
{
    // the P4 form loads a level's four locations / weights as 16-B vectors: only for 16-B aligned tensors (the ABI asks
    // for element alignment only)
    const bool vec = pb.P == 4 && aligned(16, {loc, aw});
    auto kern = vec ? &msda::bwd_levelsum_kernel<true, TV> : &msda::bwd_levelsum_kernel<false, TV>;
    const hipError_t e = msda::set_lds_limit(reinterpret_cast<const void *>(kern), lds);
    *at_lds_limit = e != hipSuccess;
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(msda::levelsum_grid(lg)), dim3(msda::kLsThreads), lds, stream, loc, aw, grad_out, grad_value, lg);
    return hipGetLastError();
}

// ---- bf16 storage (value / out / grad_out / grad_value), fp32 compute: the fp32 scratch image of grad_value and its one rounding -------
bool bf16_scratch(hipStream_t stream, size_t n_floats, float **out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(g_ws_mu);
    Workspace &ws = g_ws[std::make_pair(dev, stream)];
    if (!grow_buffer(ws, stream, ws.gv32, ws.gv32_cap, n_floats, 0, sizeof(float))) return false;
    *out = ws.gv32;
    return true;
}

// What atomics add grad_value into: grad_value itself, or for bf16 storage the library's fp32 scratch -- null until a path asks (have()).
template <typename T, typename TV>
struct GradAcc {
    T *ptr = nullptr;
    size_t n_value;
    hipStream_t stream;
    GradAcc(TV *grad_value, size_t n, hipStream_t st) : n_value(n), stream(st) { if constexpr (std::is_same<T, TV>::value) ptr = grad_value; }
    bool have() { if constexpr (std::is_same<T, TV>::value) return true; else return bf16_scratch(stream, n_value, &ptr); }
};

// n4 vectors of four elements (dst 8-byte aligned), then the n - 4*n4 elements of the tail one by one
__global__ __launch_bounds__(256) void round_to_bf16_kernel(const float *__restrict__ src, msda::bf16_t *__restrict__ dst, size_t n4,
                                                             size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
        msda::st4(dst + 4 * i, *reinterpret_cast<const float4 *>(src + 4 * i));
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = msda::to_storage<msda::bf16_t, float>(src[i]);
}

// ---- kernel selection: msda_forward_* / msda_backward_* ------------------------------------------------------------------------------
// forward_impl / backward_impl serve every element type: T is the type of sampling_loc / attn_weight and their gradients (float or
// double), TV the storage type of value / out / grad_out / grad_value (T, or msda::bf16_t beside T = float -- a capability the reference
// does not have: it dispatches float / double only, ms_deform_attn_cuda.cu:64,134; every sum is formed in fp32 or f64 LDS windows and
// rounded to bf16 once).  The order in which the paths are tried is the same for all; what differs between the instances is listed
// here and marked kBf16 / is_same<T, float> below.  Each line is today's behaviour; whether it is wanted is a question of its own.
//
//                                     f32 / f64 storage                             bf16 storage
//   pointer alignment demanded        sizeof(T); 2*sizeof(T) for loc / grad_loc     the same rule: 2 B data, 4 B weights, 8 B loc / grad_loc
//   window forward eligible           f32 only; value, out 16-B aligned; plan ok    value, out 8-B aligned; plan ok  (both: rows of four)
//   channels per lane                 widest <= 16 B that D and the pointers allow  widest <= 4 channels (8 B)
//   split forward / backward          f32 only                                      yes
//   "too many levels" (forward)       checked after the split kernel was considered before it  (a call the split kernel takes has L <= 32)
//   routed / band backward entered    bwd_variant 4, or 0 with Lq == S (band: 5);   the same variants, and only with value / grad_out / grad_value
//                                     f32 only                                      8-B aligned, D = 32 and the fp32 scratch to be had (band: a
//                                                                                   scratch only if its plan has atomic levels)
//   ... a launch error there          the profile record is given back              the profile record stays
//   level-sum backward                f32: any subset of levels, the rest by        only when it takes ALL levels; else fp32 scratch + zero-fill +
//                                     atomics after a zero-fill of grad_value;      direct kernel + one rounding pass
//   level-sum + split in one launch   yes (bwd_dd_roles; P = 4, loc / aw 16-B aligned)  no: two launches (not measured there)
//   bwd_direct_cpl option             honoured                                      ignored
//   direct backward adds grad_value   into grad_value                               into the fp32 scratch (null when level-sum took everything)
//   no scratch during stream capture  n/a                                           MSDA_ERR_BAD_DIMS
//   error texts                       as written                                    the runtime's (HIP) errors + " (bf16)", "LDS limit"; "... needs 8
//                                                                                   bytes"; the refusals ("too many levels", no scratch) untagged
//
// msda_forward_prep_* (locations computed from the projection: PrepLoc below) against msda_forward_* (locations given: GivenLoc), all types:
//   one launch, decoder-shaped        the call's own alignment set (+ ref, offsets, logits); its misalignment text says "2*sizeof(T)" and its
//   (fwd_prep_fused >= 1)             launch error carries no " (bf16)" for bf16 too; no split forward; profile variant 5
//   window kernel, encoder-shaped     fp32 compute, P = 4, fwd_variant != 1: the problem is checked BEFORE the location / softmax kernel's
//   (fwd_prep_fused = 2)              own checks (otherwise after them, and after its launch); the fused window kernel (profile variant 6)
//                                     asks for its rows (value / out rows of four, offsets in pairs, ref / loc 8 B) and the plan only: the
//                                     alignment set of msda_forward_* (the level tables' 8 B too) comes after it and the location / softmax launch
//   ... the monitor chose direct      location / softmax kernel, then the 8-lane direct kernel (variant 1) with the choice held; a forced
//       or fwd_variant = 3            fwd_variant 3 ends there too where the window kernel applies: it is not the split kernel on this path
int too_many_levels(int L) { return fail(MSDA_ERR_BAD_DIMS, "too many levels (L=%d) for the level table in LDS", L); }

// Where a forward call's sampling locations and attention weights come from, and with that all that differs between msda_forward_* and the
// one-launch forms of msda_forward_prep_*: kernel templates, profile variants, alignment sets, error texts.  GivenLoc: the caller's tensors.
template <typename T, typename TV>
struct GivenLoc {
    static constexpr bool kBf16 = std::is_same<TV, msda::bf16_t>::value, kSplit = true;      // (the split forward is tried on this path only)
    static constexpr int kDirectVariant = 1, kWindowVariant = 2;
    static constexpr const char *kDirectWhat = "launch of the direct forward kernel", *kWindowWhat = "launch of the tiled forward kernel";
    static constexpr const char *kTag = kBf16 ? " (bf16)" : "", *kMisaligned = kBf16 ? "sampling_loc needs 8 bytes" : "sampling_loc needs 2*sizeof(T)";
    const T *loc, *aw;
    bool call_aligned(const TV *value, const TV *out, const LevelTables &lt) const
    {
        return aligned(sizeof(TV), {value, out}) && aligned(sizeof(T), {aw}) && aligned(2 * sizeof(T), {loc}) && aligned(8, {lt.shapes, lt.lsi});
    }
    bool window_rows(const TV *value, const TV *out) const { return aligned(4 * sizeof(TV), {value, out}); }
    hipError_t launch_window(const Problem &pb, const TV *value, TV *out, unsigned *probe, hipStream_t stream) const
    {
        return msda::launch_fwd_tiled_tv<TV>(value, loc, aw, out, pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data(), probe, stream);
    }
    template <int CC, int WAVES>
    void launch_direct(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const TV *value, const LevelTables &lt, TV *out, const msda::DirectGeom &g) const
    {
        hipLaunchKernelGGL((msda::fwd_direct_kernel<T, CC, WAVES, TV>), grid, block, lds, stream, value, lt.shapes, lt.lsi, loc, aw, out, g);
    }
};

// PrepLoc: computed by the kernel itself from the raw projection (offsets, logits) and the reference points; loc / aw are by-products.
template <typename T, typename TV, typename TP>
struct PrepLoc {
    static constexpr bool kSplit = false;
    static constexpr int kDirectVariant = 5, kWindowVariant = 6;
    static constexpr const char *kDirectWhat = "launch of the fused location / softmax / gather kernel";
    static constexpr const char *kWindowWhat = "launch of the fused location / softmax / window-gather kernel";
    static constexpr const char *kTag = "", *kMisaligned = "sampling_loc needs 2*sizeof(T)";
    const TP *offsets, *logits;
    int64_t off_stride, log_stride;
    const T *ref;
    int ref_dim;
    T *loc, *aw;
    bool call_aligned(const TV *value, const TV *out, const LevelTables &lt) const
    {
        return aligned(sizeof(TV), {value, out}) && aligned(sizeof(T), {aw, ref}) && aligned(2 * sizeof(T), {loc}) &&
               aligned(sizeof(TP), {offsets, logits}) && aligned(8, {lt.shapes, lt.lsi});
    }
    bool window_rows(const TV *value, const TV *out) const
    {
        return aligned(4 * sizeof(TV), {value, out}) && aligned(2 * sizeof(TP), {offsets}) && off_stride % 2 == 0 && aligned(sizeof(TP), {logits}) &&
               aligned(8, {ref, loc}) && aligned(4, {aw});
    }
    hipError_t launch_window(const Problem &pb, const TV *value, TV *out, unsigned *probe, hipStream_t stream) const
    {
        const msda::TiledPrepSrc src{offsets, logits, (long long)off_stride, (long long)log_stride, ref, ref_dim, loc, aw};
        return msda::launch_fwd_tiled_prep<TV, TP>(value, src, out, pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data(), probe, stream);
    }
    template <int CC, int WAVES>
    void launch_direct(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const TV *value, const LevelTables &lt, TV *out, const msda::DirectGeom &g) const
    {
        const msda::PrepSrc<TP> src{offsets, logits, off_stride, log_stride, ref_dim};
        hipLaunchKernelGGL((msda::fwd_direct_prep_kernel<T, CC, WAVES, TV, TP>), grid, block, lds, stream, value, lt.shapes, lt.lsi, src, ref, loc, aw, out, g);
    }
};

// The window-kernel attempt (msda_tiled.h: fp32 compute, rows read four channels at a time).  `variant`: what was asked for; where a window
// kernel applies (*applies), what the call runs -- in automatic mode the locality monitor's choice.  kNextPath unless that is 2.
template <typename TV, typename Src>
int window_fwd(int &variant, bool *applies, const Problem &pb, const TV *value, TV *out, const Src &src, hipStream_t stream)
{
    *applies = variant != 1 && src.window_rows(value, out) &&
               msda::plan_gather(pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data()).ok;
    if (!*applies) return kNextPath;
    const FwdChoice ch = choose_window_fwd(variant, pb, src.loc, stream);
    variant = ch.variant;
    if (variant != 2) return kNextPath;
    const int rc = run_path(0, Src::kWindowVariant, (int)sizeof(TV), Attempt::kNo, pb, stream, [&]() {
        return Launched{src.launch_window(pb, value, out, ch.probe, stream), Src::kWindowWhat, Src::kTag};
    });
    if (ch.probe) monitor_finish_probe(ch.mo, 2.0 * pb.N * pb.Lq * pb.M * pb.L * pb.P, stream, rc == MSDA_OK);
    return rc;
}

// The direct kernels (msda_direct.h); for given locations the split kernel first -- small calls at D = 32 (decoder-shaped): 32 lanes per item,
// all of a lane's gathers in flight at once (fwd_split_kernel); fwd_variant 3 forces it wherever it applies, 1 keeps the 8-lane kernel.
template <typename T, typename TV, typename Src>
int direct_fwd(int variant, const Problem &pb, const TV *value, const LevelTables &lt, TV *out, const Src &src, hipStream_t stream)
{
    constexpr bool kBf16 = std::is_same<TV, msda::bf16_t>::value;
    const int C = pick_channels<TV>(pb.D, kMaxChannels<TV>, {value, out});
    msda::DirectGeom g = direct_geom(pb, C);
    const size_t lds = msda::direct_lds_bytes<T>(g);
    if (kBf16 && lds > 64 * 1024) return too_many_levels(pb.L);
    if constexpr (Src::kSplit && std::is_same<T, float>::value) {
        if (split_fits(pb, C) && (variant == 3 || (variant != 1 && split_small(pb))))
            return run_path(0, 3, (int)sizeof(TV), Attempt::kNo, pb, stream, [&]() {
                return Launched{launch_fwd_split<TV>(pb, value, lt.shapes, lt.lsi, src.loc, src.aw, out, g, stream), "launch of the split forward kernel",
                                Src::kTag};
            });
    }
    if (lds > 64 * 1024) return too_many_levels(pb.L);
    return run_path(0, Src::kDirectVariant, (int)sizeof(TV), Attempt::kNo, pb, stream, [&]() {
        const dim3 grid(direct_grid(g)), block(msda::kDirectThreads);
        with_channels<T>(C, [&](auto cc) {
            constexpr int CC = decltype(cc)::value;
            if (many_items(pb)) src.template launch_direct<CC, 6>(grid, block, lds, stream, value, lt, out, g);
            else src.template launch_direct<CC, 4>(grid, block, lds, stream, value, lt, out, g);
        });
        return Launched{hipGetLastError(), Src::kDirectWhat, Src::kTag};
    });
}

// The forward of a checked problem with given locations, for the variant the caller (msda_forward_* or _forward_prep_*) decided on.
template <typename T, typename TV>
int forward_body(int variant, const Problem &pb, const TV *value, const LevelTables &lt, const GivenLoc<T, TV> &src, TV *out, hipStream_t stream)
{
    if constexpr (std::is_same<T, float>::value) {
        bool applies;
        const int rc = window_fwd(variant, &applies, pb, value, out, src, stream);
        if (rc != kNextPath) return rc;
    }
    return direct_fwd<T, TV>(variant, pb, value, lt, out, src, stream);
}

template <typename T, typename TV = T>
int forward_impl(const Options &opt, const TV *value, const LevelTables &lt, const T *loc, const T *aw, int N, int S, int M, int D, int L, int Lq,
                 int P, int im2col_step, TV *out, msda_stream_t stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const GivenLoc<T, TV> src{loc, aw};
    Problem pb{N, S, M, D, L, Lq, P, {}, {}};
    if (int rc = checked_problem(pb, value && lt.shapes && lt.lsi && loc && aw && out, lt, im2col_step, stream, src.call_aligned(value, out, lt),
                                 src.kMisaligned))
        return rc;
    return forward_body<T, TV>(opt.fwd_variant, pb, value, lt, src, out, stream);
}

// One attempt of an fp32-compute backward call at the routed pixel-stationary kernels (msda_rps.h; variant 4) or the row-band kernel
// (msda_band.h; variant 5): kNextPath when the kernel does not apply.  Both take grad_value twice: the tensor, and an fp32 image for the
// levels several workgroups add to -- grad_value itself, or for bf16 the library's scratch (zeroed by the kernels, rounded once at the end);
// plain bf16 stores serve the levels a workgroup owns alone.
template <typename TV>
int bwd_routed_or_band(int variant, const Problem &pb, const TV *value, const float *loc, const float *aw, const TV *grad_out, TV *grad_value,
                       float *grad_loc, float *grad_aw, hipStream_t stream)
{
    constexpr bool kBf16 = std::is_same<TV, msda::bf16_t>::value;
    constexpr const char *kTag = kBf16 ? " (bf16)" : "";
    constexpr Attempt kAttempt = kBf16 ? Attempt::kRecordStaysOnError : Attempt::kRecordBackOnError;      // (the table's "... a launch error there")
    if (kBf16 && !aligned(8, {value, grad_out, grad_value})) return kNextPath;
    GradAcc<float, TV> acc(grad_value, (size_t)pb.N * pb.S * pb.M * pb.D, stream);
    bool go = false;
    if (variant == 4) go = (!kBf16 || pb.D == msda::kRpsD) && acc.have();
    else if (variant == 5 && (!kBf16 || pb.D == msda::kBandD)) {
        go = true;
        if constexpr (kBf16) {      // (a scratch only if the plan has levels that several workgroups add to)
            const msda::BandPlan bp = msda::plan_band(pb.N, pb.S, pb.M, pb.D, pb.L, pb.Lq, pb.P, pb.shapes.data(), pb.lsi.data());
            go = bp.ok && (!bp.atomic_levels || acc.have());
        }
    }
    if (!go) return kNextPath;
    return run_path(1, variant, (int)sizeof(TV), kAttempt, pb, stream, [&]() {
        if (variant == 4)
            return Launched{launch_bwd_rps<TV>(pb, value, loc, aw, grad_out, grad_value, acc.ptr, grad_loc, grad_aw, stream), "launch of the routed backward kernels", kTag};
        return Launched{launch_bwd_band<TV>(pb, value, loc, aw, grad_out, grad_value, acc.ptr, grad_loc, grad_aw, stream), "launch of the row-band backward kernel", kTag};
    });
}

template <typename T, typename TV = T>
int backward_impl(const Options &opt, const TV *value, const LevelTables &lt, const T *loc, const T *aw, const TV *grad_out, int N, int S, int M,
                  int D, int L, int Lq, int P, int im2col_step, TV *grad_value, T *grad_loc, T *grad_aw, msda_stream_t stream_)
{
    constexpr bool kBf16 = std::is_same<TV, msda::bf16_t>::value;
    constexpr const char *kTag = kBf16 ? " (bf16)" : "";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Problem pb{N, S, M, D, L, Lq, P, {}, {}};
    if (int rc = checked_problem(pb, value && lt.shapes && lt.lsi && loc && aw && grad_out && grad_value && grad_loc && grad_aw, lt, im2col_step, stream,
                                 aligned(sizeof(TV), {value, grad_out, grad_value}) && aligned(sizeof(T), {aw, grad_aw}) &&
                                     aligned(2 * sizeof(T), {loc, grad_loc}) && aligned(8, {lt.shapes, lt.lsi}),
                                 kBf16 ? "sampling_loc / grad_sampling_loc need 8 bytes" : "sampling_loc / grad_sampling_loc need 2*sizeof(T)"))
        return rc;
    const size_t n_value = (size_t)N * S * M * D;

    // Kernel choice: the routed pixel-stationary kernels (msda_rps.h: no float atomics, no zero-fill, cost independent of where
    // the points fall) for encoder-shaped fp32-compute calls at D = 32 (bwd_variant 4 forces them for any Lq, 1 forces the direct
    // path); everything else -- other D, f64, decoder shapes -- runs the level-sum + direct kernels below.
    // bwd_variant 5: the row-band kernel (msda_band.h) -- grad_value, grad_sampling_loc and grad_attn_weight in ONE launch, no zero-fill of
    // grad_value.  A measured option, not the automatic choice: 101-123 us on the decoder call Dd against 88 us for the level-sum + direct
    // kernels below (profiles/r05_dd_backward.md).
    if constexpr (std::is_same<T, float>::value) {
        const int variant = opt.bwd_variant ? opt.bwd_variant : (Lq == S ? 4 : 1);
        const int rc = bwd_routed_or_band<TV>(variant, pb, value, loc, aw, grad_out, grad_value, grad_loc, grad_aw, stream);
        if (rc != kNextPath) return rc;
    }

    // Direct path.  Levels summed in f64 LDS windows by their own kernel (msda_levelsum.h; fp32 compute only) are taken away from the
    // atomics below; when that is ALL levels (decoder-shaped calls) grad_value is written, not accumulated: no zero-fill, no atomics, and
    // for bf16 no scratch (the window is rounded at its one store).  bf16 takes all levels or none: otherwise every corner goes to the
    // fp32 scratch with row atomics.
    unsigned ls_levels = 0;
    msda::LevelSumGeom lg;
    size_t ls_lds = 0;
    if constexpr (std::is_same<T, float>::value) {
        // (its plain per-level stores need the levels to tile [0, S) without overlap; check_problem only bounds them)
        if (opt.levelsum && levels_tile(pb))
            ls_levels = msda::plan_levelsum(N, S, M, D, L, Lq, P, pb.shapes.data(), pb.lsi.data(), lg, ls_lds);
        if (kBf16 && ls_levels != all_levels_mask(L)) ls_levels = 0;
    }
    const bool all_summed = ls_levels == all_levels_mask(L);
    // what the direct kernel accumulates grad_value into (the reference gets it from at::zeros_like, ms_deform_attn_cuda.cu:121)
    GradAcc<T, TV> acc(grad_value, n_value, stream);
    if (!all_summed) {
        if (!acc.have())
            return fail(MSDA_ERR_BAD_DIMS, "bf16 backward of this shape needs an fp32 scratch buffer, which cannot be allocated "
                                           "while the stream is being captured: run the call once outside the capture");
        const hipError_t e = hipMemsetAsync(acc.ptr, 0, sizeof(T) * n_value, stream);
        if (e != hipSuccess) return hip_fail(e, kBf16 ? "zero-fill of the fp32 scratch" : "zero-fill of grad_value");
    }
    // Float atomics run at full rate only as >= 128-B row segments (one dword per lane): with 32 or more
    // channels put ONE channel on a lane, so that a wave-instruction adds two whole 128-B rows.
    int C = pick_channels<TV>(D, kMaxChannels<TV>, {value, grad_out});
    const int cpl = kBf16 ? 0 : opt.bwd_cpl;
    if (cpl > 0) C = cpl <= C ? cpl : C;
    else if (D * (int)sizeof(T) >= 128 && !all_summed) C = 1;
    msda::DirectGeom g = direct_geom(pb, C);
    const size_t lds = msda::direct_lds_bytes<T>(g);
    if (lds > 64 * 1024) return too_many_levels(L);
    // grad_value complete after the level-sum kernel: the location / weight gradients of a small call come from the split kernel
    // (bwd_split = 0 keeps the 8-lane one) -- and, fp32 storage, both jobs from ONE launch whose workgroups are of two kinds (msda_roles.h:
    // 65.9-66.7 against 70.0-70.2 us on call Dd; bwd_dd_roles = 0 keeps the two launches; bf16 storage keeps them too: the one-launch form
    // has not been measured there).  (Forking the level-sum kernel onto a second stream beside the direct kernel was tried: the cross-stream
    // fork / join costs more than the overlap gains on a 90 us call -- 113 vs 96 us.)
    const bool split = all_summed && opt.bwd_split && split_fits(pb, C) && split_small(pb);
    const bool roles = !kBf16 && opt.bwd_dd_roles && split && P == 4 && aligned(16, {loc, aw});
    return run_path(1, 1, (int)sizeof(TV), Attempt::kNo, pb, stream, [&]() -> Launched {
        hipError_t e;
        if constexpr (std::is_same<T, float>::value) {
            if constexpr (!kBf16) {
                if (roles) {
                    e = launch_bwd_dd_roles(pb, value, lt.shapes, lt.lsi, loc, aw, grad_out, grad_value, grad_loc, grad_aw, g, stream);
                    if (e == hipSuccess) ++g_bwd_dd_roles_calls;
                    if (e != hipErrorNotSupported) return {e, "launch of the level-sum / split role kernel"};
                }
            }
            if (ls_levels) {
                bool at_lds_limit;
                e = launch_bwd_levelsum<TV>(pb, loc, aw, grad_out, grad_value, lg, ls_lds, stream, &at_lds_limit);
                if (e != hipSuccess && at_lds_limit) return {e, kBf16 ? "LDS limit" : "launch of the level-sum backward kernel"};
                if (e != hipSuccess) return {e, "launch of the level-sum backward kernel", kTag};
                g.gv_skip = ls_levels;
            }
            if (split) return {launch_bwd_split<TV>(pb, value, lt.shapes, lt.lsi, loc, aw, grad_out, grad_loc, grad_aw, g, stream), "launch of the split backward kernel", kTag};
        }
        with_channels<T>(C, [&](auto cc) {
            hipLaunchKernelGGL((msda::bwd_direct_kernel<T, decltype(cc)::value, TV>), dim3(direct_grid(g)), dim3(msda::kDirectThreads), lds, stream,
                               value, lt.shapes, lt.lsi, loc, aw, grad_out, acc.ptr, grad_loc, grad_aw, g);
        });
        if ((e = hipGetLastError()) != hipSuccess) return {e, "launch of the direct backward kernel", kTag};
        if constexpr (kBf16) {
            if (!all_summed) {      // one rounding of the fp32 sums
                const size_t n4 = aligned(8, {grad_value}) ? n_value / 4 : 0;
                hipLaunchKernelGGL(round_to_bf16_kernel, dim3(2048), dim3(256), 0, stream, acc.ptr, grad_value, n4, n_value);
                return {hipGetLastError(), "rounding grad_value to bf16"};
            }
        }
        return {hipSuccess};
    });
}

// ---- module-level element-wise kernels (msda_prep.h) -----------------------------------------------------------------------------
int prep_geom(msda::PrepGeom &g, int N, int Lq, int M, int L, int P, int ref_dim, const int64_t *shapes_host)
{
    if (N <= 0 || Lq <= 0 || M <= 0 || L <= 0 || P <= 0) return fail(MSDA_ERR_BAD_DIMS, "non-positive dimension");
    if (L > msda::kPrepMaxL || L * P > 64) return fail(MSDA_ERR_BAD_DIMS, "L (%d) > %d or L*P (%d) > 64", L, msda::kPrepMaxL, L * P);
    if (ref_dim != 2 && ref_dim != 4) return fail(MSDA_ERR_BAD_DIMS, "Last dim of reference_points must be 2 or 4, but get %d instead.", ref_dim);
    if (!shapes_host) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    g = msda::PrepGeom{};
    g.N = N; g.Lq = Lq; g.M = M; g.L = L; g.P = P; g.ref_dim = ref_dim;
    int G = 1;
    while (G < L * P) G <<= 1;
    g.G = G;
    for (int l = 0; l < L; ++l) {
        g.H[l] = (float)shapes_host[2 * l];
        g.W[l] = (float)shapes_host[2 * l + 1];
    }
    return MSDA_OK;
}

template <typename T, typename TP = T>
int prep_forward_impl(const TP *offsets, int64_t off_stride, const TP *logits, int64_t log_stride, const T *ref, int ref_dim,
                      const int64_t *shapes_host, int N, int Lq, int M, int L, int P, T *loc, T *aw, msda_stream_t stream_)
{
    g_err[0] = 0;
    if (!offsets || !logits || !ref || !loc || !aw) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    msda::PrepGeom g;
    if (int rc = prep_geom(g, N, Lq, M, L, P, ref_dim, shapes_host)) return rc;
    if (off_stride < (int64_t)M * L * P * 2 || log_stride < (int64_t)M * L * P)
        return fail(MSDA_ERR_BAD_DIMS, "row stride smaller than a row (offsets %lld, logits %lld)", (long long)off_stride, (long long)log_stride);
    g.off_stride = off_stride;
    g.log_stride = log_stride;
    const int64_t items = (int64_t)N * Lq * M, per_block = 256 / g.G;
    const int grid = (int)std::min<int64_t>((items + per_block - 1) / per_block, 8192);
    hipLaunchKernelGGL((msda::prep_forward_kernel<T, TP>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream_), offsets, logits, ref, loc, aw, g);
    return launched("launch of the location / softmax kernel");
}

template <typename T, typename TP = T>
int prep_backward_impl(const T *grad_loc, const T *grad_aw, const T *aw, const TP *offsets, int64_t off_stride, const T *ref,
                       int ref_dim, const int64_t *shapes_host, int N, int Lq, int M, int L, int P, TP *grad_offsets,
                       int64_t goff_stride, TP *grad_logits, int64_t glog_stride, T *grad_ref, msda_stream_t stream_)
{
    g_err[0] = 0;
    if (!grad_loc || !grad_aw || !aw || !ref || !grad_offsets || !grad_logits || (ref_dim == 4 && grad_ref && !offsets))
        return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    msda::PrepGeom g;
    if (int rc = prep_geom(g, N, Lq, M, L, P, ref_dim, shapes_host)) return rc;
    if (goff_stride < (int64_t)M * L * P * 2 || glog_stride < (int64_t)M * L * P)
        return fail(MSDA_ERR_BAD_DIMS, "row stride smaller than a row");
    g.off_stride = off_stride;
    g.goff_stride = goff_stride;
    g.glog_stride = glog_stride;
    const int64_t items = (int64_t)N * Lq, per_block = 256 / g.G;
    const int grid = (int)std::min<int64_t>((items + per_block - 1) / per_block, 8192);
    hipLaunchKernelGGL((msda::prep_backward_kernel<T, TP>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream_), grad_loc, grad_aw,
                       aw, offsets, ref, grad_offsets, grad_logits, grad_ref, g);
    return launched("launch of the location / softmax backward kernel");
}

}  // namespace

// ---- msda_forward_prep_*: the module's softmax + location arithmetic and the operator's forward behind ONE entry point ----------------
// Decoder-shaped calls (Lq != S) with L * P <= 32 run fwd_direct_prep_kernel -- one launch, sampling_loc / attn_weight written as a
// by-product --; everything else (the encoder-shaped calls keep their LDS-window kernel and its locality monitor, which read
// sampling_loc) runs the location / softmax kernel and then the forward of the same library, as two launches.  Results are those of
// msda_prep_forward_* followed by msda_forward_* (the softmax sums in a different order: last-ulp differences).
template <typename T, typename TV, typename TP>
int forward_prep_impl(const Options &opt, const TV *value, const LevelTables &lt, const TP *offsets, int64_t off_stride, const TP *logits,
                      int64_t log_stride, const T *ref, int ref_dim, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step, TV *out,
                      T *loc, T *aw, msda_stream_t stream_)
{
    g_err[0] = 0;
    if (!value || !lt.shapes || !lt.lsi || !offsets || !logits || !ref || !out || !loc || !aw) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (ref_dim != 2 && ref_dim != 4) return fail(MSDA_ERR_BAD_DIMS, "reference points must have 2 or 4 components, got %d", ref_dim);
    if (off_stride < (int64_t)M * L * P * 2 || log_stride < (int64_t)M * L * P)
        return fail(MSDA_ERR_BAD_DIMS, "row stride smaller than a row (offsets %lld, logits %lld)", (long long)off_stride, (long long)log_stride);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const PrepLoc<T, TV, TP> src{offsets, logits, off_stride, log_stride, ref, ref_dim, loc, aw};
    Problem pb{N, S, M, D, L, Lq, P, {}, {}};
    if (opt.fwd_prep_fused && Lq != S && L * P <= msda::kPointBatch) {      // decoder-shaped: one launch
        if (int rc = checked_problem(pb, true, lt, im2col_step, stream, src.call_aligned(value, out, lt), src.kMisaligned)) return rc;
        return direct_fwd<T, TV>(0, pb, value, lt, out, src, stream);
    }
    // Encoder-shaped calls (round 5): the LDS-window kernel reads the raw projection itself -- softmax by the
    // quad that owns the query, location arithmetic by the lane that resolves the point --: no prep_forward_kernel launch, no re-read of loc /
    // aw.  While the locality monitor sends the call to the direct kernel the two-launch form below runs, with that choice held.
    const GivenLoc<T, TV> given{loc, aw};
    int variant = opt.fwd_variant;
    bool checked = false;
    if constexpr (std::is_same<T, float>::value) {
        if (opt.fwd_prep_fused >= 2 && P == 4 && variant != 1) {
            if (int rc = checked_problem(pb, true, lt, im2col_step, stream, true, "")) return rc;      // (alignment: see below)
            checked = true;
            bool applies;
            const int rc = window_fwd(variant, &applies, pb, value, out, src, stream);
            if (rc != kNextPath) return rc;
            variant = applies ? 1 : opt.fwd_variant;
        }
    }
    // two launches: the location / softmax kernel, then the forward with the locations it wrote
    if (int rc = prep_forward_impl<T, TP>(offsets, off_stride, logits, log_stride, ref, ref_dim, lt.shapes_host, N, Lq, M, L, P, loc, aw, stream_))
        return rc;
    if (checked) {      // what is left of the check: the alignment msda_forward_* demands
        if (!given.call_aligned(value, out, lt)) return misaligned_fail(given.kMisaligned);
    } else if (int rc = checked_problem(pb, true, lt, im2col_step, stream, given.call_aligned(value, out, lt), given.kMisaligned))
        return rc;
    return forward_body<T, TV>(variant, pb, value, lt, given, out, stream);
}

// The options: one table read by msda_set_option and msda_get_option.  A value is accepted when it lies in [lo, hi] and, where `values`
// is not 0, bit `value` of it is set.  hi < lo: the option cannot be set.
namespace {
struct Option {
    const char *key;
    std::atomic<int> *at;
    int lo, hi;
    unsigned values;
};
const Option *find_option(const char *key)
{
    static const Option table[] = {
        {"fwd_variant", &g_fwd_variant, 0, 3, 0},
        {"fwd_prep_fused", &g_fwd_prep_fused, 0, 2, 0},      // 1: decoder-shaped calls; 2: + encoder-shaped
        {"bwd_variant", &g_bwd_variant, 0, 5, 1u << 0 | 1u << 1 | 1u << 4 | 1u << 5},
        {"band_lds_kb", &msda::band_options().lds_kb, 16, 150, 0},
        {"band_hits", &msda::band_options().hits, 32, 65536, 0},
        {"rps_tile", &msda::rps_options().tile, 4, 16, 0},
        {"rps_max_chunks", &msda::rps_options().max_chunks, 1, 4096, 0},
        {"rps_route_wgs", &msda::rps_options().route_wgs, 1, 64, 0},
        {"rps_seg_shift", &msda::rps_options().seg_shift, 3, 11, 0},
        {"rps_order", &msda::rps_options().order, 0, 1, 0},
        {"bwd_direct_cpl", &g_bwd_cpl, 0, 4, 1u << 0 | 1u << 1 | 1u << 2 | 1u << 4},
        {"tile_region", &msda::tiled_options().region_px, 4, 64, 0},
        {"tile_margin", &msda::tiled_options().margin, 0, 32, 0},
        {"tile_persist", &msda::tiled_options().persist, 0, 65536, 0},
        {"bwd_levelsum", &g_levelsum, 0, 1, 0},
        {"bwd_split", &g_bwd_split, 0, 1, 0},
        {"bwd_dd_roles", &g_bwd_dd_roles, 0, 1, 0},
        {"bwd_dd_roles_calls", &g_bwd_dd_roles_calls, 0, -1, 0},   // read-only: calls that took the one-launch path
        {"profile_filter", &g_prof_filter, 0, 47, 0},
        {"levelsum_lds_kb", &msda::levelsum_lds_kb(), 8, 150, 0},
        {"tile_grow", &msda::tiled_options().grow, 0, 1, 0},
        {"locality_monitor", &g_monitor_on, 0, 1, 0},
        {"locality_share_ppm", &g_last_share_ppm, 0, -1, 0},   // read-only
    };
    for (const Option &o : table)
        if (key && !strcmp(key, o.key)) return &o;
    return nullptr;
}

// a storage pointer of the ABI as the kernels take it: bf16 travels as uint16_t
template <typename X> X *kptr(X *p) { return p; }
const msda::bf16_t *kptr(const uint16_t *p) { return reinterpret_cast<const msda::bf16_t *>(p); }
msda::bf16_t *kptr(uint16_t *p) { return reinterpret_cast<msda::bf16_t *>(p); }
}  // namespace

extern "C" {

int msda_abi_version(void) { return RICHSEM_MSDA_ABI_VERSION; }

// the host variants the reference declares and does not implement (src/cpu/ms_deform_attn_cpu.cpp:17-41)
int msda_forward_cpu(const void *, const int64_t *, const int64_t *, const void *, const void *, int, int, int, int, int, int, int, int, void *)
{
    return fail(MSDA_ERR_NOT_ON_CPU, "Not implement on cpu");
}
int msda_backward_cpu(const void *, const int64_t *, const int64_t *, const void *, const void *, const void *, int, int, int, int, int, int, int,
                      int, void *, void *, void *)
{
    return fail(MSDA_ERR_NOT_ON_CPU, "Not implement on cpu");
}

const char *msda_last_error(void) { return g_err; }

int msda_set_option(const char *key, int value)
{
    const Option *o = find_option(key);
    if (!o || value < o->lo || value > o->hi || (o->values && !(o->values >> value & 1)))
        return fail(MSDA_ERR_BAD_OPTION, "unknown option or value: %s=%d", key ? key : "(null)", value);
    *o->at = value;
    if (o->at == &g_monitor_on) {
        for (Monitor &mo : g_monitors) {   // switching it (either way) forgets what was learnt
            std::lock_guard<std::mutex> lock(mo.mu);
            mo.table.clear();
            for (ProbeSlot &ps : mo.slot) ps.pending = false;   // (probes still in flight belong to what is being forgotten)
        }
        g_last_share_ppm = -1;
    }
    return MSDA_OK;
}

int msda_get_option(const char *key, int *value)
{
    if (!value) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    const Option *o = find_option(key);
    if (!o) return fail(MSDA_ERR_BAD_OPTION, "unknown option: %s", key ? key : "(null)");
    *value = *o->at;
    return MSDA_OK;
}

int msda_tiled_plan(int N, int S, int M, int D, int L, int Lq, int P, const int64_t *shapes_host,
                    const int64_t *level_start_host, int *info)
{
    if (!shapes_host || !level_start_host || !info) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (L < 1 || L > 64) return fail(MSDA_ERR_BAD_DIMS, "bad L=%d", L);
    const msda::TiledPlan pl = msda::plan_gather(N, S, M, D, L, Lq, P, shapes_host, level_start_host);
    info[0] = pl.ok ? 1 : 0;
    info[1] = pl.g.GY;
    info[2] = pl.g.GX;
    info[3] = pl.g.nphases;
    info[4] = (int)pl.lds_bytes;
    info[5] = pl.grid * (msda::kTD / msda::kFwdGC);
    info[6] = pl.g.margin;
    info[7] = 0;
    if (pl.ok) {   // largest number of queries any region holds
        for (int gy = 0; gy < pl.g.GY; ++gy)
            for (int gx = 0; gx < pl.g.GX; ++gx) {
                int nq = 0;
                for (int l = 0; l < L; ++l) {
                    const msda::LevelRect r = msda::level_rect(pl.g.H[l], pl.g.W[l], gy, gx, pl.g.GY, pl.g.GX, pl.g.margin_l[l]);
                    nq += r.qnr * r.qnc;
                }
                info[7] = nq > info[7] ? nq : info[7];
            }
    }
    return MSDA_OK;
}

int msda_levelsum_plan(int N, int S, int M, int D, int L, int Lq, int P, const int64_t *shapes_host,
                       const int64_t *level_start_host, int *info)
{
    if (!shapes_host || !level_start_host || !info) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (L < 1 || L > 64) return fail(MSDA_ERR_BAD_DIMS, "bad L=%d", L);
    msda::LevelSumGeom lg;
    size_t lds = 0;
    const unsigned mask = msda::plan_levelsum(N, S, M, D, L, Lq, P, shapes_host, level_start_host, lg, lds);
    info[0] = (int)mask;
    info[1] = lg.nlev;
    info[2] = lg.nslices;
    info[3] = (int)lds;
    info[4] = mask ? msda::levelsum_grid(lg) : 0;
    int rows = 0;
    for (int e = 0; e < lg.nlev; ++e) rows = lg.nr[e] > rows ? lg.nr[e] : rows;
    info[5] = rows;
    info[6] = info[7] = 0;
    return MSDA_OK;
}

int msda_debug_stats(void *device_counter)
{
    msda::tiled_options().stats = static_cast<unsigned *>(device_counter);
    return MSDA_OK;
}

int msda_debug_stamps(void *device_buffer)
{
    msda::tiled_options().stamps = static_cast<unsigned long long *>(device_buffer);
    return MSDA_OK;
}

int msda_profile_enable(int capacity)
{
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_on = false;
    for (auto &s : g_prof_slots) {
        (void)hipEventDestroy(s.start);
        (void)hipEventDestroy(s.stop);
    }
    g_prof_slots.clear();
    g_prof_used = 0;
    if (capacity <= 0) return MSDA_OK;
    g_prof_slots.resize((size_t)capacity);
    for (auto &s : g_prof_slots) {
        hipError_t e = hipEventCreate(&s.start);
        if (e == hipSuccess) e = hipEventCreate(&s.stop);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
    }
    g_prof_on = true;
    return MSDA_OK;
}

int msda_profile_collect(msda_profile_record *records, int max_records, int *n_records)
{
    if (!records || !n_records) return fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    int n = 0;
    for (int i = 0; i < g_prof_used && n < max_records; ++i) {
        ProfileSlot &s = g_prof_slots[i];
        hipError_t e = hipEventSynchronize(s.stop);
        if (e == hipSuccess) e = hipEventElapsedTime(&s.rec.kernel_ms, s.start, s.stop);
        if (e != hipSuccess) return hip_fail(e, "reading profile events");
        records[n++] = s.rec;
    }
    *n_records = n;
    g_prof_used = 0;
    return MSDA_OK;
}

// The operator's entry points of one suffix: T the compute type (sampling_loc, attn_weight, reference points and their gradients), TA the
// storage type as the ABI spells it (uint16_t for bf16), TV as the kernels do (kptr turns one into the other).
#define MSDA_EXPORTS(SFX, T, TA, TV)                                                                                                                 \
    int msda_forward_##SFX(const TA *value, const int64_t *spatial_shapes, const int64_t *level_start, const T *sampling_loc,                        \
                           const T *attn_weight, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step, TA *out,                        \
                           const int64_t *shapes_host, const int64_t *level_start_host, msda_stream_t stream)                                        \
    {                                                                                                                                                \
        const LevelTables lt{spatial_shapes, level_start, shapes_host, level_start_host};                                                            \
        return forward_impl<T, TV>(Options{}, kptr(value), lt, sampling_loc, attn_weight, N, S, M, D, L, Lq, P, im2col_step, kptr(out), stream); \
    }                                                                                                                                                \
    int msda_backward_##SFX(const TA *value, const int64_t *spatial_shapes, const int64_t *level_start, const T *sampling_loc,                       \
                            const T *attn_weight, const TA *grad_out, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,             \
                            TA *grad_value, T *grad_sampling_loc, T *grad_attn_weight, const int64_t *shapes_host,                                   \
                            const int64_t *level_start_host, msda_stream_t stream)                                                                   \
    {                                                                                                                                                \
        const LevelTables lt{spatial_shapes, level_start, shapes_host, level_start_host};                                                            \
        return backward_impl<T, TV>(Options{}, kptr(value), lt, sampling_loc, attn_weight, kptr(grad_out), N, S, M, D, L, Lq, P, im2col_step,   \
                                    kptr(grad_value), grad_sampling_loc, grad_attn_weight, stream);                                                  \
    }                                                                                                                                                \
    int msda_forward_prep_##SFX(const TA *value, const int64_t *spatial_shapes, const int64_t *level_start, const TA *offsets, int64_t off_stride,   \
                                const TA *logits, int64_t log_stride, const T *ref, int ref_dim, int N, int S, int M, int D, int L, int Lq, int P,   \
                                int im2col_step, TA *out, T *sampling_loc, T *attn_weight, const int64_t *shapes_host,                               \
                                const int64_t *level_start_host, msda_stream_t stream)                                                               \
    {                                                                                                                                                \
        const LevelTables lt{spatial_shapes, level_start, shapes_host, level_start_host};                                                            \
        return forward_prep_impl<T, TV, TV>(Options{}, kptr(value), lt, kptr(offsets), off_stride, kptr(logits), log_stride, ref, ref_dim, N,   \
                                            S, M, D, L, Lq, P, im2col_step, kptr(out), sampling_loc, attn_weight, stream);                           \
    }                                                                                                                                                \
    int msda_prep_forward_##SFX(const TA *offsets, int64_t off_stride, const TA *logits, int64_t log_stride, const T *ref, int ref_dim,              \
                                const int64_t *shapes_host, int N, int Lq, int M, int L, int P, T *loc, T *aw, msda_stream_t stream)                 \
    {                                                                                                                                                \
        return prep_forward_impl<T, TV>(kptr(offsets), off_stride, kptr(logits), log_stride, ref, ref_dim, shapes_host, N, Lq, M, L, P, loc, aw,    \
                                        stream);                                                                                                     \
    }                                                                                                                                                \
    int msda_prep_backward_##SFX(const T *grad_loc, const T *grad_aw, const T *aw, const TA *offsets, int64_t off_stride, const T *ref,              \
                                 int ref_dim, const int64_t *shapes_host, int N, int Lq, int M, int L, int P, TA *grad_offsets,                      \
                                 int64_t goff_stride, TA *grad_logits, int64_t glog_stride, T *grad_ref, msda_stream_t stream)                       \
    {                                                                                                                                                \
        return prep_backward_impl<T, TV>(grad_loc, grad_aw, aw, kptr(offsets), off_stride, ref, ref_dim, shapes_host, N, Lq, M, L, P,                \
                                         kptr(grad_offsets), goff_stride, kptr(grad_logits), glog_stride, grad_ref, stream);                         \
    }
MSDA_EXPORTS(f32, float, float, float)
MSDA_EXPORTS(f64, double, double, double)
MSDA_EXPORTS(bf16, float, uint16_t, msda::bf16_t)
#undef MSDA_EXPORTS

}  // extern "C"
