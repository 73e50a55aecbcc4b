// modgpu_capi.cpp -- host side of the C ABI in include/modgpu.h: devices, launch planning, the
// entry points.  (host_stream.cpp: host-buffer / file routes; scalar_path.cpp: the host loop.)
//
// Compiled by hipcc as host-only C++ and linked with cycle_kernel.hip into libmodgpu.so.  The only
// arithmetic done here for a GPU call is the per-launch jump-ahead (a handful of modular powers)
// that seeds the kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/modgpu_testing.h"
#include "crossover_table.h"
#include "cycle_feed_kernel.h"
#include "cycle_keep_kernel.h"
#include "cycle_kernel.h"
#include "cycle_rekey_kernel.h"
#include "cycle_rekey_table_kernel.h"
#include "cycle_rekey_move_table_kernel.h"
#include "cycle_verify_table_kernel.h"
#include "cycle_rekey_verify_table_kernel.h"
#include "cycle_verify_kernel.h"
#include "cycle_rekey_verify_kernel.h"
#include "cycle_table_kernel.h"
#include "cycle_to_kernel.h"
#include "cycle_xfer_kernel.h"
#include "lcg.h"
#include "modgpu_internal.h"
#include "numa_place.h"
#include "scalar_path.h"

#ifndef MODGPU_KERNEL_SOURCE_HASH
#define MODGPU_KERNEL_SOURCE_HASH "unknown"
#endif
#ifndef MODGPU_TO_KERNEL_SOURCE_HASH
#define MODGPU_TO_KERNEL_SOURCE_HASH "unknown"
#endif
#ifndef MODGPU_XFER_KERNEL_SOURCE_HASH
#define MODGPU_XFER_KERNEL_SOURCE_HASH "unknown"
#endif
#ifndef MODGPU_REKEY_KERNEL_SOURCE_HASH
#define MODGPU_REKEY_KERNEL_SOURCE_HASH "unknown"
#endif

namespace modgpu {

thread_local std::string t_err;
Stats g_stats;

int fail(int code, const char *what)
{
    t_err = what;
    return code;
}
int fail(int code, const std::string &what)
{
    t_err = what;
    return code;
}
int fail_hip(hipError_t e, const char *where)
{
    t_err = std::string(where) + ": " + hipGetErrorString(e);
    return MODGPU_ERR_HIP;
}
int fail_io(const char *what)
{
    t_err = std::string(what) + ": " + std::strerror(errno);
    return MODGPU_ERR_IO;
}

// MODGPU_MIN_GPU_BYTES (read once): modgpu_cycle_auto_host serves buffers shorter than this with the host loop.
// A kernel launch plus the wait for it costs ~14 us before the first byte moves and the data crosses PCIe twice; the AVX-512
// host loop does 17 GB/s per core on the MI355X node's EPYC 9575F: a 4 KiB header takes 0.4 us against 16, 512 KiB (the
// largest header the reference can write, CArk.cpp:911-912) 30 us against 44 (profiles/r05_small_call_crossover.txt).  Since
// round 5's short-launch grid and finer cut the kernel route overtakes ONE host thread at 2 MiB already (it was 16-32 MiB when
// this default was chosen, r03), but from 4 MiB the host loop runs on several threads and stays ahead up to this size
// (4 / 8 / 16 MiB: 31 / 61 / 115 GB/s against 29 / 37 / 42), so below it a call is over sooner on the host whichever way one
// counts; from here up the default policy (below) gives the buffer to the GPU and the cores back to the caller.
constexpr uint64_t kMinGpuBytesDefault = 16ull << 20;
uint64_t min_gpu_bytes()
{
    static const uint64_t v = [] {
        const char *e = std::getenv("MODGPU_MIN_GPU_BYTES");
        if (!e || !*e) return kMinGpuBytesDefault;
        char *end = nullptr;
        unsigned long long x = std::strtoull(e, &end, 0);
        return end && end != e ? (uint64_t)x : kMinGpuBytesDefault;
    }();
    return v;
}

// MODGPU_HOST_POLICY (read once): what modgpu_cycle_auto_host -- CEncryptionCycler::Cycle -- does with a buffer of
// MODGPU_MIN_GPU_BYTES or more when a GPU is usable.
//   offload (default)  the kernel.  The host's cores stay free for the caller (an unpack walks 100 000 files beside the cipher)
//                      and every further GPU adds a PCIe link; the headline path is HBM-resident data anyway.
//   fastest            whichever engine the committed crossover table (crossover_table.h) says finishes THIS call sooner,
//                      the host loop priced as it really runs: on its threads, as many as this size, the control group's CPU
//                      quota and the caller's affinity mask give it.  On the node the table was taken on that is the host
//                      loop at every size (its threads out-run one PCIe link), so `fastest` mostly means "the GPU only when
//                      the host loop is short of threads".
// modgpu_path_stats().auto_policy_host counts the calls `fastest` kept on the host.
enum class HostPolicy { Offload, Fastest };
HostPolicy host_policy()
{
    static const HostPolicy v = [] {
        const char *e = std::getenv("MODGPU_HOST_POLICY");
        return e && std::strcmp(e, "fastest") == 0 ? HostPolicy::Fastest : HostPolicy::Offload;
    }();
    return v;
}

bool gpu_required()
{
    static const bool v = [] {
        const char *e = std::getenv("MODGPU_REQUIRE_GPU");
        return e && *e && std::strcmp(e, "0") != 0;
    }();
    return v;
}

// ---- devices ----------------------------------------------------------------------------------
int physical_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return std::min(n, kMaxDevices);
}

namespace {
// MODGPU_DEVICE_ALIAS=N (read once): rehearse N-GPU code on fewer GPUs.  0 = off.
int alias_count()
{
    static const int v = [] {
        const char *e = std::getenv("MODGPU_DEVICE_ALIAS");
        int x = e ? std::atoi(e) : 0;
        return x < 0 ? 0 : std::min(x, kMaxDevices);
    }();
    return v;
}
} // namespace

int logical_count()
{
    int p = physical_count();
    return p > 0 && alias_count() > 0 ? alias_count() : p;
}

int physical_of(int logical)
{
    int p = physical_count();
    return p > 0 ? logical % p : 0;
}

int select_device(int device)
{
    int n = logical_count();
    if (n <= 0) return fail(MODGPU_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0) return MODGPU_OK; // keep the thread's current device
    if (device >= n) return fail(MODGPU_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(physical_of(device)));
    return MODGPU_OK;
}

int resolve_device(int device, int *out)
{
    int rc = select_device(device);
    if (rc) return rc;
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    *out = device;
    return MODGPU_OK;
}

#ifdef MODGPU_TESTING_HOOKS
std::atomic<int> g_forced_gpu_node{-2}; // modgpu_debug_set_gpu_node: -2 = by sysfs
#endif
// NUMA node the GPU behind a logical device hangs off (-1: unknown, or placement switched off by MODGPU_NUMA=0).
int device_numa_node(int logical)
{
    static std::mutex mu;
    static int cached[kMaxDevices];
    static bool known[kMaxDevices] = {};
    if (!numa::enabled() || logical < 0 || logical >= kMaxDevices || physical_count() <= 0) return -1;
#ifdef MODGPU_TESTING_HOOKS
    if (const int forced = g_forced_gpu_node.load(std::memory_order_relaxed); forced >= -1) return forced; // modgpu_debug_set_gpu_node
#endif
    std::lock_guard<std::mutex> lock(mu);
    if (!known[logical]) {
        char bdf[64] = {};
        int node = -1;
        if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf - 1, physical_of(logical)) == hipSuccess) {
            for (char *c = bdf; *c; ++c) *c = (char)std::tolower((unsigned char)*c); // sysfs spells it lower-case
            node = numa::node_of_pci("/sys", bdf);
        } else {
            (void)hipGetLastError();
        }
        cached[logical] = node;
        known[logical] = true;
    }
    return cached[logical];
}

void run_near_device(int logical)
{
    const int node = device_numa_node(logical);
    if (node >= 0) (void)numa::run_on_node("/sys", node);
}

DeviceScope::DeviceScope(int device, bool always_save)
{
    if ((device >= 0 || always_save) && hipGetDevice(&prev_) != hipSuccess) {
        (void)hipGetLastError();
        prev_ = -1;
    }
    rc = device >= 0 || !always_save ? select_device(device) : MODGPU_OK;
}

DeviceScope::~DeviceScope()
{
    if (prev_ >= 0) (void)hipSetDevice(prev_); // the caller's thread keeps the device it came with
}

// ---- launch planning -----------------------------------------------------------------

namespace {

struct Plan {
    CycleArgs args;
    int variant;
    uint32_t grid;
};

// the calling thread's last launch (modgpu_last_launch: reporting only)
thread_local modgpu_launch_info_t t_last_launch{};
// forced shape / grid cap: exist only in the testing flavour of the library (libmodgpu_testing.so)
#ifdef MODGPU_TESTING_HOOKS
std::atomic<int> g_force_variant{-1};
std::atomic<uint32_t> g_grid_cap{0};
std::atomic<uint32_t> g_pcie_grid{0}; // modgpu_debug_set_pcie_grid: 0 = the product's rule
int forced_variant() { return g_force_variant.load(std::memory_order_relaxed); }
uint32_t forced_grid_cap() { return g_grid_cap.load(std::memory_order_relaxed); }
uint32_t forced_pcie_grid() { return g_pcie_grid.load(std::memory_order_relaxed); }
#else
constexpr int forced_variant() { return -1; }
constexpr uint32_t forced_grid_cap() { return 0; }
constexpr uint32_t forced_pcie_grid() { return 0; }
#endif

// The device's CU count (256 on MI355X), looked up once per device: the grid of the static streaming shape (one persistent
// 1024-thread workgroup per CU) and what the work-queue shape's grid is derived from (queue_grid: 25 main workgroups per
// 32 CUs plus a helper on each CU they leave idle).
uint32_t large_grid()
{
    static std::mutex mu;
    static uint32_t cus[kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256u;
    std::lock_guard<std::mutex> lock(mu);
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = (uint32_t)std::min(n, 2048); // grid * 32 tiles must stay <= 65536
    }
    return cus[dev];
}
// Work-queue shape: every launch needs a {ticket, done} pair that is zero when it starts; the kernel's last
// workgroup zeroes it again and then signs off in a host-visible word, so a per-device ring of pairs (one 128-byte
// line each) is allocated and cleared once.  Two launches must never share a pair while either runs (their
// tickets would interleave: chunks skipped in one, done twice in neither -- wrong bytes, no error), so
//   * an eager launch takes a ring line only if the line's previous user has signed off (done[line] ==
//     issued[line], an acquire load of host-coherent memory: no HIP call, nothing extra on the stream); if every
//     line is busy the launch takes the static streaming shape, which needs no pair;
//   * a launch that is being captured into a hipGraph is baked into the graph together with its pair, and may
//     be replayed at any later time, so it never draws from the ring: it gets a line of its own from a
//     separate grow-only pool that is never handed out again (pool empty: static shape).
constexpr uint32_t kQueueRing = 4096; // eager lines: more than any caller keeps in flight (a launch that finds none free still has the static shape)
constexpr uint32_t kGraphPool = 1024; // lines owned by captured launches, for the life of the process
// A pair has a 128-byte line to itself: that is the L2 line size, and two launches in flight must not have their ticket
// counters in one line (nor may anything that is polled sit there: profiles/r03_tune_dvfs.txt, stand-by helpers -- a reader in
// the ticket counter's line cost 15 %)
constexpr uint32_t kLineWords = 32;
struct QueueRing {
    std::mutex mu;
    std::atomic<uint32_t *> base{nullptr}; // device: (kQueueRing + kGraphPool) lines of kLineWords words, all zero between launches
    uint32_t *done = nullptr;              // host-coherent pinned memory: one word per ring line, written by the kernel
    uint32_t *done_dev = nullptr;          // the same words as the device addresses them
    uint32_t issued[kQueueRing] = {};      // sequence number given to the line's latest user   (under mu)
    uint32_t next = 0;                     // where the search for a free line starts           (under mu)
    uint32_t graph_used = 0;               // pool lines given away                             (under mu)
};
QueueRing g_queue_ring[kMaxDevices];
std::atomic<uint64_t> g_queue_eager{0}, g_queue_busy{0}, g_queue_graph{0}, g_queue_graph_full{0};
#ifdef MODGPU_TESTING_HOOKS
std::atomic<uint32_t> g_ring_lines{kQueueRing}; // modgpu_debug_set_queue_ring: a ring of 1 makes every overlap a collision
uint32_t ring_lines() { return g_ring_lines.load(std::memory_order_relaxed); }
#else
constexpr uint32_t ring_lines() { return kQueueRing; }
#endif

struct QueuePair {
    uint32_t *pair = nullptr; // nullptr: none available -> static shape
    uint32_t *done = nullptr;
    uint32_t seq = 0;
    int line = -1; // ring line to give back if the launch does not happen; -1: pool line / none
    int dev = -1;
};

// One-time set-up of a device's ring.  Not possible while `stream` is being captured (allocating there
// would break the capture); other threads' captures are kept out of it by relaxed capture mode.
bool queue_ring_create(QueueRing &r, hipStream_t stream)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return false;
    }
    std::lock_guard<std::mutex> lock(r.mu);
    if (r.base.load(std::memory_order_acquire)) return true;
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    uint32_t *lines = nullptr, *done = nullptr, *done_dev = nullptr;
    hipStream_t st = nullptr;
    const size_t bytes = (size_t)(kQueueRing + kGraphPool) * kLineWords * sizeof(uint32_t);
    bool ok = hipMalloc(reinterpret_cast<void **>(&lines), bytes) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&done), kQueueRing * sizeof(uint32_t),
                            hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer(reinterpret_cast<void **>(&done_dev), done, 0) == hipSuccess &&
              // the zeroes are in place before the ring is published: a kernel on ANY stream (non-blocking ones
              // included) may be the first user
              hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
              hipMemsetAsync(lines, 0, bytes, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    if (st) (void)hipStreamDestroy(st);
    if (ok) {
        std::memset(done, 0, kQueueRing * sizeof(uint32_t));
        r.done = done;
        r.done_dev = done_dev;
        r.base.store(lines, std::memory_order_release);
    } else {
        (void)hipGetLastError();
        if (lines) (void)hipFree(lines);
        if (done) (void)hipHostFree(done);
    }
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    return ok;
}

QueuePair queue_pair(hipStream_t stream)
{
    QueuePair q;
    if (hipGetDevice(&q.dev) != hipSuccess || q.dev < 0 || q.dev >= kMaxDevices) return q;
    QueueRing &r = g_queue_ring[q.dev];
    if (!r.base.load(std::memory_order_acquire) && !queue_ring_create(r, stream)) return q;
    uint32_t *base = r.base.load(std::memory_order_acquire);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return q;
    }
    std::lock_guard<std::mutex> lock(r.mu);
    if (cap != hipStreamCaptureStatusNone) { // the graph keeps its line for good
        if (r.graph_used >= kGraphPool) {
            g_queue_graph_full.fetch_add(1, std::memory_order_relaxed);
            return q;
        }
        q.pair = base + (size_t)(kQueueRing + r.graph_used++) * kLineWords;
        g_queue_graph.fetch_add(1, std::memory_order_relaxed);
        return q;
    }
    const uint32_t lines = std::max(1u, std::min(ring_lines(), kQueueRing));
    for (uint32_t k = 0; k < lines; ++k) {
        const uint32_t line = (r.next + k) % lines;
        // (an acquire load of a word the GPU writes: what follows is ordered behind seeing the sign-off)
        if (__atomic_load_n(&r.done[line], __ATOMIC_ACQUIRE) != r.issued[line]) continue; // its latest user has not signed off yet
        r.next = line + 1;
        q.pair = base + (size_t)line * kLineWords;
        q.done = r.done_dev + line;
        q.seq = ++r.issued[line];
        q.line = (int)line;
        g_queue_eager.fetch_add(1, std::memory_order_relaxed);
        return q;
    }
    g_queue_busy.fetch_add(1, std::memory_order_relaxed);
    return q;
}

// The launch that took this ring line did not happen: nobody will sign off for it.
void queue_pair_unused(const QueuePair &q)
{
    if (q.line < 0 || q.dev < 0) return;
    QueueRing &r = g_queue_ring[q.dev];
    std::lock_guard<std::mutex> lock(r.mu);
    --r.issued[q.line];
}

// Helper workgroups of the work-queue shape join while the shader clock is below this: with the three-instruction keystream
// the 25-per-32 main workgroups stay HBM-bound down to ~1.7 GHz (profiles/r03_first_pass.txt: 1 711 MHz 6.97 TB/s, 1 645 6.87,
// 1 579 6.69), and the steady-state clock sits at 2.0-2.2 GHz.  Thresholds from 1 600 to 1 950 MHz measure within run-to-run
// spread of each other, back to back (r03_tune_dvfs.txt) and with host gaps between launches (bench.py's first-pass series,
// A/B'd on one box: 1 850 a little better than 1 750 there, steady state identical); ~1 850 keeps ~150 MHz off the steady state.
// Round 4: the default is no longer a constant tuned on this pool's parts but a share of the device's own peak shader clock
// (hipDeviceAttributeClockRate: 2 400 MHz on MI355X -> 1 848 MHz): 77 %.  MODGPU_HELPER_BELOW_MHZ still overrides it.
constexpr uint32_t kHelperBelowMHzFallback = 1850;
constexpr uint32_t kHelperBelowPercentOfPeak = 77;
uint32_t helper_below_mhz() // MODGPU_HELPER_BELOW_MHZ (read once; 0 = helpers never join), else 77 % of the current device's peak clock
{
    static const long forced = [] {
        const char *e = std::getenv("MODGPU_HELPER_BELOW_MHZ");
        return e && *e ? (long)std::strtoul(e, nullptr, 0) : -1L;
    }();
    if (forced >= 0) return (uint32_t)forced;
    static std::mutex mu;
    static uint32_t by_dev[kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return kHelperBelowMHzFallback;
    std::lock_guard<std::mutex> lock(mu);
    if (!by_dev[dev]) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev) != hipSuccess || khz < 500000 || khz > 5000000) {
            (void)hipGetLastError();
            by_dev[dev] = kHelperBelowMHzFallback;
        } else {
            by_dev[dev] = (uint32_t)((long long)khz / 1000 * kHelperBelowPercentOfPeak / 100);
        }
    }
    return by_dev[dev];
}
#ifdef MODGPU_TESTING_HOOKS
std::atomic<int> g_helper_mode{0}; // modgpu_debug_set_helpers: 0 by the clock, 1 always join, 2 no helper workgroups
int helper_mode() { return g_helper_mode.load(std::memory_order_relaxed); }
#else
constexpr int helper_mode() { return 0; }
#endif

#ifdef MODGPU_TESTING_HOOKS
std::atomic<int> g_batch_mode{0}; // modgpu_debug_set_batch: 0 by size, 1 every group of >= 2 parts, 2 never
int batch_mode() { return g_batch_mode.load(std::memory_order_relaxed); }
#else
constexpr int batch_mode() { return 0; }
#endif
std::atomic<uint64_t> g_batch_launches{0}, g_batch_parts{0};

constexpr uint32_t kSmallGridMax = 16384u;   // 4 KiB chunks: grid * 1 tile <= 65536
// Hand-over between the small and the work-queue shape, measured warm and cold (profiles/r02_tune_cycle_sizes_cold.txt,
// r03_handover.txt, and again in profiles/r04_tail.txt at 100 MB): up to 256 MiB the one-shot 4 KiB-chunk grid wins (a
// launch's fixed cost is ~3 us against ~7 us, and a warm buffer sits in the 256 MiB Infinity Cache); beyond it the
// work-queue streaming kernel (64 KiB chunks handed out by tickets) does.
constexpr uint64_t kLargeMin = (256ull << 20) + 1;

// ---- a resident slice of large in-place passes (cycle_keep_kernel.hip) ----
// A single buffer of kKeepMin bytes or more takes the work-queue kernel's copy with a cache policy per chunk: of every kKeepMask + 1
// chunks of 64 KiB (16 MiB of addresses) the first `run` are stored so that they stay in the 256 MiB Infinity Cache, about
// kKeepBytes of the call in all; the next pass over the same memory finds them there.  The pattern is laid on absolute addresses, so
// it is the same for every call that touches a line.  Below kKeepMin the main kernel is launched, as for batches.
constexpr uint64_t kKeepMin = 1ull << 30;
constexpr uint64_t kKeepBytes = 192ull << 20; // S: resident bytes aimed at (the cache has 256 MiB); profiles/r13_keep.json
constexpr uint32_t kKeepMask = 255u;
struct KeepPolicy {
    bool route;         // launch the keep kernel
    uint32_t mask, run; // CycleKeepArgs
};
#ifdef MODGPU_TESTING_HOOKS
std::mutex g_keep_mutex; // modgpu_debug_set_keep
uint64_t g_keep_min = 0; // 0 = the product's rule
uint32_t g_keep_mask = 0, g_keep_run = 0;
#endif
KeepPolicy keep_policy(uint64_t bytes)
{
#ifdef MODGPU_TESTING_HOOKS
    {
        std::lock_guard<std::mutex> lock(g_keep_mutex);
        if (g_keep_min != 0) return {bytes >= g_keep_min, g_keep_mask, g_keep_run};
    }
#endif
    if (bytes < kKeepMin) return {false, kKeepMask, 0u};
    // run = floor(S / bytes * (mask + 1)): 0 once the call is so large that S is less than one chunk per period
    return {true, kKeepMask, (uint32_t)std::min<uint64_t>(kKeepBytes * (kKeepMask + 1ull) / bytes, kKeepMask + 1ull)};
}

// Splits [buf, buf+n) into <16 head bytes, an aligned body of 16-byte words and <16 tail bytes,
// and computes the states that seed each piece.  key_res != 0.
// Over PCIe (page-locked host memory): the link, not HBM, is the bound, and it is saturated by a few
// dozen workgroups of the one-word shape; more only adds contention (profiles/r02_sweep_pinned_routes.txt:
// 4 KiB chunks, grid <= 256: 50 GB/s of payload at 64 MiB .. 4 GiB; uncapped 46; the streaming shape 41-46).
constexpr uint32_t kPcieGridMax = 256u;
// ... and a SHORT launch across the link -- a staged chunk of 1-8 MiB, a header -- does best with fewer still (round 5,
// profiles/r05_pcie_grid.txt and the kernel traces beside it): with 256 workgroups every lane has its one 16-byte word in flight
// at the same moment, 1 MiB per grid trip, so a 4 MiB chunk is four bursts of reads each followed by a burst of writes and the
// link runs one way at a time for most of the launch; 32 workgroups (128 KiB per trip, still above the link's bandwidth-delay
// product) turn the same chunk into a 32-trip pipeline whose reads and writes overlap.  Pageable 64 MiB: 32 -> 39-40 GB/s.
constexpr uint32_t kPcieGridShort = 32u;
constexpr uint64_t kPcieShortMax = 64ull << 20;

// Workgroups of a work-queue launch over `chunks` chunks on a device of `cus` CUs: most main workgroups, and helpers.
// (A persistent 1024-thread, 128-VGPR workgroup needs a CU to itself, and the grid asks for every CU: whenever another kernel
//  holds part of a CU -- a caller's own work on another stream, a profiler's probe -- the LAST workgroup of its XCD, a helper
//  since helpers are dispatched last, does not start before another one there has left.  A helper looks at the clock for 2 us
//  and leaves, or finds the tickets gone: harmless by construction.  It is the reason helpers must never wait for anything --
//  round 5's stand-by experiment tripped over exactly this, profiles/r05_standby.txt.)
void queue_grid(uint64_t chunks, uint64_t cus, uint64_t *main_cap, uint64_t *helpers)
{
    const uint32_t grid_cap = forced_grid_cap();
    uint64_t cap = std::max<uint64_t>(1, cus * 25 / 32);
    const bool capped = grid_cap >= 1 && grid_cap < cus; // (testing flavour: a forced grid)
    if (capped && grid_cap < cap) cap = grid_cap;
    // (a launch of a few trips is over before a helper has looked at the clock; a forced grid gets helpers only when the
    //  tests force them to join, in the product's proportion)
    *helpers = 0;
    if (helper_mode() == 1) *helpers = capped ? std::max<uint64_t>(1, cap * 7 / 25) : cus - cap;
    else if (helper_mode() == 0 && !capped && chunks >= 4 * cus) *helpers = cus - cap;
    *main_cap = cap;
}

// The launch shape a single buffer takes by its size (or the one the testing flavour forces).
int choose_variant(const void *dev_buf, uint64_t n, bool over_pcie)
{
    const int forced = forced_variant();
    if (forced >= 0 && forced < kCycleVariants) return forced;
    const uint64_t head = std::min<uint64_t>(n, (16 - (reinterpret_cast<uintptr_t>(dev_buf) & 15)) & 15);
    const uint64_t body_bytes = (n - head) / 16 * 16;
    return body_bytes >= kLargeMin && !over_pcie ? CYCLE_QUEUE : CYCLE_SMALL;
}

// The small shape or the streaming shape with the static chunk map (the work-queue shape is planned by launch_queue).
Plan plan_cycle(void *dev_buf, uint64_t n, uint32_t key_res, uint64_t stream_off, bool over_pcie, int variant)
{
    Plan p{};
    uintptr_t addr = reinterpret_cast<uintptr_t>(dev_buf);
    uint64_t head = std::min<uint64_t>(n, (16 - (addr & 15)) & 15);
    uint64_t words = (n - head) / 16;
    uint64_t tail = n - head - words * 16;
    // the stream position of byte j is stream_off + j; positions reduce mod PERIOD
    uint64_t o = stream_off % lcg::PERIOD;

    CycleArgs &a = p.args;
    a.head_ptr = static_cast<uint8_t *>(dev_buf);
    a.head_n = (uint32_t)head;
    a.body = a.head_ptr + head;
    a.body_words = words;
    a.tail_ptr = a.head_ptr + head + words * 16;
    a.tail_n = (uint32_t)tail;
    a.base_head = lcg::state_residue(key_res, o);
    a.base_body = lcg::state_residue(key_res, o + head);
    a.base_tail = lcg::state_residue(key_res, o + head + (words * 16) % lcg::PERIOD);

    uint64_t body_bytes = words * 16;
    p.variant = variant == CYCLE_SMALL ? CYCLE_SMALL : CYCLE_LARGE;
    const uint64_t chunk = modgpu_variant_chunk_bytes(p.variant);
    // chunks sit on absolute chunk-aligned addresses: the first starts `lead` bytes before the body,
    // and the kernel counts positions from there, so its base state is stepped back by a^(-lead)
    a.lead = (uint32_t)(reinterpret_cast<uintptr_t>(a.body) & (chunk - 1));
    a.base_body = lcg::mulmod(a.base_body, lcg::powmod(lcg::A, lcg::PERIOD - a.lead % lcg::PERIOD));
    uint64_t chunks = (a.lead + body_bytes + chunk - 1) / chunk;
    uint64_t cap = p.variant == CYCLE_SMALL ? kSmallGridMax : large_grid();
    const uint32_t grid_cap = forced_grid_cap();
    if (grid_cap >= 1 && grid_cap < cap) cap = grid_cap;
    if (over_pcie) cap = forced_pcie_grid() ? std::min<uint64_t>(kSmallGridMax, forced_pcie_grid()) : std::min<uint64_t>(cap, body_bytes <= kPcieShortMax ? kPcieGridShort : kPcieGridMax);
    p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunks, cap));
    // one grid trip advances every lane-word by grid chunks
    a.stride_mul2 = 2u * lcg::powmod(lcg::A, ((uint64_t)p.grid * chunk) % lcg::PERIOD);
    return p;
}

// One launch of the work-queue shape over parts[0..n) -- 1..kCycleBatchMax non-empty buffers of the current device, each its
// own keystream.  Returns MODGPU_OK, an error, or 1: not possible right now (no ticket pair free -- every ring line busy, or a
// capture with the graph pool used up -- or a part beyond the kernel's three-byte chunk jump tables): the caller takes a shape
// that needs no pair.
// `warm_keep` (prepare_device): a single buffer takes the keep kernel whatever its size, with no chunk kept.
int launch_queue(void *const *bufs, const uint64_t *sizes, const uint64_t *offs, int n, uint32_t key_res, hipStream_t stream, bool warm_keep = false)
{
    CycleQueueArgs a{};
    const uint64_t chunk = modgpu_queue_chunk_bytes();
    uint64_t total = 0, bytes = 0;
    for (int k = 0; k < n; ++k) {
        CycleQueuePart &P = a.part[k];
        const uintptr_t addr = reinterpret_cast<uintptr_t>(bufs[k]);
        const uint64_t head = std::min<uint64_t>(sizes[k], (16 - (addr & 15)) & 15);
        const uint64_t words = (sizes[k] - head) / 16;
        const uint64_t o = (offs ? offs[k] : 0) % lcg::PERIOD; // the stream position of byte j is off + j; positions reduce mod PERIOD
        P.body = static_cast<uint8_t *>(bufs[k]) + head;
        P.head_n = (uint32_t)head;
        P.tail_n = (uint32_t)(sizes[k] - head - words * 16);
        // chunks sit on absolute chunk-aligned addresses: the first starts `lead` bytes before the body, and the kernel
        // counts positions from there, so the base state is stepped back by a^(-lead)
        P.lead = (uint32_t)(reinterpret_cast<uintptr_t>(P.body) & (chunk - 1));
        P.end = P.lead + words * 16;
        P.base_head = lcg::state_residue(key_res, o);
        P.base_body = lcg::mulmod(lcg::state_residue(key_res, o + head), lcg::powmod(lcg::A, lcg::PERIOD - P.lead % lcg::PERIOD));
        P.base_tail = lcg::state_residue(key_res, o + head + (words * 16) % lcg::PERIOD);
        const uint64_t n_chunks = (P.end + chunk - 1) / chunk, first = P.lead != 0 ? 1 : 0;
        if (n_chunks >= (1ull << 24)) return 1;
        a.start[k] = (uint32_t)total;
        total += n_chunks > first ? n_chunks - first : 0; // the cut first chunk is workgroup k's, outside the index space
        bytes += sizes[k];
    }
    for (int k = n; k <= kCycleBatchMax; ++k) a.start[k] = (uint32_t)total;
    a.n_parts = (uint32_t)n;
    const QueuePair q = queue_pair(stream);
    if (!q.pair) return 1;
    a.queue = q.pair;
    a.queue_done = q.done;
    a.queue_seq = q.seq;
    // With chunks handed out by tickets any grid finishes the job, and the memory system does best with fewer
    // streams than CUs: 25 workgroups per 32 CUs (200 on MI355X) -- measured plateau 184..208, +1.6 % at 4 GiB and
    // +2.4 % at 402 MiB over one per CU; 160 and below fall off (profiles/r02_tune_cycle_queue_grid.txt).
    // ... at the clock the chip normally runs at.  While power management holds the shader clock low (the first ~10 ms after
    // load onset) the kernel is bound by its arithmetic instead, and the CUs left idle are worth more than the tidy memory
    // pattern: they get a HELPER workgroup each, which measures the clock when it starts and joins the ticket queue only
    // while it is below MODGPU_HELPER_BELOW_MHZ (default: 77 % of the device's peak shader clock, 1 848 MHz on MI355X; cycle_kernel_impl.h; profiles/r03_first_pass.txt, r03_tune_dvfs.txt).
    uint64_t cap = 0, helpers = 0;
    queue_grid(total, large_grid(), &cap, &helpers);
    const uint64_t main_groups = std::max<uint64_t>(1, std::min<uint64_t>(total, cap));
    a.main_groups = (uint32_t)main_groups;
    a.helper_below_mhz = helper_mode() == 1 ? 0xFFFFFFFFu : helper_below_mhz();
    const uint32_t grid = (uint32_t)(main_groups + helpers);
    // one large buffer: the same launch through the kernel that keeps a slice of it in the Infinity Cache
    const KeepPolicy keep = n != 1 ? KeepPolicy{false, 0u, 0u} : warm_keep ? KeepPolicy{true, kKeepMask, 0u} : keep_policy(bytes);
    hipError_t e;
    if (keep.route) {
        CycleKeepArgs ka{};
        static_cast<CycleQueueArgs &>(ka) = a;
        ka.keep_mask = keep.mask;
        ka.keep_run = keep.run;
        e = modgpu_launch_cycle_keep(ka, grid, stream);
    } else {
        e = modgpu_launch_cycle_queue(a, grid, stream);
    }
    if (e != hipSuccess) {
        queue_pair_unused(q);
        return fail_hip(e, "cycle kernel launch (work queue)");
    }
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    if (n > 1) {
        g_batch_launches.fetch_add(1, std::memory_order_relaxed);
        g_batch_parts.fetch_add((uint64_t)n, std::memory_order_relaxed);
    }
    if (keep.route) t_last_launch = {modgpu_keep_kernel_name(), CYCLE_QUEUE, grid, modgpu_keep_block(), (uint32_t)chunk, bytes, (uint32_t)main_groups, MODGPU_KEEP_KERNEL_SOURCE_HASH};
    else t_last_launch = {modgpu_queue_kernel_name(), n > 1 ? CYCLE_BATCH : CYCLE_QUEUE, grid, modgpu_queue_block(), (uint32_t)chunk, bytes, (uint32_t)main_groups, MODGPU_KERNEL_SOURCE_HASH};
    return MODGPU_OK;
}

} // namespace

int cycle_device_impl(void *dev_buf, uint64_t n, int32_t key, uint64_t stream_off, hipStream_t stream, bool over_pcie)
{
    if (n == 0) return MODGPU_OK;
    if (!dev_buf) return fail(MODGPU_ERR_INVALID, "null device buffer");
    uint32_t key_res = lcg::key_residue(key);
    if (key_res == 0) return MODGPU_OK; // keystream is all zero (state sticks at m): identity
    int variant = choose_variant(dev_buf, n, over_pcie);
    if (variant == CYCLE_QUEUE) {
        const int rc = launch_queue(&dev_buf, &n, &stream_off, 1, key_res, stream);
        if (rc != 1) return rc;
        variant = CYCLE_LARGE; // no ticket pair to be had: the same bursts with the static chunk map
    }
    Plan p = plan_cycle(dev_buf, n, key_res, stream_off, over_pcie, variant);
    hipError_t e = modgpu_launch_cycle(p.args, p.variant, p.grid, stream);
    if (e != hipSuccess) return fail_hip(e, "cycle kernel launch");
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    t_last_launch = {modgpu_variant_kernel_name(p.variant), p.variant, p.grid, modgpu_variant_block(p.variant),
                     modgpu_variant_chunk_bytes(p.variant), n, p.grid, MODGPU_KERNEL_SOURCE_HASH};
    return MODGPU_OK;
}

void note_feed_launch(uint32_t grid, uint64_t bytes)
{
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    t_last_launch = {modgpu_feed_kernel_name(), CYCLE_FEED, grid, modgpu_feed_block(), kFeedPieceBytes, bytes, grid, MODGPU_FEED_KERNEL_SOURCE_HASH};
}
void note_xfer_launch(const char *kernel, uint32_t grid, uint64_t bytes)
{
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    t_last_launch = {kernel, CYCLE_XFER, grid, modgpu_xfer_block(), kFeedPieceBytes, bytes, grid, MODGPU_XFER_KERNEL_SOURCE_HASH};
}
void note_xfer_list_launch(const char *kernel, uint32_t grid, uint64_t bytes, bool digest)
{
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    t_last_launch = {kernel, digest ? CYCLE_XFER_LIST_DIGEST : CYCLE_XFER_LIST, grid, modgpu_xfer_block(), kFeedPieceBytes, bytes, grid, MODGPU_XFER_KERNEL_SOURCE_HASH};
}

// n_parts buffers resident on the CURRENT device, each its own Cycle call (keystream from offs[i], or 0), asynchronous on
// `stream`.  Runs of up to kCycleBatchMax non-empty parts share one launch when that pays (profiles/r03_parts_batched.txt,
// one launch per part against one per run, 2..16 parts of 64 KiB..4 GiB): together beyond the small shape's range -- a
// launch's ~7 us of fixed cost is 5 % of a 411 MB part, and parts of 50-100 MB gain 16-30 % -- or small on average, where
// the per-launch cost is most of the time (16 x 1 MiB: 3x).  Only a few mid-sized parts that together fit the Infinity
// Cache (2 x 64 MiB: -12 %, 4 x 32 MiB: even) are better off with the one-shot small launches.  Everything else is
// launched part by part.
constexpr uint64_t kBatchSmallMean = 24ull << 20;
int cycle_batch_impl(void *const *bufs, const uint64_t *sizes, const uint64_t *offs, int n_parts, int32_t key, hipStream_t stream)
{
    for (int i = 0; i < n_parts; ++i)
        if (sizes[i] && !bufs[i]) return fail(MODGPU_ERR_INVALID, "null device buffer");
    const uint32_t key_res = lcg::key_residue(key);
    if (key_res == 0) return MODGPU_OK;
    int i = 0;
    while (i < n_parts) {
        void *gb[kCycleBatchMax];
        uint64_t gs[kCycleBatchMax], go[kCycleBatchMax], bytes = 0;
        int g = 0;
        for (; i < n_parts && g < kCycleBatchMax; ++i) {
            if (!sizes[i]) continue;
            gb[g] = bufs[i];
            gs[g] = sizes[i];
            go[g] = offs ? offs[i] : 0;
            bytes += sizes[i];
            ++g;
        }
        int rc = 1;
        if (g >= 2 && batch_mode() != 2 && (batch_mode() == 1 || bytes >= kLargeMin || bytes <= kBatchSmallMean * (uint64_t)g))
            rc = launch_queue(gb, gs, go, g, key_res, stream);
        if (rc == 1) {
            rc = MODGPU_OK;
            for (int k = 0; k < g && rc == MODGPU_OK; ++k) rc = cycle_device_impl(gb[k], gs[k], key, go[k], stream);
        }
        if (rc != MODGPU_OK) return rc;
    }
    return MODGPU_OK;
}

// ---- out of place: dst = src ^ keystream (modgpu_cycle_device_to / modgpu_cycle_batch_device_to) ---------------------------------
namespace {
bool ranges_meet(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

// How a source whose phase differs from the destination's by a non-whole number of dwords is read (cycle_to_kernel.h): the funnel,
// measured 1.3-2.2 % faster than unaligned loads at 64 MiB .. 4 GiB (profiles/r07_cycle_to.json)
constexpr int kToFormShipped = CYCLE_TO_FUNNEL;
#ifdef MODGPU_TESTING_HOOKS
std::atomic<int> g_to_form{kToFormShipped}; // modgpu_debug_set_to_form
int to_form() { return g_to_form.load(std::memory_order_relaxed); }
#else
constexpr int to_form() { return kToFormShipped; }
#endif

// Where one out-of-place entry lies on the chunk grid of its DESTINATION (the out-of-place and the rekey kernel share it): < 16 head
// bytes up to the first 16-byte aligned destination byte, a body of whole words whose chunks sit on absolute chunk-aligned addresses
// -- the first starts `lead` bytes before the body, and positions count from there --, and < 16 tail bytes.
struct EntryGeom {
    uint64_t head, words, tail;
    uint32_t lead;
    uint64_t end;      // lead + body bytes
    uint64_t n_chunks; // chunks from the chunk origin, the cut first one included
    uint64_t first;    // 1 if the first chunk is cut (it is the entry's own workgroup's, outside the index space)
};
EntryGeom entry_geom(const uint8_t *dst, uint64_t size, uint64_t chunk)
{
    EntryGeom g;
    g.head = std::min<uint64_t>(size, (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
    g.words = (size - g.head) / 16;
    g.tail = size - g.head - g.words * 16;
    g.lead = (uint32_t)(reinterpret_cast<uintptr_t>(dst + g.head) & (chunk - 1));
    g.end = g.lead + g.words * 16;
    g.n_chunks = (g.end + chunk - 1) / chunk;
    g.first = g.lead != 0 ? 1 : 0;
    return g;
}
// The three base states of a keystream from stream position o (< PERIOD) over an entry: head, body (stepped back by a^(-lead) to the
// chunk origin), tail.
void entry_bases(const EntryGeom &g, uint32_t key_res, uint64_t o, uint32_t &head, uint32_t &body, uint32_t &tail)
{
    head = lcg::state_residue(key_res, o);
    body = lcg::mulmod(lcg::state_residue(key_res, o + g.head), lcg::powmod(lcg::A, lcg::PERIOD - g.lead % lcg::PERIOD));
    tail = lcg::state_residue(key_res, o + g.head + (g.words * 16) % lcg::PERIOD);
}

// One run of an entry-list call: up to kCycleBatchMax non-empty entries of the current device, gathered from the caller's arrays.
// `role` is the pointer the chunk grid lies on: the destination (out of place, rekey), expect (the verifying calls), and for a digest
// entry its destination if it has one, else its source.  Offsets are as the caller gave them (no list: 0); plan_entries' binders reduce them.
struct EntryRun {
    int n = 0;
    int idx[kCycleBatchMax]; // where each entry stands in the caller's arrays
    uint8_t *role[kCycleBatchMax];
    const uint8_t *src[kCycleBatchMax];
    uint64_t size[kCycleBatchMax], off[2][kCycleBatchMax];
};

// The run loop of the five entry-list calls: fn(run) for each run of up to kCycleBatchMax non-empty entries that `keep` accepts, in the
// caller's order, until one fails.  `role` may be null, and so may its entries, only where the check let that pass (digest): the source
// stands in (it is never stored through).
template <class Keep, class Fn>
int for_each_run(const void *const *role, const void *const *src, const uint64_t *sizes, const uint64_t *offs_a, const uint64_t *offs_b, int n,
                 Keep keep, Fn fn)
{
    EntryRun r;
    for (int i = 0; i < n;) {
        for (r.n = 0; i < n && r.n < kCycleBatchMax; ++i) {
            if (!sizes[i] || !keep(i)) continue;
            const int k = r.n++;
            r.idx[k] = i;
            r.role[k] = const_cast<uint8_t *>(static_cast<const uint8_t *>(role && role[i] ? role[i] : src[i]));
            r.src[k] = static_cast<const uint8_t *>(src[i]);
            r.size[k] = sizes[i];
            r.off[0][k] = offs_a ? offs_a[i] : 0;
            r.off[1][k] = offs_b ? offs_b[i] : 0;
        }
        if (r.n == 0) break;
        if (const int rc = fn(r)) return rc;
    }
    return MODGPU_OK;
}
constexpr auto every_entry = [](int) { return true; };

// The entry planner: every part's geometry on the chunk grid of its role pointer, the chunk index space start[] with its padding, and
// n_parts.  bind(P, k, g) fills what only that call has: the role pointer's field, its base states (entry_bases, one set or two, or none
// for an identity keystream: the zeroes stay), its result.  `oversized`: an entry beyond the kernels' three-byte chunk jump tables.
struct EntryPlan {
    uint64_t total = 0, bytes = 0;
    bool misaligned = false, oversized = false;
};
template <class Args, class Bind> EntryPlan plan_entries(Args &a, const EntryRun &r, uint64_t chunk, Bind bind)
{
    EntryPlan p;
    for (int k = 0; k < r.n; ++k) {
        auto &P = a.part[k];
        const EntryGeom g = entry_geom(r.role[k], r.size[k], chunk);
        P.src_body = r.src[k] + g.head;
        P.head_n = (uint32_t)g.head;
        P.tail_n = (uint32_t)g.tail;
        P.lead = g.lead;
        P.end = g.end;
        bind(P, k, g);
        a.start[k] = (uint32_t)p.total;
        p.total += g.n_chunks > g.first ? g.n_chunks - g.first : 0;
        p.bytes += r.size[k];
        // a source whose phase differs from the role pointer's by a whole number of dwords needs no funnel: dword-aligned dwordx4 loads
        p.misaligned |= g.words != 0 && ((reinterpret_cast<uintptr_t>(r.src[k]) - reinterpret_cast<uintptr_t>(r.role[k])) & 3) != 0;
        p.oversized |= g.n_chunks >= (1ull << 24);
    }
    for (int k = r.n; k <= kCycleBatchMax; ++k) a.start[k] = (uint32_t)p.total;
    a.n_parts = (uint32_t)r.n;
    return p;
}
// The work-queue kernel's grid cap, main workgroups only: 25 per 32 CUs (cycle_kernel.hip)
uint64_t queue_cap(uint64_t total)
{
    uint64_t cap = 0, helpers = 0;
    queue_grid(total, large_grid(), &cap, &helpers);
    return cap;
}
// ... and no grid has more workgroups than there are chunks
uint32_t entry_grid(uint64_t total, uint64_t cap) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(total, cap)); }
// After an entry launch: its error (`ticket`: the ring line a ticketed kernel drew and nobody will sign off), or the count and the report.
int entry_launched(hipError_t e, const char *what, const QueuePair *ticket, const char *kernel, int variant, uint32_t grid, uint32_t block,
                   uint64_t chunk, uint64_t bytes, const char *source_hash)
{
    if (e != hipSuccess) {
        if (ticket) queue_pair_unused(*ticket);
        return fail_hip(e, what);
    }
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    t_last_launch = {kernel, variant, grid, block, (uint32_t)chunk, bytes, grid, source_hash};
    return MODGPU_OK;
}

// One launch of the out-of-place kernel over a run.  MODGPU_OK, an error, or 1: no ticket pair to be had right now (or an entry beyond
// the three-byte chunk jump tables): the caller copies and cycles in place.
int launch_to(const EntryRun &r, uint32_t key_res, hipStream_t stream)
{
    CycleToArgs a{};
    const uint64_t chunk = modgpu_to_chunk_bytes();
    const EntryPlan p = plan_entries(a, r, chunk, [&](CycleToPart &P, int k, const EntryGeom &g) {
        P.dst_body = r.role[k] + g.head;
        entry_bases(g, key_res, r.off[0][k] % lcg::PERIOD, P.base_head, P.base_body, P.base_tail);
    });
    if (p.oversized) return 1;
    const QueuePair q = queue_pair(stream);
    if (!q.pair) return 1;
    a.queue = q.pair;
    a.queue_done = q.done;
    a.queue_seq = q.seq;
    const uint32_t grid = entry_grid(p.total, queue_cap(p.total));
    const int form = p.misaligned ? to_form() : CYCLE_TO_PLAIN;
    return entry_launched(modgpu_launch_cycle_to(a, form, grid, stream), "cycle kernel launch (out of place)", &q, modgpu_to_kernel_name(form), CYCLE_TO,
                          grid, modgpu_to_block(), chunk, p.bytes, MODGPU_TO_KERNEL_SOURCE_HASH);
}

// The rules of one entry that writes: a source, and a destination that is its source or lies clear of it.  (No destination at all -- d
// null -- is the digest call's entry that only reads.)
int check_to_entry(const void *d, const void *s, uint64_t size)
{
    if (!s) return fail(MODGPU_ERR_INVALID, "null buffer");
    if (d && d != s && ranges_meet(d, size, s, size)) return fail(MODGPU_ERR_INVALID, "destination partly overlaps its source (only dst == src may alias)");
    return MODGPU_OK;
}
// ... and of the entries among each other: no destination meets any OTHER entry's source or destination (sources may overlap each other:
// they are only read).  `dst` may be null, and so may its entries, where the caller let that pass.
int check_to_meetings(void *const *dst, const void *const *src, const uint64_t *sizes, int n)
{
    auto d = [&](int i) -> const void * { return dst && sizes[i] ? dst[i] : nullptr; };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (i != j && d(i) && (ranges_meet(d(i), sizes[i], src[j], sizes[j]) || (d(j) && ranges_meet(d(i), sizes[i], d(j), sizes[j]))))
                return fail(MODGPU_ERR_INVALID, "a destination meets another entry's source or destination");
    return MODGPU_OK;
}
// The checks of the out-of-place and the rekey calls, before any device work: the lists, a null pointer with bytes to move, and the two
// rules above.
int check_to_entries(void *const *dst, const void *const *src, const uint64_t *sizes, int n)
{
    if (n < 0 || (n > 0 && (!dst || !src || !sizes))) return fail(MODGPU_ERR_INVALID, "bad entry list");
    for (int i = 0; i < n; ++i) {
        if (!sizes[i]) continue;
        if (!dst[i]) return fail(MODGPU_ERR_INVALID, "null buffer");
        if (int rc = check_to_entry(dst[i], src[i], sizes[i])) return rc;
    }
    return check_to_meetings(dst, src, sizes, n);
}
// What the calls with results check of them, and of an entry's span: their kernels have no second route for an entry beyond the chunk
// jump tables (the kernel jumps to a chunk's keystream state by the three bytes of its index in the entry).
int check_results(int n, const void *results)
{
    if (n > 0 && !results) return fail(MODGPU_ERR_INVALID, "null result");
    if (reinterpret_cast<uintptr_t>(results) & 7) return fail(MODGPU_ERR_INVALID, "result not 8-byte aligned");
    return MODGPU_OK;
}
int check_entry_span(const void *role, uint64_t size, uint64_t chunk)
{
    if (size >= (1ull << 41) || entry_geom(static_cast<const uint8_t *>(role), size, chunk).n_chunks >= (1ull << 24))
        return fail(MODGPU_ERR_INVALID, "an entry that spans 2^24 chunks of 64 KiB or more (1 TiB)");
    return MODGPU_OK;
}

// Entries already checked (check_to_entries), on the current device, asynchronous on `stream`.  Runs of up to kCycleBatchMax
// non-empty entries share one launch.  Keys == 0 mod m have the identity keystream: out of place that is a copy.  With no ticket
// pair free, each entry of the run is copied (hipMemcpyAsync, capturable) and cycled in place on the same stream.
int cycle_to_impl(void *const *dst, const void *const *src, const uint64_t *sizes, const uint64_t *offs, int n, int32_t key, hipStream_t stream)
{
    const uint32_t key_res = lcg::key_residue(key);
    return for_each_run(dst, src, sizes, offs, nullptr, n, every_entry, [&](const EntryRun &r) {
        int rc = key_res ? launch_to(r, key_res, stream) : 1;
        if (rc == 1) {
            rc = MODGPU_OK;
            for (int k = 0; k < r.n && rc == MODGPU_OK; ++k) {
                if (r.role[k] != r.src[k]) {
                    const hipError_t e = hipMemcpyAsync(r.role[k], r.src[k], r.size[k], hipMemcpyDefault, stream);
                    if (e != hipSuccess) return fail_hip(e, "hipMemcpyAsync (out of place)");
                }
                if (key_res) rc = cycle_device_impl(r.role[k], r.size[k], key, r.off[0][k], stream);
            }
        }
        return rc;
    });
}

// ---- rekey: dst = src ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j] (modgpu_rekey_device_to / modgpu_rekey_batch_device_to) ----
// Launch shape (cycle_rekey_kernel.h): one workgroup per CU on every CU.  Two keystreams make the pass VALU-bound on the out-of-place
// kernel's 200 workgroups (5.92 TB/s at 4 GiB); on all 256 it sits at the HBM ceiling (6.99, against 7.04 for one keystream) --
// DESIGN.md 4.7, profiles/r08_rekey.json.
constexpr int kRekeyShapeShipped = CYCLE_REKEY_SHAPE_ALL;
#ifdef MODGPU_TESTING_HOOKS
std::atomic<int> g_rekey_shape{kRekeyShapeShipped}; // modgpu_debug_set_rekey_form
int rekey_shape() { return g_rekey_shape.load(std::memory_order_relaxed); }
#else
constexpr int rekey_shape() { return kRekeyShapeShipped; }
#endif

// One launch of the rekey kernel over a run, both keys non-zero residues.  MODGPU_OK, an error, or 1: no ticket pair to be had right
// now (or an entry beyond the three-byte chunk jump tables).
// `own_pair`: a clean ticket pair of the caller's (the move call's workspace header) instead of one of the ring's.
int launch_rekey(const EntryRun &r, uint32_t key_from, uint32_t key_to, hipStream_t stream, uint32_t *own_pair = nullptr)
{
    CycleRekeyArgs a{};
    const uint64_t chunk = modgpu_rekey_chunk_bytes();
    const EntryPlan p = plan_entries(a, r, chunk, [&](CycleRekeyPart &P, int k, const EntryGeom &g) {
        P.dst_body = r.role[k] + g.head;
        // two keystreams, two sets of bases on the same positions: differing offsets change nothing else
        entry_bases(g, key_from, r.off[0][k] % lcg::PERIOD, P.base_head[0], P.base_body[0], P.base_tail[0]);
        entry_bases(g, key_to, r.off[1][k] % lcg::PERIOD, P.base_head[1], P.base_body[1], P.base_tail[1]);
    });
    if (p.oversized) return 1;
    QueuePair q;
    if (own_pair) {
        q.pair = own_pair;
    } else {
        q = queue_pair(stream);
        if (!q.pair) return 1;
    }
    a.queue = q.pair;
    a.queue_done = q.done;
    a.queue_seq = q.seq;
    const uint32_t grid = entry_grid(p.total, rekey_shape() == CYCLE_REKEY_SHAPE_ALL ? large_grid() : queue_cap(p.total));
    const int form = p.misaligned ? CYCLE_REKEY_FUNNEL : CYCLE_REKEY_PLAIN;
    return entry_launched(modgpu_launch_cycle_rekey(a, form, grid, stream), "cycle kernel launch (rekey)", &q, modgpu_rekey_kernel_name(form), CYCLE_REKEY,
                          grid, modgpu_rekey_block(), chunk, p.bytes, MODGPU_REKEY_KERNEL_SOURCE_HASH);
}

// The rekey calls' degenerate keystreams, entry by entry: the same reduced key at the same stream position has ks ^ ks = 0.
struct SameStream {
    bool same_key;
    const uint64_t *offs_from, *offs_to;
    static uint64_t at(const uint64_t *offs, int i) { return offs ? offs[i] % lcg::PERIOD : 0; }
    bool operator()(int i) const { return same_key && at(offs_from, i) == at(offs_to, i); }
};

// Entries already checked (check_to_entries), on the current device, asynchronous on `stream`.  Degenerate keystreams take the
// out-of-place call: a key == 0 mod m has the identity keystream, so only the other key is left to apply (both zero: a copy); an
// entry with the same reduced key at the same stream position has ks ^ ks = 0 and is copied.  The rest run in groups of up to
// kCycleBatchMax per launch; with no ticket pair free a group is done in two passes on the same stream, out of place under key_from,
// then in place under key_to.
int rekey_impl(void *const *dst, const void *const *src, const uint64_t *sizes, const uint64_t *offs_from, const uint64_t *offs_to, int n,
               int32_t key_from, int32_t key_to, hipStream_t stream)
{
    const uint32_t kf = lcg::key_residue(key_from), kt = lcg::key_residue(key_to);
    if (!kf) return cycle_to_impl(dst, src, sizes, offs_to, n, key_to, stream); // (key_to == 0 too: a copy)
    if (!kt) return cycle_to_impl(dst, src, sizes, offs_from, n, key_from, stream);
    const SameStream identity{kf == kt, offs_from, offs_to};
    for (int i = 0; i < n; ++i)
        if (sizes[i] && identity(i))
            if (int rc = cycle_to_impl(&dst[i], &src[i], &sizes[i], nullptr, 1, 0, stream)) return rc;
    return for_each_run(dst, src, sizes, offs_from, offs_to, n, [&](int i) { return !identity(i); }, [&](const EntryRun &r) {
        int rc = launch_rekey(r, kf, kt, stream);
        if (rc == 1) {
            rc = MODGPU_OK;
            for (int k = 0; k < r.n && rc == MODGPU_OK; ++k) {
                void *d = r.role[k];
                const void *s = r.src[k];
                rc = cycle_to_impl(&d, &s, &r.size[k], &r.off[0][k], 1, key_from, stream);
                if (rc == MODGPU_OK) rc = cycle_device_impl(d, r.size[k], key_to, r.off[1][k], stream);
            }
        }
        return rc;
    });
}


// ---- move: rekey with memmove rules, any overlap of destination and source (modgpu_rekey_move_device) ----
// The workspace: a header line -- words 0, 1 the ticket pair, word kMoveStatusWord the status (0, or 1 + the stalled chunk) --, one
// 32-bit flag per chunk the body can have, and scratch for the ragged pieces: a head of less than a chunk (or all of a range whose
// body is empty: less than a chunk + 16 bytes) and a tail of less than 16 bytes.
constexpr uint64_t kMoveHdrBytes = 128;
constexpr uint32_t kMoveStatusWord = 16; // (a line of the pair's own would be wasted: the word is written by a pass that has failed)
constexpr uint64_t kMoveMaxChunks = 1ull << 24;
struct MoveLayout {
    uint64_t flags, head, tail, bytes;
};
MoveLayout move_layout(uint64_t n)
{
    const uint64_t chunk = modgpu_rekey_chunk_bytes();
    MoveLayout L;
    L.flags = kMoveHdrBytes;
    L.head = L.flags + ((n / chunk + 2) * sizeof(uint32_t) + 127) / 128 * 128;
    L.tail = L.head + chunk + 64;
    L.bytes = L.tail + 64;
    return L;
}
#ifdef MODGPU_TESTING_HOOKS
std::atomic<uint32_t> g_move_grid{0}; // modgpu_debug_set_move_grid
uint32_t move_grid_forced() { return g_move_grid.load(std::memory_order_relaxed); }
#else
constexpr uint32_t move_grid_forced() { return 0; }
#endif

// The chunks, other than chunk c itself, whose source reads meet chunk c's destination: c + lo .. c + lo + count - 1.  delta = src -
// dst.  A chunk's reads span its source rounded out to whole dwords of the SOURCE (the funnel form reads the dword below a misaligned
// start and the one that holds the last byte; the body's destination is chunk-aligned, so delta's phase mod 4 is the source's).
// Rounded like that no chunk's reads reach below its own destination when delta > 0, nor above it when delta < 0: every chunk of the
// window lies on the side the move walks AWAY from, at a lower position.
void move_window(int64_t delta, int64_t chunk, int32_t *lo, uint32_t *count)
{
    const int64_t dlo = delta - ((delta % 4 + 4) % 4), dhi = dlo + (delta % 4 != 0 ? 4 : 0);
    const int64_t mid = dlo >= 0 ? -(dlo / chunk) : (-dlo + chunk - 1) / chunk; // about -delta / chunk
    *lo = 0;
    *count = 0;
    for (int64_t m = mid - 3; m <= mid + 3; ++m) {
        // chunk c + m reads [m * chunk + dlo, (m + 1) * chunk + dhi) counted from chunk c's first destination byte
        if (m == 0 || !(m * chunk + dlo < chunk && (m + 1) * chunk + dhi > 0)) continue;
        if (!*count) *lo = (int32_t)m;
        ++*count;
    }
}

// The launches of a move whose ranges partly overlap, both keys non-zero residues, offsets already reduced: memset, pieces into
// scratch, body, pieces into place.
int move_launches(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t kf, uint64_t of, uint32_t kt, uint64_t ot, uint8_t *ws, const MoveLayout &L,
                  hipStream_t stream)
{
    const uint64_t chunk = modgpu_rekey_chunk_bytes();
    uint64_t head = std::min<uint64_t>(n, (chunk - (reinterpret_cast<uintptr_t>(dst) & (chunk - 1))) & (chunk - 1));
    uint64_t body = (n - head) & ~15ull, tail = n - head - body;
    if (body == 0) { // all of it goes through scratch
        head = n;
        tail = 0;
    }
    uint32_t *const hdr = reinterpret_cast<uint32_t *>(ws);
    (void)hipGetLastError();
    HIP_TRY(hipMemsetAsync(ws, 0, L.head, stream)); // header and flags
    // the pieces are READ first: nothing of the source has been written yet
    if (head || tail) {
        EntryRun r;
        auto piece = [&](uint8_t *d, uint64_t at, uint64_t len) {
            const int k = r.n++;
            r.role[k] = d, r.src[k] = src + at, r.size[k] = len, r.off[0][k] = of + at, r.off[1][k] = ot + at;
        };
        if (head) piece(ws + L.head, 0, head);
        if (tail) piece(ws + L.tail, head + body, tail);
        const int rc = launch_rekey(r, kf, kt, stream, hdr);
        if (rc != MODGPU_OK) return rc == 1 ? fail(MODGPU_ERR_INVALID, "move: a ragged piece beyond the chunk tables") : rc;
    }
    if (body) {
        CycleRekeyArgs a{};
        CycleRekeyPart &P = a.part[0];
        P.dst_body = dst + head;
        P.src_body = src + head;
        P.end = body;
        P.base_body[0] = lcg::state_residue(kf, of + head);
        P.base_body[1] = lcg::state_residue(kt, ot + head);
        const uint64_t total = (body + chunk - 1) / chunk;
        for (int k = 1; k <= kCycleBatchMax; ++k) a.start[k] = (uint32_t)total;
        a.n_parts = 1;
        a.queue = hdr;
        a.move_flags = reinterpret_cast<uint32_t *>(ws + L.flags);
        a.move_status = hdr + kMoveStatusWord;
        a.move_down = dst > src ? 1u : 0u;
        const int64_t delta = (int64_t)(reinterpret_cast<uintptr_t>(src) - reinterpret_cast<uintptr_t>(dst));
        move_window(delta, (int64_t)chunk, &a.move_win_lo, &a.move_win_n);
        if (a.move_win_n > 3 || (a.move_win_n && (delta > 0 ? a.move_win_lo + (int32_t)a.move_win_n > 0 : a.move_win_lo < 1)))
            return fail(MODGPU_ERR_INVALID, "move: internal error (a chunk would wait for a later one)");
        // the rekey call's grid; every position is a ticket, so the pass needs no workgroup that is not running, but a grid the
        // device holds at once wastes none (modgpu_launch_cycle_rekey_move caps it)
        uint32_t grid = entry_grid(total, move_grid_forced() ? move_grid_forced() : rekey_shape() == CYCLE_REKEY_SHAPE_ALL ? large_grid() : queue_cap(total));
        const int form = (delta & 3) != 0 ? CYCLE_REKEY_FUNNEL : CYCLE_REKEY_PLAIN;
        const hipError_t e = modgpu_launch_cycle_rekey_move(a, form, &grid, stream);
        if (e != hipSuccess) return fail_hip(e, "cycle kernel launch (move)");
        g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
        t_last_launch = {modgpu_rekey_kernel_name(form), CYCLE_REKEY_MOVE, grid, modgpu_rekey_block(), (uint32_t)chunk, n, grid, MODGPU_REKEY_KERNEL_SOURCE_HASH};
    }
    if (head) HIP_TRY(hipMemcpyAsync(dst, ws + L.head, head, hipMemcpyDeviceToDevice, stream));
    if (tail) HIP_TRY(hipMemcpyAsync(dst + head + body, ws + L.tail, tail, hipMemcpyDeviceToDevice, stream));
    return MODGPU_OK;
}

// One fixed non-zero key at one offset on both sides: ks ^ ks = 0, the two-keystream block as a bit-exact memmove
constexpr uint32_t kMovePlainKey = 1u;

int rekey_move_impl(void *dev_dst, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to, uint64_t off_to, void *ws,
                    uint64_t ws_bytes, int device, hipStream_t stream)
{
    if (n == 0) return MODGPU_OK;
    if (!dev_dst || !dev_src) return fail(MODGPU_ERR_INVALID, "null buffer");
    const uint64_t chunk = modgpu_rekey_chunk_bytes();
    if (n >= kMoveMaxChunks * chunk || entry_geom(static_cast<const uint8_t *>(dev_dst), n, chunk).n_chunks >= kMoveMaxChunks)
        return fail(MODGPU_ERR_INVALID, "an entry of 2^24 chunks or more (the move call's limit)");
    if (!ws) return fail(MODGPU_ERR_INVALID, "null workspace");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(MODGPU_ERR_INVALID, "workspace not 8-byte aligned");
    const MoveLayout L = move_layout(n);
    if (ws_bytes < L.bytes) return fail(MODGPU_ERR_INVALID, "workspace smaller than modgpu_move_workspace_bytes(n)");
    if (ranges_meet(ws, L.bytes, dev_dst, n) || ranges_meet(ws, L.bytes, dev_src, n))
        return fail(MODGPU_ERR_INVALID, "the workspace meets the destination or the source");
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    int phys = -1;
    HIP_TRY(hipGetDevice(&phys));
    if (modgpu_xfer_device_of(ws, L.bytes) != phys) return fail(MODGPU_ERR_INVALID, "the workspace is not device memory of the call's device");
    if (dev_dst == dev_src || !ranges_meet(dev_dst, n, dev_src, n)) {
        // (the header is reset on this route too: modgpu_move_status speaks of the LAST call on the workspace, whatever its route)
        HIP_TRY(hipMemsetAsync(ws, 0, kMoveHdrBytes, stream));
        return rekey_impl(&dev_dst, &dev_src, &n, &off_from, &off_to, 1, key_from, key_to, stream);
    }
    if (modgpu_xfer_device_of(dev_dst, n) != phys || modgpu_xfer_device_of(dev_src, n) != phys)
        return fail(MODGPU_ERR_INVALID, "overlapping ranges that are not device memory of the call's device");
    uint8_t *const d = static_cast<uint8_t *>(dev_dst), *const w = static_cast<uint8_t *>(ws);
    const uint8_t *const s = static_cast<const uint8_t *>(dev_src);
    const uint32_t kf = lcg::key_residue(key_from), kt = lcg::key_residue(key_to);
    const uint64_t of = off_from % lcg::PERIOD, ot = off_to % lcg::PERIOD;
    if (kf && kt && !(kf == kt && of == ot)) return move_launches(d, s, n, kf, of, kt, ot, w, L, stream);
    // keystreams that cancel or are both the identity: a plain move; exactly one identity: the move, then the other key in place
    if (int rc = move_launches(d, s, n, kMovePlainKey, 0, kMovePlainKey, 0, w, L, stream)) return rc;
    if (!kf != !kt) return kf ? cycle_device_impl(d, n, key_from, off_from, stream) : cycle_device_impl(d, n, key_to, off_to, stream);
    return MODGPU_OK;
}

// ---- verify: count and locate the j with expect[j] != (src[j] ^ ks(key)[off + j]) (modgpu_verify_device / modgpu_verify_batch_device) ----
// Launch shape (cycle_verify_kernel.h): static chunk assignment on one workgroup per CU.  No ticket pair is drawn, so there is nothing
// to run out of and no second route -- DESIGN.md 4.10, profiles/r11_verify.json.
static_assert(sizeof(modgpu_verify_result_t) == sizeof(CycleVerifyResult) && sizeof(modgpu_verify_result_t) == 32 &&
                  offsetof(modgpu_verify_result_t, first_mismatch) == offsetof(CycleVerifyResult, first_mismatch) &&
                  offsetof(modgpu_verify_result_t, n) == offsetof(CycleVerifyResult, n) &&
                  offsetof(modgpu_verify_result_t, reserved) == offsetof(CycleVerifyResult, reserved),
              "the kernels' result record is the public one");
#ifdef MODGPU_TESTING_HOOKS
std::atomic<uint32_t> g_verify_grid{0}; // modgpu_debug_set_verify_form
uint32_t verify_grid_forced() { return g_verify_grid.load(std::memory_order_relaxed); }
#else
constexpr uint32_t verify_grid_forced() { return 0; }
#endif

// One compare launch over a run (key_res == 0: the identity forms); result r.idx[k] of `results` is entry k's.
int launch_verify(const EntryRun &r, modgpu_verify_result_t *results, uint32_t key_res, hipStream_t stream)
{
    CycleVerifyArgs a{};
    const uint64_t chunk = modgpu_verify_chunk_bytes();
    const EntryPlan p = plan_entries(a, r, chunk, [&](CycleVerifyPart &P, int k, const EntryGeom &g) {
        P.expect_body = r.role[k] + g.head;
        P.result = reinterpret_cast<CycleVerifyResult *>(results + r.idx[k]);
        P.n = r.size[k];
        if (key_res) entry_bases(g, key_res, r.off[0][k] % lcg::PERIOD, P.base_head, P.base_body, P.base_tail);
    });
    const uint32_t grid = entry_grid(p.total, verify_grid_forced() ? verify_grid_forced() : large_grid());
    const int form = (p.misaligned ? CYCLE_VERIFY_FUNNEL : CYCLE_VERIFY_PLAIN) | (key_res ? 0 : CYCLE_VERIFY_IDENTITY);
    return entry_launched(modgpu_launch_cycle_verify(a, form, grid, stream), "verify kernel launch", nullptr, modgpu_verify_kernel_name(form), CYCLE_VERIFY,
                          grid, modgpu_verify_block(), chunk, p.bytes, MODGPU_VERIFY_KERNEL_SOURCE_HASH);
}

// Everything that is checked before a device is looked at.
int check_verify_entries(const void *const *expect, const void *const *src, const uint64_t *sizes, int n, const modgpu_verify_result_t *results)
{
    if (n < 0 || (n > 0 && (!expect || !src || !sizes))) return fail(MODGPU_ERR_INVALID, "bad entry list");
    if (int rc = check_results(n, results)) return rc;
    for (int i = 0; i < n; ++i) {
        if (!sizes[i]) continue;
        if (!expect[i] || !src[i]) return fail(MODGPU_ERR_INVALID, "null buffer");
        if (int rc = check_entry_span(expect[i], sizes[i], modgpu_verify_chunk_bytes())) return rc;
    }
    return MODGPU_OK;
}

// What the calls with results do before their first launch, n > 0: the records are device memory of the call's device, an earlier
// call's error is cleared (the launches report hipGetLastError: it must not be taken for theirs), and the records are made clean on the
// call's own stream -- the verify record by a launch (first_mismatch starts at all ones) ...
int results_on_device(const void *results, uint64_t bytes)
{
    int phys = -1;
    HIP_TRY(hipGetDevice(&phys));
    if (modgpu_xfer_device_of(results, bytes) != phys) return fail(MODGPU_ERR_INVALID, "the result is not device memory of the call's device");
    return MODGPU_OK;
}
int prepare_results(modgpu_verify_result_t *results, int n, hipStream_t stream)
{
    if (int rc = results_on_device(results, (uint64_t)n * sizeof *results)) return rc;
    (void)hipGetLastError();
    const hipError_t e = modgpu_launch_verify_init(reinterpret_cast<CycleVerifyResult *>(results), (uint64_t)n, stream);
    if (e != hipSuccess) return fail_hip(e, "verify init launch");
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    t_last_launch = {"modgpu_cycle_verify_init", CYCLE_VERIFY, (uint32_t)(((uint64_t)n + 255) / 256), 256u, 0u, 0, 0u, MODGPU_VERIFY_KERNEL_SOURCE_HASH};
    return MODGPU_OK;
}
// ... and the digest record by a memset (a node of a capture, so a replay starts clean), which comes before the clearing.
int prepare_results(modgpu_digest_result_t *results, int n, hipStream_t stream)
{
    if (int rc = results_on_device(results, (uint64_t)n * sizeof *results)) return rc;
    HIP_TRY(hipMemsetAsync(results, 0, (size_t)n * sizeof *results, stream));
    (void)hipGetLastError();
    return MODGPU_OK;
}

// Entries already checked (check_verify_entries), on the current device, asynchronous on `stream`: one launch initialises all n results,
// then runs of up to kCycleBatchMax non-empty entries share a compare launch.
int verify_impl(const void *const *expect, const void *const *src, const uint64_t *sizes, const uint64_t *offs, int n, int32_t key,
                modgpu_verify_result_t *results, hipStream_t stream)
{
    if (n == 0) return MODGPU_OK;
    if (int rc = prepare_results(results, n, stream)) return rc;
    const uint32_t key_res = lcg::key_residue(key);
    return for_each_run(expect, src, sizes, offs, nullptr, n, every_entry, [&](const EntryRun &r) { return launch_verify(r, results, key_res, stream); });
}

// ---- digest: Adler-32 of out[j] = src[j] ^ ks(key)[off + j], with or without storing out (modgpu_digest_device / modgpu_digest_batch_device) ----
// The out-of-place kernels' digest loop (cycle_to_kernel.h): static chunk assignment on one workgroup per CU, like verify.  No ticket
// pair is drawn, so there is nothing to run out of and no second route -- DESIGN.md 4.16, profiles/r16_digest.json.
static_assert(sizeof(modgpu_digest_result_t) == sizeof(CycleToDigest) && sizeof(modgpu_digest_result_t) == 32 &&
                  offsetof(modgpu_digest_result_t, s2) == offsetof(CycleToDigest, s2) && offsetof(modgpu_digest_result_t, n) == offsetof(CycleToDigest, n) &&
                  offsetof(modgpu_digest_result_t, reserved) == offsetof(CycleToDigest, reserved),
              "the kernel's record is the public one");
static_assert(sizeof(CycleToArgs) <= 4096, "the table of entries travels in the kernel arguments");
#ifdef MODGPU_TESTING_HOOKS
std::atomic<uint32_t> g_digest_grid{0}; // modgpu_debug_set_digest_grid
uint32_t digest_grid_forced() { return g_digest_grid.load(std::memory_order_relaxed); }
#else
constexpr uint32_t digest_grid_forced() { return 0; }
#endif

// One digest launch over a run (key_res == 0: out = src); record r.idx[k] of `results` is entry k's.  An entry without a destination
// (`dst` null, or its entry) is planned with its source in the destination's role: the chunk grid lies on the source, whose phase
// against itself is 0.
int launch_digest(const EntryRun &r, void *const *dst, modgpu_digest_result_t *results, uint32_t key_res, hipStream_t stream)
{
    CycleToArgs a{};
    const uint64_t chunk = modgpu_to_chunk_bytes();
    const EntryPlan p = plan_entries(a, r, chunk, [&](CycleToPart &P, int k, const EntryGeom &g) {
        P.dst_body = r.role[k] + g.head;
        if (key_res) entry_bases(g, key_res, r.off[0][k] % lcg::PERIOD, P.base_head, P.base_body, P.base_tail);
        a.result[k] = reinterpret_cast<CycleToDigest *>(results + r.idx[k]);
        if (dst && dst[r.idx[k]]) a.store_mask |= 1u << k;
    });
    a.digest = CYCLE_TO_DIGEST_ON | (key_res ? 0u : CYCLE_TO_DIGEST_IDENTITY);
    // digest only: one workgroup per CU, as verify (a read-only stream).  A launch that stores takes the out-of-place kernel's grid,
    // 25 workgroups per 32 CUs (cycle_kernel.hip: the memory system does best with fewer read/write streams than CUs)
    const uint32_t grid = entry_grid(p.total, digest_grid_forced() ? digest_grid_forced() : a.store_mask ? queue_cap(p.total) : large_grid());
    const int form = p.misaligned ? to_form() : CYCLE_TO_PLAIN;
    return entry_launched(modgpu_launch_cycle_to_digest(a, form, grid, stream), "digest kernel launch", nullptr, modgpu_to_kernel_name(form), CYCLE_TO_DIGEST,
                          grid, modgpu_to_block(), chunk, p.bytes, MODGPU_TO_KERNEL_SOURCE_HASH);
}

// Everything that is checked before a device is looked at.  `dst` may be null (digest only), and so may any of its entries; an entry
// that has a destination keeps the out-of-place rules (check_to_entry, check_to_meetings).
int check_digest_entries(void *const *dst, const void *const *src, const uint64_t *sizes, int n, const modgpu_digest_result_t *results)
{
    if (n < 0 || (n > 0 && (!src || !sizes))) return fail(MODGPU_ERR_INVALID, "bad entry list");
    if (int rc = check_results(n, results)) return rc;
    for (int i = 0; i < n; ++i) {
        if (!sizes[i]) continue;
        const void *const d = dst ? dst[i] : nullptr;
        if (int rc = check_to_entry(d, src[i], sizes[i])) return rc;
        if (int rc = check_entry_span(d ? d : src[i], sizes[i], modgpu_to_chunk_bytes())) return rc;
    }
    return check_to_meetings(dst, src, sizes, n);
}

// Entries already checked (check_digest_entries), on the current device, asynchronous on `stream`: all n records are zeroed on the
// call's own stream, then runs of up to kCycleBatchMax non-empty entries share a launch.
int digest_impl(void *const *dst, const void *const *src, const uint64_t *sizes, const uint64_t *offs, int n, int32_t key,
                modgpu_digest_result_t *results, hipStream_t stream)
{
    if (n == 0) return MODGPU_OK;
    if (int rc = prepare_results(results, n, stream)) return rc;
    const uint32_t key_res = lcg::key_residue(key);
    return for_each_run(dst, src, sizes, offs, nullptr, n, every_entry, [&](const EntryRun &r) { return launch_digest(r, dst, results, key_res, stream); });
}


// ---- rekey verify: count and locate the j with expect[j] != (src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j])
// (modgpu_verify_rekey_device / modgpu_verify_rekey_batch_device) ----
// One two-keystream compare launch over 1..kCycleBatchMax non-empty entries of the current device, both keys non-zero residues:
// launch_verify's geometry with two sets of bases.
static_assert(sizeof(CycleRekeyVerifyArgs) <= 4096, "the table of entries travels in the kernel arguments");
int launch_rekey_verify(const EntryRun &r, modgpu_verify_result_t *results, uint32_t key_from, uint32_t key_to, hipStream_t stream)
{
    CycleRekeyVerifyArgs a{};
    const uint64_t chunk = modgpu_rekey_verify_chunk_bytes();
    const EntryPlan p = plan_entries(a, r, chunk, [&](CycleRekeyVerifyPart &P, int k, const EntryGeom &g) {
        P.expect_body = r.role[k] + g.head;
        P.result = reinterpret_cast<CycleVerifyResult *>(results + r.idx[k]);
        P.n = r.size[k];
        entry_bases(g, key_from, r.off[0][k] % lcg::PERIOD, P.base_head[0], P.base_body[0], P.base_tail[0]);
        entry_bases(g, key_to, r.off[1][k] % lcg::PERIOD, P.base_head[1], P.base_body[1], P.base_tail[1]);
    });
    const uint32_t grid = entry_grid(p.total, verify_grid_forced() ? verify_grid_forced() : large_grid());
    const int form = p.misaligned ? CYCLE_REKEY_VERIFY_FUNNEL : CYCLE_REKEY_VERIFY_PLAIN;
    return entry_launched(modgpu_launch_cycle_rekey_verify(a, form, grid, stream), "rekey verify kernel launch", nullptr, modgpu_rekey_verify_kernel_name(form),
                          CYCLE_REKEY_VERIFY, grid, modgpu_rekey_verify_block(), chunk, p.bytes, MODGPU_REKEY_VERIFY_KERNEL_SOURCE_HASH);
}

// Entries already checked (check_verify_entries), on the current device, asynchronous on `stream`.  One launch initialises all n
// results.  Degenerate keystreams follow rekey_impl's rules and run on the verify kernels: a key == 0 mod m leaves only the other key
// (both zero: the identity forms); an entry with the same reduced key at the same stream position has ks ^ ks = 0 and is compared under
// the identity forms.  The entries whose two streams differ come first, in groups of up to kCycleBatchMax per two-keystream launch,
// then the coinciding ones in groups of their own.
int verify_rekey_impl(const void *const *expect, const void *const *src, const uint64_t *sizes, const uint64_t *offs_from, const uint64_t *offs_to,
                      int n, int32_t key_from, int32_t key_to, modgpu_verify_result_t *results, hipStream_t stream)
{
    const uint32_t kf = lcg::key_residue(key_from), kt = lcg::key_residue(key_to);
    if (!kf) return verify_impl(expect, src, sizes, offs_to, n, key_to, results, stream); // (key_to == 0 too: a plain compare)
    if (!kt) return verify_impl(expect, src, sizes, offs_from, n, key_from, results, stream);
    if (n == 0) return MODGPU_OK;
    if (int rc = prepare_results(results, n, stream)) return rc;
    const SameStream identity{kf == kt, offs_from, offs_to};
    if (int rc = for_each_run(expect, src, sizes, offs_from, offs_to, n, [&](int i) { return !identity(i); },
                              [&](const EntryRun &r) { return launch_rekey_verify(r, results, kf, kt, stream); }))
        return rc;
    return for_each_run(expect, src, sizes, nullptr, nullptr, n, identity, [&](const EntryRun &r) { return launch_verify(r, results, 0u, stream); });
}
} // namespace

int cycle_to_device_impl(void *dst, const void *src, uint64_t n, int32_t key, uint64_t stream_off, hipStream_t stream)
{
    return cycle_to_impl(&dst, &src, &n, &stream_off, 1, key, stream);
}

// One-time work a device's FIRST launch would otherwise pay inside the caller's timed region: loading the code object
// (~10 ms) and setting up the ticket ring (two allocations, a stream, a memset).  modgpu_alloc calls this for the device
// it allocates on -- a caller that keeps parts resident has paid it before its first pass (profiles/r03_first_pass.txt:
// 13 ms for launch 1 of a process without it, 1.2 ms with).  Best effort: whatever fails here is retried by the launch.
void prepare_device()
{
    static std::mutex mu;
    static bool done[kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        (void)hipGetLastError();
        return;
    }
    {
        std::lock_guard<std::mutex> lock(mu);
        if (done[dev]) return;
        done[dev] = true;
    }
    hipStream_t st = nullptr;
    uint8_t *scratch = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&scratch), 4096) == hipSuccess) {
        // the ticket ring, and one empty launch: the code object all three shapes live in is loaded by it
        (void)queue_ring_create(g_queue_ring[dev], st);
        CycleArgs a{};
        a.body = a.head_ptr = a.tail_ptr = scratch;
        a.base_head = a.base_body = a.base_tail = 1;
        a.stride_mul2 = 2;
        (void)modgpu_launch_cycle(a, CYCLE_SMALL, 1, st);
        // ... and two REAL launches of the work-queue kernel over a scratch buffer (two 64 KiB parts sharing a launch: ring line,
        // ticket traffic, sign-off word and all).  A process's first real work-queue launch costs 15-35 us more than its later
        // ones -- the runtime resolves the kernel function, the ring's host-visible sign-off words are touched for the first time --
        // and HIP events around a caller's first large launch count that: a fresh process's first 411 MB launch after an upload
        // took 0.143-0.148 ms without this against 0.128-0.133 with it, 0.126-0.128 being the size's steady rate
        // (profiles/r05_first_launch.txt; an EMPTY launch of the same kernel, even on the full grid, bought only 0.139).
        // Not counted in modgpu_path_stats / modgpu_queue_stats, not reported by modgpu_last_launch: it is nobody's launch.
        {
            const modgpu_launch_info_t keep = t_last_launch;
            uint8_t *big = nullptr;
            if (hipMalloc(reinterpret_cast<void **>(&big), 3u << 16) == hipSuccess) {
                void *parts[2] = {big, big + (1u << 16)};
                const uint64_t sizes[2] = {1u << 16, 1u << 16};
                for (int k = 0; k < 2; ++k)
                    if (launch_queue(parts, sizes, nullptr, 2, /*key_res=*/1, st) == MODGPU_OK) {
                        g_stats.gpu_launches.fetch_sub(1, std::memory_order_relaxed);
                        g_queue_eager.fetch_sub(1, std::memory_order_relaxed);
                        g_batch_launches.fetch_sub(1, std::memory_order_relaxed);
                        g_batch_parts.fetch_sub(2, std::memory_order_relaxed);
                    }
                // ... and of its copy with a resident slice, which a single buffer of kKeepMin bytes or more takes: the same first-launch
                // cost (measured 0.6 ms on a fresh process's first 4 GiB pass without this), paid here instead
                for (int k = 0; k < 2; ++k)
                    if (launch_queue(parts, sizes, nullptr, 1, /*key_res=*/1, st, /*warm_keep=*/true) == MODGPU_OK) {
                        g_stats.gpu_launches.fetch_sub(1, std::memory_order_relaxed);
                        g_queue_eager.fetch_sub(1, std::memory_order_relaxed);
                    }
                (void)hipStreamSynchronize(st);
                (void)hipFree(big);
            }
            t_last_launch = keep;
        }
        (void)hipStreamSynchronize(st);
    }
    (void)hipGetLastError();
    if (scratch) (void)hipFree(scratch);
    if (st) (void)hipStreamDestroy(st);
}

// ---- page-locked host memory ----------------------------------------------------------------
namespace {
enum class HostKind {
    HipHost,    // hipHostMalloc
    Plain,      // posix_memalign: no GPU, or the pages could not be locked
    Registered, // the caller's own memory, pinned in place by modgpu_host_register (never freed here)
    Placed,     // our own mmap with a NUMA policy per part, pinned in place by hipHostRegister (or not pinned: see `pinned`)
};
struct HostRange {
    uintptr_t base;
    uint64_t size;
    bool pinned; // page-locked and device-visible
    HostKind kind;
};
std::mutex g_host_mu;
std::vector<HostRange> g_host_ranges; // few, long-lived allocations: linear scan
} // namespace

bool host_range_pinned(const void *p, uint64_t n)
{
    if (!p) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lock(g_host_mu);
    for (const HostRange &r : g_host_ranges)
        if (r.pinned && a >= r.base && n <= r.size && a - r.base <= r.size - n) return true;
    return false;
}

namespace {

int cycle_host_impl(uint8_t *host, uint64_t n, int32_t key, uint64_t stream_off, int device, bool host_may_finish = false,
                    StreamOutcome *out = nullptr)
{
    if (out) *out = StreamOutcome{};
    if (n == 0) return MODGPU_OK;
    if (!host) return fail(MODGPU_ERR_INVALID, "null host buffer");
    Endpoint e;
    e.mem = host;
    e.pinned = host_range_pinned(host, n);
    return stream_impl(e, e, n, key, stream_off, device, host_may_finish, out);
}

int scalar_impl(uint8_t *host, uint64_t n, int32_t key, uint64_t stream_off, int isa = MODGPU_ISA_AUTO)
{
    if (n && !host) return fail(MODGPU_ERR_INVALID, "null host buffer");
    if (gpu_required()) return fail(MODGPU_ERR_FORBIDDEN, "host loop forbidden by MODGPU_REQUIRE_GPU");
    if (isa != MODGPU_ISA_AUTO && !modgpu_scalar_isa_usable(isa)) return fail(MODGPU_ERR_INVALID, "this CPU does not run that host-loop body");
    modgpu_scalar_cycle(host, n, key, stream_off, isa);
    g_stats.scalar_calls.fetch_add(1, std::memory_order_relaxed);
    g_stats.scalar_bytes.fetch_add(n, std::memory_order_relaxed);
    return MODGPU_OK;
}

uint32_t load_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

void store_le32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

} // namespace
// ---- the eight calls over a table in device memory: modgpu_cycle_table_device, modgpu_rekey_table_device, modgpu_verify_table_device,
// modgpu_verify_rekey_table_device, modgpu_digest_table_device, modgpu_cycle_digest_table_device, modgpu_rekey_digest_table_device (three launches: plan, finish, stream) and modgpu_rekey_move_table_device
// (five) -- and modgpu_rekey_relayout_table_device, the move call's launches twice (ten).
// One workspace walk, one set of grid hooks and one call body (table_call); a call is its layout, its launches and its names. --------
namespace {
static_assert(sizeof(modgpu_table_entry_t) == sizeof(CycleTableEntry) && offsetof(modgpu_table_entry_t, key) == offsetof(CycleTableEntry, key) &&
                  offsetof(modgpu_table_entry_t, flags) == offsetof(CycleTableEntry, flags),
              "the kernels read the public entry layout");
static_assert(MODGPU_TABLE_MAX_ENTRIES == kTableMaxEntries, "one limit");
static_assert(sizeof(modgpu_rekey_table_entry_t) == sizeof(RekeyTableEntry) && offsetof(modgpu_rekey_table_entry_t, off_to) == offsetof(RekeyTableEntry, off_to) &&
                  offsetof(modgpu_rekey_table_entry_t, key_from) == offsetof(RekeyTableEntry, key_from) &&
                  offsetof(modgpu_rekey_table_entry_t, key_to) == offsetof(RekeyTableEntry, key_to) &&
                  offsetof(modgpu_rekey_table_entry_t, flags) == offsetof(RekeyTableEntry, flags) &&
                  offsetof(modgpu_rekey_table_entry_t, reserved) == offsetof(RekeyTableEntry, reserved) && sizeof(modgpu_rekey_table_entry_t) == 56,
              "the kernels read the public entry layout");
static_assert(sizeof(RekeyTablePlan) == sizeof(CycleTablePlan), "the table call's layout holds the rekey plan records");
static_assert(sizeof(modgpu_verify_table_summary_t) == 32 && offsetof(modgpu_verify_table_summary_t, first_bad_entry) == offsetof(VerifyTableSummary, first_bad_entry) &&
                  offsetof(modgpu_verify_table_summary_t, entries) == offsetof(VerifyTableSummary, entries) &&
                  offsetof(modgpu_verify_table_summary_t, reserved) == offsetof(VerifyTableSummary, reserved),
              "the summary line starts with the public record");
static_assert(sizeof(CycleTableHdr) == 64 && sizeof(MoveTableHdr) == 64 && sizeof(VerifyTableSummary) == 64, "the header and the summary are one line each");

// Where everything of a call over n entries lies in its workspace: offsets from its start, each section on a 64-byte line.  The header
// comes first in every kind (modgpu_table_status reads them all), a verifying call's summary line right behind it
// (modgpu_verify_table_summary).  A section the call does not have is 0.
struct TableLayout {
    uint64_t sum, blk, plan, edge, scratch, flags, win, level[kTableLevels], level_n[kTableLevels], cap, bytes;
    uint32_t top, n_blk;
};
// The next section of a workspace: its offset; the cursor `at` moves past it to the next line
uint64_t take(uint64_t &at, uint64_t bytes)
{
    const uint64_t section = at;
    at = (at + bytes + 63) & ~63ull;
    return section;
}
// The search levels: level k holds ceil(n / 16^k) keys padded to a multiple of 16, up to the first level of at most 16 keys (the top)
void take_levels(TableLayout &L, uint64_t &at, uint64_t n)
{
    uint64_t cnt = n;
    for (uint32_t k = 0; k < (uint32_t)kTableLevels; ++k) {
        L.level[k] = take(at, ((cnt + 15) & ~15ull) * sizeof(uint32_t));
        L.level_n[k] = cnt;
        L.top = k;
        if (cnt <= 16) break;
        cnt = (cnt + 15) / 16;
    }
}
// The three-launch calls: header, [summary,] the 1024-entry records, the plan records, the search levels[, the edge states]
TableLayout three_launch_layout(uint64_t n, bool summary, bool edges)
{
    TableLayout L{};
    L.n_blk = (uint32_t)((n + kTableBlock - 1) / kTableBlock);
    uint64_t at = sizeof(CycleTableHdr);
    if (summary) L.sum = take(at, sizeof(VerifyTableSummary));
    L.blk = take(at, (uint64_t)L.n_blk * sizeof(CycleTableBlk));
    L.plan = take(at, n * sizeof(CycleTablePlan));
    take_levels(L, at, n);
    if (edges) L.edge = take(at, n * sizeof(RekeyTableEdge));
    L.bytes = at;
    return L;
}
TableLayout table_layout(uint64_t n) { return three_launch_layout(n, false, false); }
TableLayout rekey_table_layout(uint64_t n) { return three_launch_layout(n, false, true); }
TableLayout verify_table_layout(uint64_t n) { return three_launch_layout(n, true, false); }
TableLayout rekey_verify_table_layout(uint64_t n) { return three_launch_layout(n, true, true); }

// The move call: header, the 1024-entry records, the plan records, the edge states, 32 bytes of scratch per entry for the ragged ends,
// one "loaded" flag and one window per chunk the call may have (total_bytes / 64 KiB + 2 per entry: a body of n bytes lies on at most
// n / 64 KiB + 2 chunks of its destination), the search levels.
uint64_t move_table_chunks(uint64_t n, uint64_t total_bytes) { return total_bytes / modgpu_rekey_move_table_chunk_bytes() + 2 * n; }
TableLayout move_table_layout(uint64_t n, uint64_t total_bytes)
{
    uint64_t at = sizeof(MoveTableHdr);
    TableLayout L{};
    L.n_blk = (uint32_t)((n + kTableBlock - 1) / kTableBlock);
    L.cap = move_table_chunks(n, total_bytes);
    L.blk = take(at, (uint64_t)L.n_blk * sizeof(MoveTableBlk));
    L.plan = take(at, n * sizeof(MoveTablePlan));
    L.edge = take(at, n * sizeof(RekeyTableEdge));
    L.scratch = take(at, n * kMoveTableScratch);
    L.flags = take(at, L.cap * sizeof(uint32_t));
    L.win = take(at, L.cap * sizeof(MoveTableWin));
    take_levels(L, at, n);
    L.bytes = at;
    return L;
}
bool move_table_sizes_ok(uint64_t n, uint64_t total_bytes)
{
    return n != 0 && n <= kTableMaxEntries && total_bytes / modgpu_rekey_move_table_chunk_bytes() <= kTableMaxChunks - 2 * kTableMaxEntries;
}

// The grid of a call's stream (move) launch.  The out-of-place table takes the out-of-place kernel's (25 workgroups per 32 CUs;
// DESIGN.md 4.8 has the A/B against one per CU); its digesting mode measured the other way round and, like the
// others, takes one workgroup per CU on every CU, as the rekey and verify kernels (the move launch never gets more than the device holds at once).  modgpu_debug_set_*_table_grid forces one.
enum TableCall { kCycleTable, kRekeyTable, kVerifyTable, kRekeyVerifyTable, kMoveTable, kDigestTable, kCycleDigestTable, kRekeyDigestTable, kTableCalls };
#ifdef MODGPU_TESTING_HOOKS
std::atomic<uint32_t> g_table_grid[kTableCalls] = {};
uint32_t table_grid_forced(TableCall c) { return g_table_grid[c].load(std::memory_order_relaxed); }
void force_table_grid(TableCall c, uint32_t grid) { g_table_grid[c].store(std::min<uint32_t>(grid, 4096u), std::memory_order_relaxed); }
#else
constexpr uint32_t table_grid_forced(TableCall) { return 0; }
#endif
uint32_t table_grid(TableCall c)
{
    if (const uint32_t forced = table_grid_forced(c)) return forced;
    if (c != kCycleTable) return std::max<uint32_t>(1, large_grid());
    uint64_t cap = 0, helpers = 0;
    queue_grid(0, large_grid(), &cap, &helpers);
    return (uint32_t)std::max<uint64_t>(1, cap);
}

// What a call is: which of the eight (its grid), the size of the record it writes per entry into `results` (the verifying calls' result,
// the digest call's record; 0: the call has no `results`, and nothing looks at that argument), and what it is called -- in tier 1's
// words for a short workspace, and in modgpu_last_launch's report of its stream (move) launch
struct TableKind {
    TableCall call;
    uint32_t result_bytes;
    const char *short_workspace;
    const char *(*kernel)();
    int variant;
    uint32_t (*block)(), (*chunk_bytes)();
    const char *source_hash;
};
// One launch of a call and what fail_hip calls it.  The launches take the grid by reference: the move launch lowers it to what the device
// holds at once (the one in-out argument among them, so all of them get it rather than that launch a path of its own).
template <class Args> struct TableLaunch {
    const char *what;
    hipError_t (*launch)(const Args &a, uint32_t &grid, hipStream_t stream);
};
template <class Args, hipError_t (*F)(const Args &, hipStream_t)> hipError_t no_grid(const Args &a, uint32_t &, hipStream_t s) { return F(a, s); }
template <class Args, hipError_t (*F)(const Args &, uint32_t, hipStream_t)> hipError_t on_grid(const Args &a, uint32_t &grid, hipStream_t s) { return F(a, grid, s); }

// A table call.  Tier 1 (include/modgpu.h): everything checked before anything is queued; then the launches on `stream`, in order.
// `refused`: a refusal of the call's own, made right behind the limit (the move call's total_bytes), or nullptr;
// `layout()` plans the workspace once the pointers are known to be sound; `bind(a, w, L)` puts the call's own sections into a.
template <class Args, class Entry, size_t N, class Layout, class Bind>
int table_call(const TableKind &kind, const TableLaunch<Args> (&launches)[N], const Entry *entries, uint64_t n, const void *results,
               const char *refused, void *ws, uint64_t ws_bytes, int device, hipStream_t stream, Layout layout, Bind bind)
{
    if (n == 0) return MODGPU_OK;
    if (n > kTableMaxEntries) return fail(MODGPU_ERR_INVALID, "more than 4194304 entries (the table call's limit)");
    if (refused) return fail(MODGPU_ERR_INVALID, refused);
    if (!entries || !ws) return fail(MODGPU_ERR_INVALID, "null table or workspace");
    if (kind.result_bytes && !results) return fail(MODGPU_ERR_INVALID, "null results");
    if ((reinterpret_cast<uintptr_t>(entries) | reinterpret_cast<uintptr_t>(ws)) & 7) return fail(MODGPU_ERR_INVALID, "table or workspace not 8-byte aligned");
    if (kind.result_bytes && (reinterpret_cast<uintptr_t>(results) & 7)) return fail(MODGPU_ERR_INVALID, "results not 8-byte aligned");
    const TableLayout L = layout();
    if (ws_bytes < L.bytes) return fail(MODGPU_ERR_INVALID, kind.short_workspace);
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    int phys = -1;
    HIP_TRY(hipGetDevice(&phys));
    if (modgpu_xfer_device_of(entries, n * sizeof(Entry)) != phys || modgpu_xfer_device_of(ws, L.bytes) != phys)
        return fail(MODGPU_ERR_INVALID, "the table or the workspace is not device memory of the call's device");
    if (kind.result_bytes && modgpu_xfer_device_of(results, n * kind.result_bytes) != phys)
        return fail(MODGPU_ERR_INVALID, "the results are not device memory of the call's device");
    uint8_t *const w = static_cast<uint8_t *>(ws);
    Args a{};
    a.entries = reinterpret_cast<decltype(a.entries)>(entries);
    a.n = n;
    a.hdr = reinterpret_cast<decltype(a.hdr)>(w);
    a.blk = reinterpret_cast<decltype(a.blk)>(w + L.blk);
    a.plan = reinterpret_cast<decltype(a.plan)>(w + L.plan);
    for (uint32_t k = 0; k <= L.top; ++k) {
        a.level[k] = reinterpret_cast<uint32_t *>(w + L.level[k]);
        a.level_n[k] = L.level_n[k];
    }
    a.top = L.top;
    a.n_blk = L.n_blk;
    bind(a, w, L);
    uint32_t grid = table_grid(kind.call);
    (void)hipGetLastError(); // (the launches report hipGetLastError: an earlier call's error must not be taken for theirs)
    for (const TableLaunch<Args> &l : launches) {
        const hipError_t e = l.launch(a, grid, stream);
        if (e != hipSuccess) return fail_hip(e, l.what);
        g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    }
    t_last_launch = {kind.kernel(), kind.variant, grid, kind.block(), kind.chunk_bytes(), 0, grid, kind.source_hash};
    return MODGPU_OK;
}

// The out-of-place table call (records == nullptr: nothing looks at `side`), and the cycle digest table call: the same TU's three
// kernels in their digest mode, on the same workspace, writing one digest record per entry -- of the stored bytes or of the source
// bytes, by `side`.
int table_impl(const modgpu_table_entry_t *entries, uint64_t n, modgpu_digest_result_t *records, uint32_t side, void *ws, uint64_t ws_bytes, int device,
               hipStream_t stream)
{
    using A = CycleTableArgs;
    static constexpr TableKind kind = {kCycleTable, 0, "workspace smaller than modgpu_table_workspace_bytes(n_entries)", modgpu_table_kernel_name, CYCLE_TABLE,
                                         modgpu_table_block, modgpu_table_chunk_bytes, MODGPU_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> launches[] = {{"table plan launch", no_grid<A, modgpu_launch_table_plan>},
                                                  {"table finish launch", no_grid<A, modgpu_launch_table_finish>},
                                                  {"table stream launch", on_grid<A, modgpu_launch_table_stream>}};
    static constexpr TableKind digest_kind = {kCycleDigestTable, sizeof(modgpu_digest_result_t), "workspace smaller than modgpu_cycle_digest_table_workspace_bytes(n_entries)",
                                                modgpu_table_kernel_name, CYCLE_DIGEST_CYCLE_TABLE, modgpu_table_block, modgpu_table_chunk_bytes,
                                                MODGPU_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> digest_launches[] = {{"cycle digest table plan launch", no_grid<A, modgpu_launch_cycle_digest_table_plan>},
                                                         {"cycle digest table finish launch", no_grid<A, modgpu_launch_cycle_digest_table_finish>},
                                                         {"cycle digest table stream launch", on_grid<A, modgpu_launch_cycle_digest_table_stream>}};
    return table_call(records ? digest_kind : kind, records ? digest_launches : launches, entries, n, records, nullptr, ws, ws_bytes, device, stream,
                      [&] { return table_layout(n); },
                      [&](A &a, uint8_t *, const TableLayout &) {
                          a.side = records ? side : 0u;
                          a.records = reinterpret_cast<DigestTableRecord *>(records);
                      });
}

// modgpu_cycle_digest_table_device's own part of tier 1, in front of table_impl (where a null `records` means the plain call): the side,
// and a null `records` refused where the digest table call refuses it -- behind the count, the table and the workspace
int cycle_digest_table_impl(const modgpu_table_entry_t *entries, uint64_t n, modgpu_digest_result_t *records, uint32_t side, void *ws, uint64_t ws_bytes,
                            int device, hipStream_t stream)
{
    if (side != MODGPU_DIGEST_OUTPUT && side != MODGPU_DIGEST_INPUT)
        return fail(MODGPU_ERR_INVALID, "side is neither the output side (0) nor the input side (1)");
    if (n != 0 && n <= kTableMaxEntries && entries && ws && !records) return fail(MODGPU_ERR_INVALID, "null results");
    return table_impl(entries, n, records, side, ws, ws_bytes, device, stream);
}

// The rekey table call (records == nullptr: nothing looks at `side`), and the rekey digest table call: the same TU's three kernels in
// their digest mode, on the same workspace, writing one digest record per entry -- of the stored bytes, of the source bytes or of the
// plaintext between the two keystreams, by `side`.
int rekey_table_impl(const modgpu_rekey_table_entry_t *entries, uint64_t n, modgpu_digest_result_t *records, uint32_t side, void *ws, uint64_t ws_bytes,
                     int device, hipStream_t stream)
{
    using A = RekeyTableArgs;
    static constexpr TableKind kind = {kRekeyTable, 0, "workspace smaller than modgpu_rekey_table_workspace_bytes(n_entries)", modgpu_rekey_table_kernel_name,
                                         CYCLE_REKEY_TABLE, modgpu_rekey_table_block, modgpu_rekey_table_chunk_bytes, MODGPU_REKEY_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> launches[] = {{"rekey table plan launch", no_grid<A, modgpu_launch_rekey_table_plan>},
                                                  {"rekey table finish launch", no_grid<A, modgpu_launch_rekey_table_finish>},
                                                  {"rekey table stream launch", on_grid<A, modgpu_launch_rekey_table_stream>}};
    static constexpr TableKind digest_kind = {kRekeyDigestTable, sizeof(modgpu_digest_result_t), "workspace smaller than modgpu_rekey_digest_table_workspace_bytes(n_entries)",
                                                modgpu_rekey_table_kernel_name, CYCLE_REKEY_DIGEST_TABLE, modgpu_rekey_table_block, modgpu_rekey_table_chunk_bytes,
                                                MODGPU_REKEY_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> digest_launches[] = {{"rekey digest table plan launch", no_grid<A, modgpu_launch_rekey_digest_table_plan>},
                                                         {"rekey digest table finish launch", no_grid<A, modgpu_launch_rekey_digest_table_finish>},
                                                         {"rekey digest table stream launch", on_grid<A, modgpu_launch_rekey_digest_table_stream>}};
    return table_call(records ? digest_kind : kind, records ? digest_launches : launches, entries, n, records, nullptr, ws, ws_bytes, device, stream,
                      [&] { return rekey_table_layout(n); },
                      [&](A &a, uint8_t *w, const TableLayout &L) {
                          a.edge = reinterpret_cast<RekeyTableEdge *>(w + L.edge);
                          a.side = records ? side : 0u;
                          a.records = reinterpret_cast<DigestTableRecord *>(records);
                      });
}

// modgpu_rekey_digest_table_device's own part of tier 1, in front of rekey_table_impl (where a null `records` means the plain call): the
// side, and a null `records` refused where the digest table call refuses it -- behind the count, the table and the workspace
static_assert(MODGPU_DIGEST_OUTPUT == REKEY_TABLE_SIDE_OUTPUT && MODGPU_DIGEST_INPUT == REKEY_TABLE_SIDE_INPUT && MODGPU_DIGEST_PLAIN == REKEY_TABLE_SIDE_PLAIN,
              "the kernels read the public side");
int rekey_digest_table_impl(const modgpu_rekey_table_entry_t *entries, uint64_t n, modgpu_digest_result_t *records, uint32_t side, void *ws,
                            uint64_t ws_bytes, int device, hipStream_t stream)
{
    if (side != MODGPU_DIGEST_OUTPUT && side != MODGPU_DIGEST_INPUT && side != MODGPU_DIGEST_PLAIN)
        return fail(MODGPU_ERR_INVALID, "side is neither the output side (0), the input side (1) nor the plaintext between the keystreams (2)");
    if (n != 0 && n <= kTableMaxEntries && entries && ws && !records) return fail(MODGPU_ERR_INVALID, "null results");
    return rekey_table_impl(entries, n, records, side, ws, ws_bytes, device, stream);
}

int verify_table_impl(const modgpu_table_entry_t *entries, uint64_t n, modgpu_verify_result_t *results, void *ws, uint64_t ws_bytes, int device,
                      hipStream_t stream)
{
    using A = VerifyTableArgs;
    static constexpr TableKind kind = {kVerifyTable, sizeof(modgpu_verify_result_t), "workspace smaller than modgpu_verify_table_workspace_bytes(n_entries)", modgpu_verify_table_kernel_name,
                                         CYCLE_VERIFY_TABLE, modgpu_verify_table_block, modgpu_verify_table_chunk_bytes, MODGPU_VERIFY_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> launches[] = {{"verify table plan launch", no_grid<A, modgpu_launch_verify_table_plan>},
                                                  {"verify table finish launch", no_grid<A, modgpu_launch_verify_table_finish>},
                                                  {"verify table stream launch", on_grid<A, modgpu_launch_verify_table_stream>}};
    return table_call(kind, launches, entries, n, results, nullptr, ws, ws_bytes, device, stream, [&] { return verify_table_layout(n); },
                      [&](A &a, uint8_t *w, const TableLayout &L) {
                          a.sum = reinterpret_cast<VerifyTableSummary *>(w + L.sum);
                          a.results = reinterpret_cast<CycleVerifyResult *>(results);
                      });
}

// The digest table call: the verify table TU's three kernels in their digest mode, on the out-of-place table call's workspace (no
// summary line).  `dst` of an entry is never looked at.
static_assert(sizeof(modgpu_digest_result_t) == sizeof(DigestTableRecord) && offsetof(modgpu_digest_result_t, s2) == offsetof(DigestTableRecord, s2) &&
                  offsetof(modgpu_digest_result_t, n) == offsetof(DigestTableRecord, n) && offsetof(modgpu_digest_result_t, reserved) == offsetof(DigestTableRecord, reserved) &&
                  kDigestTableMod == kDigestMod,
              "the digest table kernels write the public record");
int digest_table_impl(const modgpu_table_entry_t *entries, uint64_t n, modgpu_digest_result_t *records, void *ws, uint64_t ws_bytes, int device,
                      hipStream_t stream)
{
    using A = VerifyTableArgs;
    static constexpr TableKind kind = {kDigestTable, sizeof(modgpu_digest_result_t), "workspace smaller than modgpu_digest_table_workspace_bytes(n_entries)",
                                         modgpu_verify_table_kernel_name, CYCLE_DIGEST_TABLE, modgpu_verify_table_block, modgpu_verify_table_chunk_bytes,
                                         MODGPU_VERIFY_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> launches[] = {{"digest table plan launch", no_grid<A, modgpu_launch_digest_table_plan>},
                                                  {"digest table finish launch", no_grid<A, modgpu_launch_digest_table_finish>},
                                                  {"digest table stream launch", on_grid<A, modgpu_launch_digest_table_stream>}};
    return table_call(kind, launches, entries, n, records, nullptr, ws, ws_bytes, device, stream, [&] { return table_layout(n); },
                      [&](A &a, uint8_t *, const TableLayout &) { a.records = reinterpret_cast<DigestTableRecord *>(records); });
}

int verify_rekey_table_impl(const modgpu_rekey_table_entry_t *entries, uint64_t n, modgpu_verify_result_t *results, void *ws, uint64_t ws_bytes,
                            int device, hipStream_t stream)
{
    using A = RekeyVerifyTableArgs;
    static constexpr TableKind kind = {kRekeyVerifyTable, sizeof(modgpu_verify_result_t), "workspace smaller than modgpu_verify_rekey_table_workspace_bytes(n_entries)",
                                         modgpu_rekey_verify_table_kernel_name, CYCLE_REKEY_VERIFY_TABLE, modgpu_rekey_verify_table_block,
                                         modgpu_rekey_verify_table_chunk_bytes, MODGPU_REKEY_VERIFY_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> launches[] = {{"verify rekey table plan launch", no_grid<A, modgpu_launch_rekey_verify_table_plan>},
                                                  {"verify rekey table finish launch", no_grid<A, modgpu_launch_rekey_verify_table_finish>},
                                                  {"verify rekey table stream launch", on_grid<A, modgpu_launch_rekey_verify_table_stream>}};
    return table_call(kind, launches, entries, n, results, nullptr, ws, ws_bytes, device, stream, [&] { return rekey_verify_table_layout(n); },
                      [&](A &a, uint8_t *w, const TableLayout &L) {
                          a.sum = reinterpret_cast<VerifyTableSummary *>(w + L.sum);
                          a.edge = reinterpret_cast<RekeyTableEdge *>(w + L.edge);
                          a.results = reinterpret_cast<CycleVerifyResult *>(results);
                      });
}

hipError_t move_table_move(const MoveTableArgs &a, uint32_t &grid, hipStream_t s) { return modgpu_launch_rekey_move_table_move(a, &grid, s); }
template <uint32_t Sweep> hipError_t relayout_plan(const MoveTableArgs &a, uint32_t &, hipStream_t s) { return modgpu_launch_rekey_relayout_plan(a, Sweep, s); }
template <uint32_t Sweep> hipError_t relayout_finish(const MoveTableArgs &a, uint32_t &, hipStream_t s) { return modgpu_launch_rekey_relayout_finish(a, Sweep, s); }
// The move table call, and (relayout) the relayout call: the same layout, workspace and tier 1, and the five launches
// twice on the one stream -- sweep 0 over the entries with dst <= src, sweep 1 over those with dst > src, the sweep a mode of the plan
// and finish kernels.
int rekey_move_table_impl(const modgpu_rekey_table_entry_t *entries, uint64_t n, uint64_t total_bytes, void *ws, uint64_t ws_bytes, int device,
                          hipStream_t stream, bool relayout = false)
{
    using A = MoveTableArgs;
    static constexpr TableKind kind = {kMoveTable, 0, "workspace smaller than modgpu_rekey_move_table_workspace_bytes(n_entries, total_bytes)",
                                         modgpu_rekey_move_table_kernel_name, CYCLE_REKEY_MOVE_TABLE, modgpu_rekey_move_table_block,
                                         modgpu_rekey_move_table_chunk_bytes, MODGPU_REKEY_MOVE_TABLE_KERNEL_SOURCE_HASH};
    static constexpr TableLaunch<A> launches[] = {{"rekey move table plan launch", no_grid<A, modgpu_launch_rekey_move_table_plan>},
                                                  {"rekey move table finish launch", no_grid<A, modgpu_launch_rekey_move_table_finish>},
                                                  {"rekey move table window launch", no_grid<A, modgpu_launch_rekey_move_table_window>},
                                                  {"rekey move table move launch", move_table_move},
                                                  {"rekey move table place launch", no_grid<A, modgpu_launch_rekey_move_table_place>}};
    static constexpr TableLaunch<A> sweeps[] = {{"rekey relayout plan launch of sweep 0", relayout_plan<kRelayoutSweepDown>},
                                                {"rekey relayout finish launch of sweep 0", relayout_finish<kRelayoutSweepDown>},
                                                {"rekey relayout window launch of sweep 0", no_grid<A, modgpu_launch_rekey_move_table_window>},
                                                {"rekey relayout move launch of sweep 0", move_table_move},
                                                {"rekey relayout place launch of sweep 0", no_grid<A, modgpu_launch_rekey_move_table_place>},
                                                {"rekey relayout plan launch of sweep 1", relayout_plan<kRelayoutSweepUp>},
                                                {"rekey relayout finish launch of sweep 1", relayout_finish<kRelayoutSweepUp>},
                                                {"rekey relayout window launch of sweep 1", no_grid<A, modgpu_launch_rekey_move_table_window>},
                                                {"rekey relayout move launch of sweep 1", move_table_move},
                                                {"rekey relayout place launch of sweep 1", no_grid<A, modgpu_launch_rekey_move_table_place>}};
    const char *refused = move_table_sizes_ok(n, total_bytes) ? nullptr : "total_bytes beyond 2^31 chunks of 64 KiB";
    auto call = [&](const auto &list) {
        return table_call(kind, list, entries, n, nullptr, refused, ws, ws_bytes, device, stream, [&] { return move_table_layout(n, total_bytes); },
                          [](A &a, uint8_t *w, const TableLayout &L) {
                              a.cap = L.cap;
                              a.edge = reinterpret_cast<RekeyTableEdge *>(w + L.edge);
                              a.scratch = w + L.scratch;
                              a.flags = reinterpret_cast<uint32_t *>(w + L.flags);
                              a.win = reinterpret_cast<MoveTableWin *>(w + L.win);
                          });
    };
    return relayout ? call(sweeps) : call(launches);
}

// The first `bytes` of a table call's workspace (its header[, its summary line]) read back for modgpu_table_status and
// modgpu_verify_table_summary: synchronous.  (modgpu_rekey_move_table_status keeps these steps written out: folded in as well, the
// libraries' lists of exported symbols are no longer the ones they had -- a weak std::to_string instance drops out.)
// modgpu_digest_check_summary reads its 32 bytes the same way, with words of its own for the two refusals.
int read_workspace_top(const void *dev_workspace, bool out_pointers, int device, void *top, size_t bytes,
                       const char *null_text = "null workspace or out pointer",
                       const char *foreign_text = "the workspace is not device memory of the call's device")
{
    if (!dev_workspace || !out_pointers) return fail(MODGPU_ERR_INVALID, null_text);
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    int phys = -1;
    HIP_TRY(hipGetDevice(&phys));
    if (modgpu_xfer_device_of(dev_workspace, bytes) != phys) return fail(MODGPU_ERR_INVALID, foreign_text);
    HIP_TRY(hipMemcpy(top, dev_workspace, bytes, hipMemcpyDeviceToHost));
    return MODGPU_OK;
}

// The digest check: records of any digest producer against a manifest of Adler-32 values, on the device.  Tier 1 (include/modgpu.h), then
// two launches on `stream`: the verify call's init launch on the one summary ({0, none, 0, 0} is its starting value too), then the verify
// table TU's finish kernel in its check mode.  No workspace of its own, no ticket, nothing that can run out.
static_assert(sizeof(modgpu_digest_check_summary_t) == 32 && sizeof(CycleVerifyResult) == 32 &&
                  offsetof(modgpu_digest_check_summary_t, bad_entries) == offsetof(CycleVerifyResult, mismatches) &&
                  offsetof(modgpu_digest_check_summary_t, first_bad_entry) == offsetof(CycleVerifyResult, first_mismatch) &&
                  offsetof(modgpu_digest_check_summary_t, entries) == offsetof(CycleVerifyResult, n) &&
                  offsetof(modgpu_digest_check_summary_t, refused) == offsetof(CycleVerifyResult, reserved),
              "the check kernel writes the public summary, and the verify call's init launch starts it");
uint64_t digest_check_bits_bytes(uint64_t n) { return n == 0 || n > kTableMaxEntries ? 0 : 8 * ((n + 63) / 64); }
int digest_check_impl(const modgpu_digest_result_t *records, const uint32_t *expect, uint64_t n, const void *table_ws,
                      modgpu_digest_check_summary_t *summary, uint64_t *bits, int device, hipStream_t stream)
{
    if (n == 0) return MODGPU_OK;
    if (n > kTableMaxEntries) return fail(MODGPU_ERR_INVALID, "more entries than a table call takes (4194304)");
    if (!records || !expect || !summary) return fail(MODGPU_ERR_INVALID, "null records, manifest or summary");
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(summary) | reinterpret_cast<uintptr_t>(bits)) & 7)
        return fail(MODGPU_ERR_INVALID, "records, summary or bits not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(expect) & 3) return fail(MODGPU_ERR_INVALID, "manifest not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(table_ws) & 7) return fail(MODGPU_ERR_INVALID, "table workspace not 8-byte aligned");
    const uint64_t records_bytes = n * sizeof *records, expect_bytes = n * sizeof *expect, bits_bytes = bits ? digest_check_bits_bytes(n) : 0;
    auto meet = [](const void *p, uint64_t pn, const void *q, uint64_t qn) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
        return pn && qn && a < b + qn && b < a + pn;
    };
    if (meet(summary, sizeof *summary, records, records_bytes) || meet(summary, sizeof *summary, expect, expect_bytes) ||
        meet(bits, bits_bytes, records, records_bytes) || meet(bits, bits_bytes, expect, expect_bytes) || meet(bits, bits_bytes, summary, sizeof *summary))
        return fail(MODGPU_ERR_INVALID, "the summary or the bits overlap the records, the manifest or each other");
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    int phys = -1;
    HIP_TRY(hipGetDevice(&phys));
    if (modgpu_xfer_device_of(records, records_bytes) != phys || modgpu_xfer_device_of(expect, expect_bytes) != phys ||
        modgpu_xfer_device_of(summary, sizeof *summary) != phys || (bits && modgpu_xfer_device_of(bits, bits_bytes) != phys))
        return fail(MODGPU_ERR_INVALID, "the records, the manifest, the summary or the bits are not device memory of the call's device");
    if (table_ws && modgpu_xfer_device_of(table_ws, sizeof(CycleTableHdr)) != phys)
        return fail(MODGPU_ERR_INVALID, "the table workspace is not device memory of the call's device");
    CycleVerifyResult *const sum = reinterpret_cast<CycleVerifyResult *>(summary);
    (void)hipGetLastError(); // (the launches report hipGetLastError: an earlier call's error must not be taken for theirs)
    hipError_t e = modgpu_launch_verify_init(sum, 1, stream);
    if (e != hipSuccess) return fail_hip(e, "digest check init launch");
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    e = modgpu_launch_digest_check(reinterpret_cast<const DigestTableRecord *>(records), expect, n, static_cast<const CycleTableHdr *>(table_ws), sum,
                                   reinterpret_cast<unsigned long long *>(bits), stream);
    if (e != hipSuccess) return fail_hip(e, "digest check launch");
    g_stats.gpu_launches.fetch_add(1, std::memory_order_relaxed);
    const uint32_t grid = (uint32_t)((n + kTableBlock - 1) / kTableBlock);
    t_last_launch = {"modgpu_cycle_verify_table_finish", CYCLE_DIGEST_CHECK, grid, kTableBlock, 0u, 0, grid, MODGPU_VERIFY_TABLE_KERNEL_SOURCE_HASH};
    return MODGPU_OK;
}

// `iters` calls of call(stream) between two events on `stream`, stopped at the first that fails: *ms_per_call = their mean
// (include/modgpu_testing.h: the modgpu_time_*_device entry points)
template <class Call> int time_calls(int device, void *hip_stream, int iters, float *ms_per_call, Call call)
{
    if (iters <= 0 || !ms_per_call) return fail(MODGPU_ERR_INVALID, "bad timing arguments");
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    int rc = MODGPU_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, st));
    for (int i = 0; i < iters && rc == MODGPU_OK; ++i) rc = call(st);
    hipError_t e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return fail_hip(e, "event timing");
    *ms_per_call = ms / (float)iters;
    return MODGPU_OK;
}

// The overlap rule of modgpu_cycle_batch_device_to over a host copy, in O(n log n): destinations sorted by start must not meet each
// other (a running maximum of ends), and a destination must not meet the source of another entry -- among the sources that start
// before it ends, the one reaching furthest, or the furthest of another entry when that one is its own.
uint32_t entry_reserved(const modgpu_table_entry_t &e) { return e.flags; }
uint32_t entry_reserved(const modgpu_rekey_table_entry_t &e) { return e.flags | e.reserved; }
template <class Entry> int table_validate_impl(const Entry *t, uint64_t n)
{
    if (n > kTableMaxEntries) return fail(MODGPU_ERR_INVALID, "more than 4194304 entries (the table call's limit)");
    if (n && !t) return fail(MODGPU_ERR_INVALID, "null table");
    auto at = [](const void *p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); };
    auto entry = [](uint64_t i, const char *what) { return fail(MODGPU_ERR_INVALID, "entry " + std::to_string(i) + ": " + what); };
    struct Range {
        uint64_t lo, hi, i;
    };
    std::vector<Range> d, s;
    for (uint64_t i = 0; i < n; ++i) {
        if (entry_reserved(t[i])) return entry(i, sizeof(Entry) == sizeof(modgpu_table_entry_t) ? "nonzero flags" : "nonzero flags or reserved");
        if (!t[i].n) continue;
        if (!t[i].dst || !t[i].src) return entry(i, "null buffer");
        const uint64_t dl = at(t[i].dst), sl = at(t[i].src);
        if (dl + t[i].n < dl || sl + t[i].n < sl) return entry(i, "range wraps the address space");
        if (dl != sl && dl < sl + t[i].n && sl < dl + t[i].n) return entry(i, "destination partly overlaps its source (only dst == src may alias)");
        d.push_back({dl, dl + t[i].n, i});
        s.push_back({sl, sl + t[i].n, i});
    }
    auto by_lo = [](const Range &x, const Range &y) { return x.lo < y.lo || (x.lo == y.lo && x.i < y.i); };
    std::sort(d.begin(), d.end(), by_lo);
    std::sort(s.begin(), s.end(), by_lo);
    uint64_t bad = UINT64_MAX;
    for (size_t k = 1, far = 0; k < d.size(); ++k) {
        if (d[k].lo < d[far].hi) bad = std::min(bad, std::min(d[k].i, d[far].i));
        if (d[k].hi > d[far].hi) far = k;
    }
    // prefix over the sources by start: the furthest end (and its entry) and the furthest end of any OTHER entry
    std::vector<uint64_t> end1(s.size()), id1(s.size()), end2(s.size());
    for (size_t k = 0; k < s.size(); ++k) {
        uint64_t e1 = k ? end1[k - 1] : 0, i1 = k ? id1[k - 1] : UINT64_MAX, e2 = k ? end2[k - 1] : 0;
        if (s[k].hi > e1) {
            if (s[k].i != i1) e2 = e1;
            e1 = s[k].hi;
            i1 = s[k].i;
        } else if (s[k].i != i1 && s[k].hi > e2) {
            e2 = s[k].hi;
        }
        end1[k] = e1;
        id1[k] = i1;
        end2[k] = e2;
    }
    for (const Range &r : d) {
        const size_t c = std::lower_bound(s.begin(), s.end(), r.hi, [](const Range &x, uint64_t v) { return x.lo < v; }) - s.begin();
        if (!c) continue;
        if ((id1[c - 1] != r.i && end1[c - 1] > r.lo) || end2[c - 1] > r.lo) bad = std::min(bad, r.i);
    }
    if (bad != UINT64_MAX) return entry(bad, "destination meets another entry's source or destination");
    return MODGPU_OK;
}

// Tiers 1 and 2 over a host copy, in O(n), as the device decides them: the direction is that of the first entry with dst != src, and
// every non-empty entry is compared with the non-empty entry before it.  (The chunk count against the workspace is the one check that
// needs total_bytes: it is not made here.)  one_way = false: the relayout call's rule, the same without the direction clause.
int rekey_move_table_validate_impl(const modgpu_rekey_table_entry_t *t, uint64_t n, bool one_way = true)
{
    if (n > kTableMaxEntries) return fail(MODGPU_ERR_INVALID, "more than 4194304 entries (the table call's limit)");
    if (n && !t) return fail(MODGPU_ERR_INVALID, "null table");
    auto at = [](const void *p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); };
    auto entry = [](uint64_t i, const char *what) { return fail(MODGPU_ERR_INVALID, "entry " + std::to_string(i) + ": " + what); };
    const uint64_t chunk = modgpu_rekey_move_table_chunk_bytes();
    int way = 0; // -1 downward, +1 upward
    for (uint64_t i = 0; i < n && !way && one_way; ++i)
        if (t[i].n) way = at(t[i].dst) < at(t[i].src) ? -1 : at(t[i].dst) > at(t[i].src) ? 1 : 0;
    uint64_t prev = UINT64_MAX;
    for (uint64_t i = 0; i < n; ++i) {
        if (entry_reserved(t[i])) return entry(i, "nonzero flags or reserved");
        if (!t[i].n) continue;
        if (!t[i].dst || !t[i].src) return entry(i, "null buffer");
        const uint64_t d = at(t[i].dst), s = at(t[i].src);
        if (t[i].n >= kTableMaxEntryChunks * chunk) return entry(i, "1 TiB or more");
        if (one_way && (way > 0 ? d < s : d > s)) return entry(i, way > 0 ? "slides down in an upward table" : "slides up in a downward table");
        if (prev != UINT64_MAX) {
            const uint64_t ps = at(t[prev].src), pd = at(t[prev].dst), pn = t[prev].n;
            if (s < ps || s - ps < pn) return entry(i, "source below the end of the previous entry's source (entries are listed by rising address, sources disjoint)");
            if (d < pd || d - pd < pn) return entry(i, "destination below the end of the previous entry's destination (entries are listed by rising address, destinations disjoint)");
        }
        prev = i;
    }
    return MODGPU_OK;
}

// The body of the ten exported entry-list calls: the checks that need no device, the call's device, the call on the caller's stream.
template <class Check, class Impl> int entry_call(int device, void *hip_stream, Check check, Impl impl)
{
    return guarded([&]() -> int {
        if (int rc = check()) return rc;
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        return impl(static_cast<hipStream_t>(hip_stream));
    });
}
} // namespace

} // namespace modgpu

using namespace modgpu;

extern "C" {

int modgpu_abi_version(void) { return MODGPU_ABI_VERSION; }

int modgpu_device_count(void) { return logical_count(); }

const char *modgpu_last_error(void) { return t_err.c_str(); }

int modgpu_cycle_device(void *dev_buf, uint64_t n, int32_t key, uint64_t stream_off, int device,
                        void *hip_stream)
{
    return guarded([&]() -> int {
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        return cycle_device_impl(dev_buf, n, key, stream_off, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_cycle_batch_device(void *const *dev_parts, const uint64_t *sizes, const uint64_t *stream_offs, int n_parts, int32_t key,
                              int device, void *hip_stream)
{
    return guarded([&]() -> int {
        if (n_parts < 0 || (n_parts > 0 && (!dev_parts || !sizes))) return fail(MODGPU_ERR_INVALID, "bad part list");
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        return cycle_batch_impl(dev_parts, sizes, stream_offs, n_parts, key, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_cycle_device_to(void *dev_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_to_entries(&dev_dst, &dev_src, &n, 1); },
                      [&](hipStream_t st) { return cycle_to_impl(&dev_dst, &dev_src, &n, &stream_off, 1, key, st); });
}

int modgpu_cycle_batch_device_to(void *const *dst_parts, const void *const *src_parts, const uint64_t *sizes, const uint64_t *stream_offs,
                                 int n_parts, int32_t key, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_to_entries(dst_parts, src_parts, sizes, n_parts); },
                      [&](hipStream_t st) { return cycle_to_impl(dst_parts, src_parts, sizes, stream_offs, n_parts, key, st); });
}

int modgpu_rekey_device_to(void *dev_dst, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to, uint64_t off_to,
                           int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_to_entries(&dev_dst, &dev_src, &n, 1); },
                      [&](hipStream_t st) { return rekey_impl(&dev_dst, &dev_src, &n, &off_from, &off_to, 1, key_from, key_to, st); });
}

uint64_t modgpu_move_workspace_bytes(uint64_t n)
{
    return n == 0 || n >= kMoveMaxChunks * modgpu_rekey_chunk_bytes() ? 0 : move_layout(n).bytes;
}

int modgpu_rekey_move_device(void *dev_dst, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to, uint64_t off_to,
                             void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return rekey_move_impl(dev_dst, dev_src, n, key_from, off_from, key_to, off_to, dev_workspace, workspace_bytes, device,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_move_status(const void *dev_workspace, int device, uint64_t *stalled_chunk)
{
    return guarded([&]() -> int {
        if (!dev_workspace || !stalled_chunk) return fail(MODGPU_ERR_INVALID, "null workspace or out pointer");
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        int phys = -1;
        HIP_TRY(hipGetDevice(&phys));
        if (modgpu_xfer_device_of(dev_workspace, kMoveHdrBytes) != phys)
            return fail(MODGPU_ERR_INVALID, "the workspace is not device memory of the call's device");
        uint32_t h[kMoveHdrBytes / sizeof(uint32_t)];
        HIP_TRY(hipMemcpy(h, dev_workspace, sizeof h, hipMemcpyDeviceToHost));
        *stalled_chunk = h[kMoveStatusWord] ? (uint64_t)h[kMoveStatusWord] - 1 : ~0ull;
        if (h[kMoveStatusWord])
            return fail(MODGPU_ERR_HIP, "the move gave up waiting at chunk " + std::to_string(*stalled_chunk) + " (the destination's contents are unspecified)");
        return MODGPU_OK;
    });
}

int modgpu_rekey_batch_device_to(void *const *dst_parts, const void *const *src_parts, const uint64_t *sizes, const uint64_t *offs_from,
                                 const uint64_t *offs_to, int n_parts, int32_t key_from, int32_t key_to, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_to_entries(dst_parts, src_parts, sizes, n_parts); },
                      [&](hipStream_t st) { return rekey_impl(dst_parts, src_parts, sizes, offs_from, offs_to, n_parts, key_from, key_to, st); });
}

int modgpu_verify_device(const void *dev_expect, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off,
                         modgpu_verify_result_t *dev_result, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_verify_entries(&dev_expect, &dev_src, &n, 1, dev_result); },
                      [&](hipStream_t st) { return verify_impl(&dev_expect, &dev_src, &n, &stream_off, 1, key, dev_result, st); });
}

int modgpu_verify_batch_device(const void *const *expect_parts, const void *const *src_parts, const uint64_t *sizes, const uint64_t *stream_offs,
                               int n_parts, int32_t key, modgpu_verify_result_t *dev_results, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_verify_entries(expect_parts, src_parts, sizes, n_parts, dev_results); },
                      [&](hipStream_t st) { return verify_impl(expect_parts, src_parts, sizes, stream_offs, n_parts, key, dev_results, st); });
}

int modgpu_verify_rekey_device(const void *dev_expect, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to,
                               uint64_t off_to, modgpu_verify_result_t *dev_result, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_verify_entries(&dev_expect, &dev_src, &n, 1, dev_result); },
                      [&](hipStream_t st) { return verify_rekey_impl(&dev_expect, &dev_src, &n, &off_from, &off_to, 1, key_from, key_to, dev_result, st); });
}

int modgpu_verify_rekey_batch_device(const void *const *expect_parts, const void *const *src_parts, const uint64_t *sizes, const uint64_t *offs_from,
                                     const uint64_t *offs_to, int n_parts, int32_t key_from, int32_t key_to, modgpu_verify_result_t *dev_results,
                                     int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_verify_entries(expect_parts, src_parts, sizes, n_parts, dev_results); },
                      [&](hipStream_t st) { return verify_rekey_impl(expect_parts, src_parts, sizes, offs_from, offs_to, n_parts, key_from, key_to, dev_results, st); });
}

int modgpu_verify_results(const modgpu_verify_result_t *dev_results, uint64_t count, int device, modgpu_verify_result_t *host_out)
{
    return guarded([&]() -> int {
        if (count > 0 && (!dev_results || !host_out)) return fail(MODGPU_ERR_INVALID, "null results or out pointer");
        if (reinterpret_cast<uintptr_t>(dev_results) & 7) return fail(MODGPU_ERR_INVALID, "results not 8-byte aligned");
        if (count > (1ull << 40)) return fail(MODGPU_ERR_INVALID, "too many results");
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        if (count == 0) return MODGPU_OK;
        int phys = -1;
        HIP_TRY(hipGetDevice(&phys));
        if (modgpu_xfer_device_of(dev_results, count * sizeof(modgpu_verify_result_t)) != phys)
            return fail(MODGPU_ERR_INVALID, "the results are not device memory of the call's device");
        HIP_TRY(hipMemcpy(host_out, dev_results, count * sizeof(modgpu_verify_result_t), hipMemcpyDeviceToHost));
        return MODGPU_OK;
    });
}

int modgpu_digest_device(void *dev_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off, modgpu_digest_result_t *dev_result,
                         int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_digest_entries(dev_dst ? &dev_dst : nullptr, &dev_src, &n, 1, dev_result); },
                      [&](hipStream_t st) { return digest_impl(dev_dst ? &dev_dst : nullptr, &dev_src, &n, &stream_off, 1, key, dev_result, st); });
}

int modgpu_digest_batch_device(void *const *dst_parts, const void *const *src_parts, const uint64_t *sizes, const uint64_t *stream_offs,
                               int n_parts, int32_t key, modgpu_digest_result_t *dev_results, int device, void *hip_stream)
{
    return entry_call(device, hip_stream, [&] { return check_digest_entries(dst_parts, src_parts, sizes, n_parts, dev_results); },
                      [&](hipStream_t st) { return digest_impl(dst_parts, src_parts, sizes, stream_offs, n_parts, key, dev_results, st); });
}

uint32_t modgpu_digest_adler32(const modgpu_digest_result_t *host_result)
{
    if (!host_result) return 1u;
    const uint64_t m = kDigestMod, s1 = host_result->s1 % m, s2 = host_result->s2 % m, n = host_result->n % m;
    const uint64_t a = (1 + s1) % m, b = (n + n * s1 % m + m - s2) % m;
    return (uint32_t)(b << 16 | a);
}

int modgpu_digest_results(const modgpu_digest_result_t *dev_results, uint64_t count, int device, modgpu_digest_result_t *host_out,
                          uint32_t *adler32_out)
{
    return guarded([&]() -> int {
        if (count > 0 && (!dev_results || !host_out)) return fail(MODGPU_ERR_INVALID, "null results or out pointer");
        if (reinterpret_cast<uintptr_t>(dev_results) & 7) return fail(MODGPU_ERR_INVALID, "results not 8-byte aligned");
        if (count > (1ull << 40)) return fail(MODGPU_ERR_INVALID, "too many results");
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        if (count == 0) return MODGPU_OK;
        int phys = -1;
        HIP_TRY(hipGetDevice(&phys));
        if (modgpu_xfer_device_of(dev_results, count * sizeof(modgpu_digest_result_t)) != phys)
            return fail(MODGPU_ERR_INVALID, "the results are not device memory of the call's device");
        HIP_TRY(hipMemcpy(host_out, dev_results, count * sizeof(modgpu_digest_result_t), hipMemcpyDeviceToHost));
        if (adler32_out)
            for (uint64_t i = 0; i < count; ++i) adler32_out[i] = modgpu_digest_adler32(host_out + i);
        return MODGPU_OK;
    });
}

uint64_t modgpu_digest_check_bits_bytes(uint64_t n_entries) { return digest_check_bits_bytes(n_entries); }

int modgpu_digest_check_device(const modgpu_digest_result_t *dev_records, const uint32_t *dev_expect, uint64_t n_entries, const void *dev_table_workspace,
                               modgpu_digest_check_summary_t *dev_summary, uint64_t *dev_bad_bits, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return digest_check_impl(dev_records, dev_expect, n_entries, dev_table_workspace, dev_summary, dev_bad_bits, device, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_digest_check_summary(const modgpu_digest_check_summary_t *dev_summary, int device, modgpu_digest_check_summary_t *host_out)
{
    return guarded([&]() -> int {
        modgpu_digest_check_summary_t s;
        if (int rc = read_workspace_top(dev_summary, host_out != nullptr, device, &s, sizeof s, "null summary or out pointer",
                                        "the summary is not device memory of the call's device"))
            return rc;
        *host_out = s;
        if (s.refused != 0)
            return fail(MODGPU_ERR_INVALID, "the table call that produced the records was refused (nothing was compared; modgpu_table_status names the entry)");
        return MODGPU_OK;
    });
}

uint64_t modgpu_table_workspace_bytes(uint64_t n_entries)
{
    return n_entries == 0 || n_entries > kTableMaxEntries ? 0 : table_layout(n_entries).bytes;
}

int modgpu_cycle_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, void *dev_workspace, uint64_t workspace_bytes,
                              int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return table_impl(dev_entries, n_entries, nullptr, 0u, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

uint64_t modgpu_cycle_digest_table_workspace_bytes(uint64_t n_entries)
{
    return n_entries == 0 || n_entries > kTableMaxEntries ? 0 : table_layout(n_entries).bytes;
}

int modgpu_cycle_digest_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, modgpu_digest_result_t *dev_records, uint32_t side,
                                     void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return cycle_digest_table_impl(dev_entries, n_entries, dev_records, side, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_table_status(const void *dev_workspace, int device, uint64_t *first_bad_entry)
{
    return guarded([&]() -> int {
        CycleTableHdr h;
        if (int rc = read_workspace_top(dev_workspace, first_bad_entry != nullptr, device, &h, sizeof h)) return rc;
        *first_bad_entry = h.first_bad;
        if (h.first_bad != kTableNoBad)
            return fail(MODGPU_ERR_INVALID, "the device refused entry " + std::to_string(h.first_bad) + " (the call wrote nothing)");
        return MODGPU_OK;
    });
}

int modgpu_table_validate(const modgpu_table_entry_t *host_entries, uint64_t n_entries)
{
    return guarded([&]() -> int { return table_validate_impl(host_entries, n_entries); });
}

uint64_t modgpu_rekey_table_workspace_bytes(uint64_t n_entries)
{
    return n_entries == 0 || n_entries > kTableMaxEntries ? 0 : rekey_table_layout(n_entries).bytes;
}

int modgpu_rekey_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, void *dev_workspace, uint64_t workspace_bytes,
                              int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return rekey_table_impl(dev_entries, n_entries, nullptr, 0u, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

uint64_t modgpu_rekey_digest_table_workspace_bytes(uint64_t n_entries) { return modgpu_rekey_table_workspace_bytes(n_entries); }

int modgpu_rekey_digest_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, modgpu_digest_result_t *dev_records, uint32_t side,
                                     void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return rekey_digest_table_impl(dev_entries, n_entries, dev_records, side, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_rekey_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries)
{
    return guarded([&]() -> int { return table_validate_impl(host_entries, n_entries); });
}

uint64_t modgpu_rekey_move_table_workspace_bytes(uint64_t n_entries, uint64_t total_bytes)
{
    return move_table_sizes_ok(n_entries, total_bytes) ? move_table_layout(n_entries, total_bytes).bytes : 0;
}

int modgpu_rekey_move_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, uint64_t total_bytes, void *dev_workspace,
                                   uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return rekey_move_table_impl(dev_entries, n_entries, total_bytes, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_rekey_move_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries)
{
    return guarded([&]() -> int { return rekey_move_table_validate_impl(host_entries, n_entries); });
}

int modgpu_rekey_relayout_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, uint64_t total_bytes, void *dev_workspace,
                                       uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return rekey_move_table_impl(dev_entries, n_entries, total_bytes, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream), true);
    });
}

int modgpu_rekey_relayout_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries)
{
    return guarded([&]() -> int { return rekey_move_table_validate_impl(host_entries, n_entries, false); });
}

int modgpu_rekey_move_table_status(const void *dev_workspace, int device, uint64_t *first_bad_entry, uint64_t *stalled_chunk)
{
    return guarded([&]() -> int {
        if (!dev_workspace || !first_bad_entry || !stalled_chunk) return fail(MODGPU_ERR_INVALID, "null workspace or out pointer");
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        int phys = -1;
        HIP_TRY(hipGetDevice(&phys));
        if (modgpu_xfer_device_of(dev_workspace, sizeof(MoveTableHdr)) != phys)
            return fail(MODGPU_ERR_INVALID, "the workspace is not device memory of the call's device");
        MoveTableHdr h;
        HIP_TRY(hipMemcpy(&h, dev_workspace, sizeof h, hipMemcpyDeviceToHost));
        *first_bad_entry = h.first_bad;
        *stalled_chunk = h.stalled ? (uint64_t)h.stalled - 1 : UINT64_MAX;
        if (h.first_bad != kTableNoBad)
            return fail(MODGPU_ERR_INVALID, "the device refused entry " + std::to_string(h.first_bad) + " (the call wrote nothing)");
        if (h.stalled)
            return fail(MODGPU_ERR_HIP, "move table: the wait of chunk " + std::to_string(h.stalled - 1) + " ran out (the destinations are unspecified)");
        return MODGPU_OK;
    });
}

uint64_t modgpu_verify_table_workspace_bytes(uint64_t n_entries)
{
    return n_entries == 0 || n_entries > kTableMaxEntries ? 0 : verify_table_layout(n_entries).bytes;
}

int modgpu_verify_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, modgpu_verify_result_t *dev_results, void *dev_workspace,
                               uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return verify_table_impl(dev_entries, n_entries, dev_results, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

uint64_t modgpu_digest_table_workspace_bytes(uint64_t n_entries)
{
    return n_entries == 0 || n_entries > kTableMaxEntries ? 0 : table_layout(n_entries).bytes;
}

int modgpu_digest_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, modgpu_digest_result_t *dev_results, void *dev_workspace,
                               uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return digest_table_impl(dev_entries, n_entries, dev_results, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

uint64_t modgpu_verify_rekey_table_workspace_bytes(uint64_t n_entries)
{
    return n_entries == 0 || n_entries > kTableMaxEntries ? 0 : rekey_verify_table_layout(n_entries).bytes;
}

int modgpu_verify_rekey_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, modgpu_verify_result_t *dev_results,
                                     void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream)
{
    return guarded([&]() -> int {
        return verify_rekey_table_impl(dev_entries, n_entries, dev_results, dev_workspace, workspace_bytes, device, static_cast<hipStream_t>(hip_stream));
    });
}

int modgpu_verify_table_summary(const void *dev_workspace, int device, modgpu_verify_table_summary_t *out)
{
    return guarded([&]() -> int {
        struct {
            CycleTableHdr h;
            VerifyTableSummary s;
        } top;
        if (int rc = read_workspace_top(dev_workspace, out != nullptr, device, &top, sizeof top)) return rc;
        if (top.h.first_bad != kTableNoBad)
            return fail(MODGPU_ERR_INVALID, "the device refused entry " + std::to_string(top.h.first_bad) + " (the call wrote no result)");
        out->mismatches = top.s.mismatches;
        out->first_bad_entry = top.s.first_bad_entry;
        out->entries = top.s.entries;
        out->reserved = 0;
        return MODGPU_OK;
    });
}

int modgpu_cycle_host(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int device)
{
    return guarded([&]() -> int { return cycle_host_impl(host_buf, n, key, stream_off, device); });
}

int modgpu_cycle_scalar_host(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off)
{
    return guarded([&]() -> int { return scalar_impl(host_buf, n, key, stream_off); });
}

// What CEncryptionCycler::Cycle does with a caller-owned host buffer -- shared by modgpu_cycle_auto_host and the
// header framing of Cycle's call sites (modgpu_hdr_*_host).
static int cycle_auto_impl(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int device)
{
    // `if (n < threshold || !gpu_ok) cpu_loop(); else ...`.  The reference's call sites pass headers
    // (CArk.cpp:338-339, 1135-1136, Modulate.cpp:485-486; <= 512 KiB by CArk.cpp:911-912): below the measured
    // crossover the host loop is the faster engine.  MODGPU_REQUIRE_GPU=1 keeps every size on the kernel.
    if (n < min_gpu_bytes() && !gpu_required()) {
        int rc = scalar_impl(host_buf, n, key, stream_off);
        if (rc == MODGPU_OK && n) g_stats.auto_small.fetch_add(1, std::memory_order_relaxed);
        return rc;
    }
    if (host_policy() == HostPolicy::Fastest && !gpu_required() && logical_count() > 0 &&
        crossover::host_us(n, modgpu_scalar_isa(), modgpu_scalar_threads_for(n)) < crossover::kernel_us(n, host_range_pinned(host_buf, n))) {
        int rc = scalar_impl(host_buf, n, key, stream_off);
        if (rc == MODGPU_OK) g_stats.auto_policy_host.fetch_add(1, std::memory_order_relaxed);
        return rc;
    }
    // The reference's Cycle cannot fail (CEncryptionCycler.cpp:4-14; its callers at CArk.cpp:338-339, 1135-1136 and
    // Modulate.cpp:485-486 do not guard it).  A GPU lost AFTER the call has begun is handled inside the route: the staged route
    // knows which pieces have reached host_buf and lets the host loop do the others (host_stream.cpp).
    StreamOutcome outcome;
    int rc = cycle_host_impl(host_buf, n, key, stream_off, device, /*host_may_finish=*/!gpu_required(), &outcome);
    if (rc == MODGPU_OK && outcome.finished_on_host) g_stats.auto_fallbacks.fetch_add(1, std::memory_order_relaxed);
    if (rc == MODGPU_OK || rc == MODGPU_ERR_INVALID) return rc;
    // No GPU, or the attempt failed before it had changed host_buf: the host loop does the whole buffer.  What is left as an
    // error: the caller forbade the host loop, or one kernel working in place on page-locked caller memory died under way --
    // nobody knows which bytes it had written and the plaintext exists nowhere else.
    if (gpu_required() || outcome.touched) return rc;
    const std::string why = t_err;
    rc = scalar_impl(host_buf, n, key, stream_off);
    if (rc == MODGPU_OK) g_stats.auto_fallbacks.fetch_add(1, std::memory_order_relaxed);
    else t_err = why;
    return rc;
}

int modgpu_cycle_auto_host(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int device)
{
    return guarded([&]() -> int { return cycle_auto_impl(host_buf, n, key, stream_off, device); });
}

int modgpu_hdr_decrypt_host(uint8_t *hdr, uint64_t size, int device)
{
    return guarded([&]() -> int {
        if (!hdr || size < 4) return fail(MODGPU_ERR_INVALID, "header shorter than its magic");
        uint32_t magic = load_le32(hdr);
        if (magic != MODGPU_MAGIC_PS3 && magic != MODGPU_MAGIC_PS4)
            return fail(MODGPU_ERR_MAGIC, "unknown header magic");
        uint32_t key = magic == MODGPU_MAGIC_PS3 ? MODGPU_KEY_PS3 : MODGPU_KEY_PS4;
        return cycle_auto_impl(hdr + 4, size - 4, (int32_t)key, 0, device);
    });
}

int modgpu_hdr_encrypt_host(uint8_t *hdr, uint64_t size, int ps4, int device)
{
    return guarded([&]() -> int {
        if (!hdr || size < 4) return fail(MODGPU_ERR_INVALID, "header shorter than its magic");
        // cipher first: on failure the caller's buffer is left as it was
        int rc = cycle_auto_impl(hdr + 4, size - 4, (int32_t)(ps4 ? MODGPU_KEY_PS4 : MODGPU_KEY_PS3), 0, device);
        if (rc) return rc;
        store_le32(hdr, ps4 ? MODGPU_MAGIC_PS4 : MODGPU_MAGIC_PS3);
        return MODGPU_OK;
    });
}

// Host buffers spread over the GPUs, buffer i -> GPU i mod N, one host thread per GPU, each buffer its own stream from offs[i]
// (nullptr: 0).  No inter-GPU traffic.
static int parts_host_impl(uint8_t *const *parts, const uint64_t *sizes, const uint64_t *offs, int n_parts, int32_t key, int n_devices)
{
    int avail = logical_count();
    if (avail <= 0) return fail(MODGPU_ERR_NO_DEVICE, "no HIP device visible");
    if (n_devices <= 0 || n_devices > avail) n_devices = avail;
    n_devices = std::min(n_devices, std::max(n_parts, 1));
    std::vector<int> rcs((size_t)n_devices, MODGPU_OK);
    std::vector<std::string> errs((size_t)n_devices);
    auto body = [&](int d, bool own_thread) {
        if (own_thread) run_near_device(d); // this worker's copies run on the socket its GPU hangs off
        for (int i = d; i < n_parts; i += n_devices) { // part i -> GPU i mod N
            int rc = cycle_host_impl(parts[i], sizes[i], key, offs ? offs[i] : 0, d);
            if (rc) {
                rcs[d] = rc;
                errs[d] = t_err;
                return;
            }
        }
    };
    std::vector<std::thread> workers;
    int started = 1; // device 0's parts are done on the calling thread
    try {
        for (int d = 1; d < n_devices; ++d, ++started) workers.emplace_back(body, d, true);
    } catch (...) { // thread limit: the remaining devices' parts are done here, one device after another
    }
    body(0, false);
    for (int d = started; d < n_devices; ++d) body(d, false);
    for (auto &w : workers) w.join();
    for (int d = 0; d < n_devices; ++d)
        if (rcs[d]) {
            t_err = errs[d];
            return rcs[d];
        }
    return MODGPU_OK;
}

int modgpu_cycle_parts_host(uint8_t *const *parts, const uint64_t *sizes, int n_parts, int32_t key,
                            int n_devices)
{
    return guarded([&]() -> int {
        if (n_parts < 0 || (n_parts > 0 && (!parts || !sizes))) return fail(MODGPU_ERR_INVALID, "bad part list");
        return parts_host_impl(parts, sizes, nullptr, n_parts, key, n_devices);
    });
}

// ONE host buffer over several GPUs ("a single buffer can also be split at any byte offset using stream_off" --
// jump-ahead makes every span an independent stream): contiguous spans, span d on GPU d with stream offset stream_off + its
// position, each through its own PCIe link.  Spans are whole multiples of 2 MiB and at least 64 MiB, so a small buffer stays
// on one GPU.
int modgpu_cycle_host_split(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int n_devices)
{
    return guarded([&]() -> int {
        if (n && !host_buf) return fail(MODGPU_ERR_INVALID, "null host buffer");
        const int avail = logical_count();
        if (avail <= 0) return fail(MODGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (n_devices <= 0 || n_devices > avail) n_devices = avail;
        constexpr uint64_t kGrain = 2ull << 20, kMinSpan = 64ull << 20;
        const uint64_t use = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_devices, n / kMinSpan));
        const uint64_t span = ((n + use - 1) / use + kGrain - 1) / kGrain * kGrain;
        std::vector<uint8_t *> parts;
        std::vector<uint64_t> sizes, offs;
        const uint64_t base = stream_off % lcg::PERIOD; // reduced first: stream_off + position must not wrap at 2^64
        for (uint64_t at = 0; at < n; at += span) {
            parts.push_back(host_buf + at);
            sizes.push_back(std::min<uint64_t>(span, n - at));
            offs.push_back(base + at);
        }
        return parts_host_impl(parts.data(), sizes.data(), offs.data(), (int)parts.size(), key, (int)use);
    });
}

// modgpu_cycle_parts_device launches on a stream of its OWN per logical device -- non-blocking, created on first use, kept --
// not on the legacy NULL stream: that one synchronises implicitly with every blocking stream of the process, so a caller with
// work of its own on such streams would get a serialisation it did not ask for (VERDICT r3 weak #9b).  Concurrent calls share the
// device's stream: their launches queue behind each other, and each waits for all of them.
// What the NULL stream did give a caller is kept: work the caller queued BEFORE the call on the NULL stream or on any
// blocking stream -- an asynchronous upload or memset of a part, a producer kernel, torch's default stream -- is finished before
// the cycle kernels start.  An event recorded on the NULL stream at entry stands for all of that (the legacy stream waits for
// every blocking stream), and the private stream waits for the event: the caller's earlier work is ordered in front of the parts'
// kernels without a single kernel running on the NULL stream.  (Work on the caller's own NON-blocking streams is the caller's
// to synchronise, as with any HIP API; modgpu.h says so.)
struct PartsLane {
    hipStream_t stream = nullptr;
    hipEvent_t after_callers_work = nullptr;
};
static PartsLane parts_lane(int logical)
{
    static std::mutex mu;
    static PartsLane lanes[kMaxDevices] = {};
    if (logical < 0 || logical >= kMaxDevices) return PartsLane{};
    std::lock_guard<std::mutex> lock(mu);
    PartsLane &l = lanes[logical];
    if (!l.stream && hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        l.stream = nullptr; // (the NULL stream still gives the right bytes, and its own ordering)
    }
    if (l.stream && !l.after_callers_work && hipEventCreateWithFlags(&l.after_callers_work, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        l.after_callers_work = nullptr;
    }
    return l;
}
// The stream a device's parts are launched on, already waiting for whatever the caller queued on the NULL / blocking streams.
static hipStream_t parts_stream_after_callers_work(int logical)
{
    const PartsLane l = parts_lane(logical);
    if (!l.stream) return nullptr;
    if (!l.after_callers_work || hipEventRecord(l.after_callers_work, nullptr) != hipSuccess || hipStreamWaitEvent(l.stream, l.after_callers_work, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr; // no way to order: fall back to the NULL stream itself, which is ordered by definition
    }
    return l.stream;
}

int modgpu_cycle_parts_device(void *const *dev_parts, const uint64_t *sizes, const int *devices, int n_parts, int32_t key)
{
    return guarded([&]() -> int {
        if (n_parts < 0 || (n_parts > 0 && (!dev_parts || !sizes || !devices))) return fail(MODGPU_ERR_INVALID, "bad part list");
        DeviceScope keep(-1, /*always_save=*/true); // this thread visits every part's GPU and leaves as it came
        int rc = MODGPU_OK;
        for (int i = 0; i < n_parts && rc == MODGPU_OK; ++i)
            if (devices[i] < 0) rc = fail(MODGPU_ERR_INVALID, "a part needs an explicit device");
        if (rc != MODGPU_OK) return rc;
        // every part its own Cycle from stream offset 0; the parts of one device go to it together (cycle_batch_impl)
        std::vector<char> taken((size_t)n_parts, 0);
        std::vector<int> started;
        std::vector<hipStream_t> started_on;
        for (int i = 0; i < n_parts && rc == MODGPU_OK; ++i) {
            if (taken[(size_t)i]) continue;
            std::vector<void *> bufs;
            std::vector<uint64_t> lens;
            for (int j = i; j < n_parts; ++j)
                if (devices[j] == devices[i]) {
                    taken[(size_t)j] = 1;
                    bufs.push_back(dev_parts[j]);
                    lens.push_back(sizes[j]);
                }
            rc = select_device(devices[i]);
            if (rc == MODGPU_OK) {
                hipStream_t st = parts_stream_after_callers_work(devices[i]);
                started.push_back(devices[i]);
                started_on.push_back(st);
                rc = cycle_batch_impl(bufs.data(), lens.data(), nullptr, (int)bufs.size(), key, st);
            }
        }
        const std::string why = t_err;
        for (size_t k = 0; k < started.size(); ++k) { // wait for what was started, also on the error path
            if (select_device(started[k]) != MODGPU_OK) continue;
            hipError_t e = hipStreamSynchronize(started_on[k]);
            if (e != hipSuccess && rc == MODGPU_OK) rc = fail_hip(e, "hipStreamSynchronize");
        }
        if (rc != MODGPU_OK && !why.empty()) t_err = why;
        return rc;
    });
}

int modgpu_host_alloc(void **host_ptr, uint64_t n)
{
    return guarded([&]() -> int {
        if (!host_ptr) return fail(MODGPU_ERR_INVALID, "null out pointer");
        *host_ptr = nullptr;
        const uint64_t bytes = n ? n : 1;
        void *p = nullptr;
        bool pinned = false;
        if (physical_count() > 0) {
            // portable + mapped: every device's DMA engines and kernels reach these pages
            if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess) pinned = true;
            else { // e.g. the locked-memory limit: ordinary memory still works, through the staged route
                (void)hipGetLastError();
                p = nullptr;
            }
        }
        if (!p && ::posix_memalign(&p, 64, bytes) != 0) return fail(MODGPU_ERR_INVALID, "out of host memory");
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            g_host_ranges.push_back({reinterpret_cast<uintptr_t>(p), bytes, pinned, pinned ? HostKind::HipHost : HostKind::Plain});
        }
        *host_ptr = p;
        return MODGPU_OK;
    });
}

int modgpu_host_free(void *host_ptr)
{
    return guarded([&]() -> int {
        if (!host_ptr) return MODGPU_OK;
        HostRange r{};
        bool found = false;
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            for (size_t i = 0; i < g_host_ranges.size(); ++i)
                if (g_host_ranges[i].base == reinterpret_cast<uintptr_t>(host_ptr) && g_host_ranges[i].kind != HostKind::Registered) {
                    r = g_host_ranges[i];
                    g_host_ranges.erase(g_host_ranges.begin() + (long)i);
                    found = true;
                    break;
                }
        }
        if (!found) return fail(MODGPU_ERR_INVALID, "not a modgpu_host_alloc pointer");
        if (r.kind == HostKind::Placed) {
            hipError_t e = r.pinned ? hipHostUnregister(host_ptr) : hipSuccess;
            numa::release(host_ptr, r.size);
            if (e != hipSuccess) return fail_hip(e, "hipHostUnregister");
        } else if (r.kind == HostKind::HipHost) {
            HIP_TRY(hipHostFree(host_ptr));
        } else {
            std::free(host_ptr);
        }
        return MODGPU_OK;
    });
}

namespace {
constexpr int kPrefaultThreads = 8; // first touch of a placed allocation (numa_place.h: prefault)
}

int modgpu_host_alloc_parts(void **host_ptr, const uint64_t *sizes, int n_parts, int n_devices)
{
    return guarded([&]() -> int {
        if (!host_ptr || n_parts < 0 || (n_parts > 0 && !sizes)) return fail(MODGPU_ERR_INVALID, "bad part list");
        *host_ptr = nullptr;
        uint64_t total = 0;
        for (int i = 0; i < n_parts; ++i) total += sizes[i];
        const int avail = logical_count();
        if (n_devices <= 0 || n_devices > avail) n_devices = avail;
        // without a GPU, or with placement switched off, this is modgpu_host_alloc
        if (avail <= 0 || !numa::enabled()) return modgpu_host_alloc(host_ptr, total);
        const uint64_t bytes = total ? total : 1;
        void *p = numa::reserve(bytes);
        if (!p) return fail(MODGPU_ERR_INVALID, "out of host memory");
        // part i -> GPU i mod n_devices (the rule of modgpu_cycle_parts_host): its whole pages go to that GPU's node
        // (a page shared by two parts stays with the default policy); pages are faulted in by the registration below
        uint64_t off = 0;
        for (int i = 0; i < n_parts; ++i) {
            const int node = device_numa_node(i % n_devices);
            (void)numa::prefer_node(static_cast<uint8_t *>(p) + off, sizes[i], node);
            numa::prefault(static_cast<uint8_t *>(p) + off, sizes[i], kPrefaultThreads, "/sys", node);
            off += sizes[i];
        }
        bool pinned = hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped) == hipSuccess;
        if (!pinned) (void)hipGetLastError(); // e.g. the locked-memory limit: ordinary memory, staged route
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            g_host_ranges.push_back({reinterpret_cast<uintptr_t>(p), bytes, pinned, HostKind::Placed});
        }
        *host_ptr = p;
        return MODGPU_OK;
    });
}

int modgpu_host_alloc_near(void **host_ptr, uint64_t n, int device)
{
    return guarded([&]() -> int {
        if (!host_ptr) return fail(MODGPU_ERR_INVALID, "null out pointer");
        const int avail = logical_count();
        if (avail > 0 && (device < 0 || device >= avail)) return fail(MODGPU_ERR_INVALID, "device index out of range");
        if (avail <= 0 || device_numa_node(device) < 0) return modgpu_host_alloc(host_ptr, n); // nothing to place by
        *host_ptr = nullptr;
        const uint64_t bytes = n ? n : 1;
        void *p = numa::reserve(bytes);
        if (!p) return fail(MODGPU_ERR_INVALID, "out of host memory");
        (void)numa::prefer_node(p, bytes, device_numa_node(device));
        numa::prefault(p, bytes, kPrefaultThreads, "/sys", device_numa_node(device));
        bool pinned = hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped) == hipSuccess;
        if (!pinned) (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            g_host_ranges.push_back({reinterpret_cast<uintptr_t>(p), bytes, pinned, HostKind::Placed});
        }
        *host_ptr = p;
        return MODGPU_OK;
    });
}

int modgpu_host_alloc_on_node(void **host_ptr, uint64_t n, int node)
{
    return guarded([&]() -> int {
        if (!host_ptr || node < 0) return fail(MODGPU_ERR_INVALID, "null out pointer or negative node");
        *host_ptr = nullptr;
        const uint64_t bytes = n ? n : 1;
        void *p = numa::reserve(bytes);
        if (!p) return fail(MODGPU_ERR_INVALID, "out of host memory");
        if (numa::prefer_node(p, bytes, node) != 0) {
            numa::release(p, bytes);
            return fail(MODGPU_ERR_INVALID, "mbind refused that node");
        }
        numa::prefault(p, bytes, kPrefaultThreads, "/sys", -1);
        bool pinned = physical_count() > 0 && hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped) == hipSuccess;
        if (!pinned) (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            g_host_ranges.push_back({reinterpret_cast<uintptr_t>(p), bytes, pinned, HostKind::Placed});
        }
        *host_ptr = p;
        return MODGPU_OK;
    });
}

int modgpu_device_numa_node(int device)
{
    if (device < 0 || device >= logical_count()) return -1;
    return device_numa_node(device);
}

int modgpu_host_register(void *host_ptr, uint64_t n)
{
    return guarded([&]() -> int {
        if (!host_ptr || n == 0) return fail(MODGPU_ERR_INVALID, "null or empty range");
        if (physical_count() <= 0) return MODGPU_OK; // nothing to pin for: the host loop reads any memory
        hipError_t e = hipHostRegister(host_ptr, n, hipHostRegisterPortable | hipHostRegisterMapped);
        if (e != hipSuccess) return fail_hip(e, "hipHostRegister");
        std::lock_guard<std::mutex> lock(g_host_mu);
        g_host_ranges.push_back({reinterpret_cast<uintptr_t>(host_ptr), n, true, HostKind::Registered});
        return MODGPU_OK;
    });
}

int modgpu_host_unregister(void *host_ptr)
{
    return guarded([&]() -> int {
        if (!host_ptr || physical_count() <= 0) return MODGPU_OK;
        bool found = false;
        {
            std::lock_guard<std::mutex> lock(g_host_mu);
            for (size_t i = 0; i < g_host_ranges.size(); ++i)
                if (g_host_ranges[i].base == reinterpret_cast<uintptr_t>(host_ptr) && g_host_ranges[i].kind == HostKind::Registered) {
                    g_host_ranges.erase(g_host_ranges.begin() + (long)i);
                    found = true;
                    break;
                }
        }
        if (!found) return fail(MODGPU_ERR_INVALID, "not a modgpu_host_register range");
        HIP_TRY(hipHostUnregister(host_ptr));
        return MODGPU_OK;
    });
}

int modgpu_host_is_pinned(const void *p, uint64_t n) { return host_range_pinned(p, n) ? 1 : 0; }

int modgpu_path_stats(modgpu_path_stats_t *out, int reset)
{
    if (!out) return fail(MODGPU_ERR_INVALID, "null out pointer");
    auto take = [&](std::atomic<uint64_t> &c) { return reset ? c.exchange(0) : c.load(); };
    out->gpu_calls = take(g_stats.gpu_calls);
    out->gpu_bytes = take(g_stats.gpu_bytes);
    out->gpu_launches = take(g_stats.gpu_launches);
    out->scalar_calls = take(g_stats.scalar_calls);
    out->scalar_bytes = take(g_stats.scalar_bytes);
    out->staged_bytes = take(g_stats.staged_bytes);
    out->direct_bytes = take(g_stats.direct_bytes);
    out->auto_fallbacks = take(g_stats.auto_fallbacks);
    out->midcall_rescues = take(g_stats.midcall_rescues);
    out->midcall_rescued_bytes = take(g_stats.midcall_rescued_bytes);
    out->auto_small = take(g_stats.auto_small);
    out->auto_policy_host = take(g_stats.auto_policy_host);
    return MODGPU_OK;
}

int modgpu_gpu_required(void) { return gpu_required() ? 1 : 0; }

uint64_t modgpu_min_gpu_bytes(void) { return min_gpu_bytes(); }

void modgpu_host_loop_info(uint64_t out[4]) { modgpu_scalar_info(out); }

const char *modgpu_host_policy(void) { return host_policy() == HostPolicy::Fastest ? "fastest" : "offload"; }

int modgpu_host_policy_engine(uint64_t n, int pinned, double *host_us, double *kernel_us)
{
    const double h = crossover::host_us(n, modgpu_scalar_isa(), modgpu_scalar_threads_for(n)), k = crossover::kernel_us(n, pinned != 0);
    if (host_us) *host_us = h;
    if (kernel_us) *kernel_us = k;
    return h < k ? 1 : 0;
}

const char *modgpu_host_loop_isa(void) { return modgpu_scalar_isa_name(modgpu_scalar_isa()); }

int modgpu_alloc(void **dev_ptr, uint64_t n, int device)
{
    return guarded([&]() -> int {
        if (!dev_ptr) return fail(MODGPU_ERR_INVALID, "null out pointer");
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        HIP_TRY(hipMalloc(dev_ptr, n ? n : 1));
        prepare_device();
        return MODGPU_OK;
    });
}

int modgpu_free(void *dev_ptr, int device)
{
    return guarded([&]() -> int {
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        HIP_TRY(hipFree(dev_ptr));
        return MODGPU_OK;
    });
}

// The chip's shader engines go to sleep within a fraction of a second without kernels -- an upload keeps only the DMA engines
// busy -- and the first launch after that pays their wake-up: ~15 us on a 411 MB launch, ~40 us for a one-wave kernel by the host's
// clock (profiles/r05_first_launch.txt; BENCH_r04 had the chip's first 411 MB launch after the upload at 0.529 of peak, the next
// at 0.816).  A part that is being uploaded is about to be cycled, and this library is the one doing the upload: when a copy
// STARTS, an empty launch (zero words, one workgroup) goes to a stream of the library's own that nobody waits for, so the engines
// wake while the DMA engine works.  Measured: first launch after a 1.5 s pause + upload 0.1420 -> 0.1262 ms at 411 MB, which is
// the size's own rate (0.1261).  Best effort; costs the caller one asynchronous launch call per copy of 1 MiB or more.
static void wake_shader_engines()
{
    static std::mutex mu;
    static hipStream_t streams[kMaxDevices] = {}; // by PHYSICAL device: a stream belongs to the device it was created on, whatever logical
                                                  // index (MODGPU_DEVICE_ALIAS) or "current device" (-1) the caller named it by
    int phys = -1;
    if (hipGetDevice(&phys) != hipSuccess || phys < 0 || phys >= kMaxDevices) {
        (void)hipGetLastError();
        return;
    }
    hipStream_t st;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (!streams[phys] && hipStreamCreateWithFlags(&streams[phys], hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            streams[phys] = nullptr;
            return;
        }
        st = streams[phys];
    }
    CycleArgs a{}; // no head, no words, no tail: the one workgroup finds nothing to do
    a.base_head = a.base_body = a.base_tail = 1;
    a.stride_mul2 = 2;
    (void)modgpu_launch_cycle(a, CYCLE_SMALL, 1, st);
    (void)hipGetLastError();
}

int modgpu_h2d(void *dev_dst, const void *host_src, uint64_t n, int device)
{
    return guarded([&]() -> int {
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        if (n >= (1ull << 20)) wake_shader_engines(); // (the scope has made the device current)
        if (n) HIP_TRY(hipMemcpy(dev_dst, host_src, n, hipMemcpyHostToDevice));
        return MODGPU_OK;
    });
}

int modgpu_prepare(int device)
{
    return guarded([&]() -> int {
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        prepare_device();      // once per device and process: code object, ticket ring, the first real work-queue launches
        wake_shader_engines(); // every call: one empty launch on a private stream nobody waits for
        return MODGPU_OK;
    });
}

int modgpu_d2h(void *host_dst, const void *dev_src, uint64_t n, int device)
{
    return guarded([&]() -> int {
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        if (n) HIP_TRY(hipMemcpy(host_dst, dev_src, n, hipMemcpyDeviceToHost));
        return MODGPU_OK;
    });
}

int modgpu_sync(int device, void *hip_stream)
{
    return guarded([&]() -> int {
        DeviceScope scope(device);
        if (scope.rc) return scope.rc;
        HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)));
        return MODGPU_OK;
    });
}

uint32_t modgpu_state_at(int32_t key, uint64_t i)
{
    uint32_t r = lcg::state_residue(lcg::key_residue(key), i);
    return r ? r : lcg::M; // the reference shows residue 0 as m (CEncryptionCycler.cpp:19-22)
}

int modgpu_jump_table(int which, uint32_t *out, int count)
{
    if (!out || count < 0) return 0;
    const uint32_t *src = nullptr;
    int n = 0;
    switch (which) {
    case 0: src = lcg::kBytePow.v; n = 16; break;
    case 1: src = lcg::kLanePow.v; n = 256; break;
    case 2: src = lcg::kTileLo.v; n = 256; break;
    case 3: src = lcg::kTileHi.v; n = 256; break;
    default: return 0;
    }
    n = std::min(n, count);
    std::memcpy(out, src, (size_t)n * sizeof(uint32_t));
    return n;
}

// ---- include/modgpu_testing.h ------------------------------------------------------------------

int modgpu_time_cycle_device(void *dev_buf, uint64_t n, int32_t key, uint64_t stream_off, int device,
                             void *hip_stream, int iters, float *ms_per_launch)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_launch, [&](hipStream_t st) { return cycle_device_impl(dev_buf, n, key, stream_off, st); });
    });
}

int modgpu_time_cycle_device_to(void *dev_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off, int device,
                                void *hip_stream, int iters, float *ms_per_launch)
{
    return guarded([&]() -> int {
        if (iters > 0 && ms_per_launch) // (the entries are checked behind the timing arguments, which time_calls refuses)
            if (int rc = check_to_entries(&dev_dst, &dev_src, &n, 1)) return rc;
        return time_calls(device, hip_stream, iters, ms_per_launch, [&](hipStream_t st) { return cycle_to_impl(&dev_dst, &dev_src, &n, &stream_off, 1, key, st); });
    });
}

int modgpu_time_rekey_device_to(void *dev_dst, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to,
                                uint64_t off_to, int device, void *hip_stream, int iters, float *ms_per_launch)
{
    return guarded([&]() -> int {
        if (iters > 0 && ms_per_launch)
            if (int rc = check_to_entries(&dev_dst, &dev_src, &n, 1)) return rc;
        return time_calls(device, hip_stream, iters, ms_per_launch, [&](hipStream_t st) {
            return rekey_impl(&dev_dst, &dev_src, &n, &off_from, &off_to, 1, key_from, key_to, st);
        });
    });
}

int modgpu_time_verify_device(const void *dev_expect, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off, void *dev_result,
                              int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        modgpu_verify_result_t *res = static_cast<modgpu_verify_result_t *>(dev_result);
        if (iters > 0 && ms_per_call)
            if (int rc = check_verify_entries(&dev_expect, &dev_src, &n, 1, res)) return rc;
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return verify_impl(&dev_expect, &dev_src, &n, &stream_off, 1, key, res, st);
        });
    });
}

int modgpu_time_verify_rekey_device(const void *dev_expect, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to,
                                    uint64_t off_to, void *dev_result, int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        modgpu_verify_result_t *res = static_cast<modgpu_verify_result_t *>(dev_result);
        if (iters > 0 && ms_per_call)
            if (int rc = check_verify_entries(&dev_expect, &dev_src, &n, 1, res)) return rc;
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return verify_rekey_impl(&dev_expect, &dev_src, &n, &off_from, &off_to, 1, key_from, key_to, res, st);
        });
    });
}

int modgpu_time_digest_device(void *dev_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off, void *dev_result, int device,
                              void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        modgpu_digest_result_t *res = static_cast<modgpu_digest_result_t *>(dev_result);
        void *const *dst = dev_dst ? &dev_dst : nullptr;
        if (iters > 0 && ms_per_call)
            if (int rc = check_digest_entries(dst, &dev_src, &n, 1, res)) return rc;
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return digest_impl(dst, &dev_src, &n, &stream_off, 1, key, res, st);
        });
    });
}

int modgpu_last_launch(modgpu_launch_info_t *out)
{
    if (!out) return fail(MODGPU_ERR_INVALID, "null out pointer");
    if (!t_last_launch.kernel) return fail(MODGPU_ERR_INVALID, "no launch on this thread yet");
    *out = t_last_launch;
    return MODGPU_OK;
}

int modgpu_cycle_scalar_host_isa(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, const char *isa)
{
    return guarded([&]() -> int {
        for (int i = 0; isa && i < MODGPU_ISA_COUNT; ++i)
            if (std::strcmp(isa, modgpu_scalar_isa_name(i)) == 0) return scalar_impl(host_buf, n, key, stream_off, i);
        return fail(MODGPU_ERR_INVALID, "unknown host-loop body");
    });
}

int modgpu_numa_probe(const char *sysfs_root, const char *bdf, int *node, int *cpus, int max_cpus)
{
    if (!sysfs_root || !bdf || !node) return -1;
    *node = numa::node_of_pci(sysfs_root, bdf);
    const std::vector<int> list = numa::cpus_of_node(sysfs_root, *node);
    int n = 0;
    for (; n < (int)list.size() && cpus && n < max_cpus; ++n) cpus[n] = list[(size_t)n];
    return n;
}

void modgpu_queue_stats(uint64_t out[6])
{
    out[0] = g_queue_eager.load();
    out[1] = g_queue_busy.load();
    out[2] = g_queue_graph.load();
    out[3] = g_queue_graph_full.load();
    out[4] = g_batch_launches.load();
    out[5] = g_batch_parts.load();
}

const char *modgpu_kernel_source_hash(void) { return MODGPU_KERNEL_SOURCE_HASH; }
const char *modgpu_feed_kernel_source_hash(void) { return MODGPU_FEED_KERNEL_SOURCE_HASH; }
const char *modgpu_to_kernel_source_hash(void) { return MODGPU_TO_KERNEL_SOURCE_HASH; }
const char *modgpu_xfer_kernel_source_hash(void) { return MODGPU_XFER_KERNEL_SOURCE_HASH; }
const char *modgpu_rekey_kernel_source_hash(void) { return MODGPU_REKEY_KERNEL_SOURCE_HASH; }
const char *modgpu_table_kernel_source_hash(void) { return MODGPU_TABLE_KERNEL_SOURCE_HASH; }
const char *modgpu_rekey_table_kernel_source_hash(void) { return MODGPU_REKEY_TABLE_KERNEL_SOURCE_HASH; }
const char *modgpu_verify_kernel_source_hash(void) { return MODGPU_VERIFY_KERNEL_SOURCE_HASH; }
const char *modgpu_verify_table_kernel_source_hash(void) { return MODGPU_VERIFY_TABLE_KERNEL_SOURCE_HASH; }
const char *modgpu_rekey_verify_kernel_source_hash(void) { return MODGPU_REKEY_VERIFY_KERNEL_SOURCE_HASH; }
const char *modgpu_keep_kernel_source_hash(void) { return MODGPU_KEEP_KERNEL_SOURCE_HASH; }
const char *modgpu_rekey_verify_table_kernel_source_hash(void) { return MODGPU_REKEY_VERIFY_TABLE_KERNEL_SOURCE_HASH; }
const char *modgpu_rekey_move_table_kernel_source_hash(void) { return MODGPU_REKEY_MOVE_TABLE_KERNEL_SOURCE_HASH; }

int modgpu_keep_policy(uint64_t bytes, uint32_t *mask, uint32_t *run)
{
    const KeepPolicy k = keep_policy(bytes);
    if (mask) *mask = k.mask;
    if (run) *run = k.run;
    return k.route ? 1 : 0;
}

int modgpu_time_cycle_table_device(const void *dev_entries, uint64_t n_entries, void *dev_workspace, uint64_t workspace_bytes,
                                   int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return table_impl(static_cast<const modgpu_table_entry_t *>(dev_entries), n_entries, nullptr, 0u, dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_time_cycle_digest_table_device(const void *dev_entries, uint64_t n_entries, void *dev_records, uint32_t side, void *dev_workspace,
                                          uint64_t workspace_bytes, int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return cycle_digest_table_impl(static_cast<const modgpu_table_entry_t *>(dev_entries), n_entries, static_cast<modgpu_digest_result_t *>(dev_records), side, dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_time_rekey_table_device(const void *dev_entries, uint64_t n_entries, void *dev_workspace, uint64_t workspace_bytes,
                                   int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return rekey_table_impl(static_cast<const modgpu_rekey_table_entry_t *>(dev_entries), n_entries, nullptr, 0u, dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_time_rekey_digest_table_device(const void *dev_entries, uint64_t n_entries, void *dev_records, uint32_t side, void *dev_workspace,
                                          uint64_t workspace_bytes, int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return rekey_digest_table_impl(static_cast<const modgpu_rekey_table_entry_t *>(dev_entries), n_entries, static_cast<modgpu_digest_result_t *>(dev_records), side, dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_time_verify_table_device(const void *dev_entries, uint64_t n_entries, void *dev_results, void *dev_workspace, uint64_t workspace_bytes,
                                    int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return verify_table_impl(static_cast<const modgpu_table_entry_t *>(dev_entries), n_entries, static_cast<modgpu_verify_result_t *>(dev_results), dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_time_digest_table_device(const void *dev_entries, uint64_t n_entries, void *dev_results, void *dev_workspace, uint64_t workspace_bytes,
                                    int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return digest_table_impl(static_cast<const modgpu_table_entry_t *>(dev_entries), n_entries, static_cast<modgpu_digest_result_t *>(dev_results), dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_time_digest_check_device(const void *dev_records, const void *dev_expect, uint64_t n_entries, const void *dev_table_workspace, void *dev_summary,
                                    void *dev_bad_bits, int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return digest_check_impl(static_cast<const modgpu_digest_result_t *>(dev_records), static_cast<const uint32_t *>(dev_expect), n_entries, dev_table_workspace, static_cast<modgpu_digest_check_summary_t *>(dev_summary), static_cast<uint64_t *>(dev_bad_bits), -1, st);
        });
    });
}

int modgpu_time_verify_rekey_table_device(const void *dev_entries, uint64_t n_entries, void *dev_results, void *dev_workspace, uint64_t workspace_bytes,
                                          int device, void *hip_stream, int iters, float *ms_per_call)
{
    return guarded([&]() -> int {
        return time_calls(device, hip_stream, iters, ms_per_call, [&](hipStream_t st) {
            return verify_rekey_table_impl(static_cast<const modgpu_rekey_table_entry_t *>(dev_entries), n_entries, static_cast<modgpu_verify_result_t *>(dev_results), dev_workspace, workspace_bytes, -1, st);
        });
    });
}

int modgpu_testing_hooks(void)
{
#ifdef MODGPU_TESTING_HOOKS
    return 1;
#else
    return 0;
#endif
}

#ifdef MODGPU_TESTING_HOOKS
void modgpu_debug_set_launch(int variant, uint32_t grid_cap)
{
    g_force_variant.store(variant, std::memory_order_relaxed);
    g_grid_cap.store(grid_cap, std::memory_order_relaxed);
}

void modgpu_debug_set_pcie_grid(uint32_t cap) { g_pcie_grid.store(cap, std::memory_order_relaxed); }
void modgpu_debug_set_gpu_node(int node) { g_forced_gpu_node.store(node >= -1 ? node : -2, std::memory_order_relaxed); }
void modgpu_debug_set_pinned_mode(int mode) { g_pinned_mode.store(mode, std::memory_order_relaxed); }
void modgpu_debug_set_staged_mode(int mode) { g_staged_mode.store(mode, std::memory_order_relaxed); }

void modgpu_debug_set_helpers(int mode) { g_helper_mode.store(mode >= 0 && mode <= 2 ? mode : 0, std::memory_order_relaxed); }

void modgpu_debug_set_batch(int mode) { g_batch_mode.store(mode >= 0 && mode <= 2 ? mode : 0, std::memory_order_relaxed); }

void modgpu_debug_set_to_form(int form) { g_to_form.store(form < 0 ? kToFormShipped : form == CYCLE_TO_FUNNEL ? CYCLE_TO_FUNNEL : CYCLE_TO_PLAIN, std::memory_order_relaxed); }

void modgpu_debug_set_rekey_form(int shape)
{
    g_rekey_shape.store(shape < 0 ? kRekeyShapeShipped : shape == CYCLE_REKEY_SHAPE_ALL ? CYCLE_REKEY_SHAPE_ALL : CYCLE_REKEY_SHAPE_QUEUE,
                        std::memory_order_relaxed);
}

void modgpu_debug_set_table_grid(uint32_t grid) { force_table_grid(kCycleTable, grid); }
void modgpu_debug_set_move_grid(uint32_t grid) { g_move_grid.store(std::min<uint32_t>(grid, 4096u), std::memory_order_relaxed); }
void modgpu_debug_set_move_table_grid(uint32_t grid) { force_table_grid(kMoveTable, grid); }
void modgpu_debug_set_rekey_table_grid(uint32_t grid) { force_table_grid(kRekeyTable, grid); }
void modgpu_debug_set_rekey_digest_table_grid(uint32_t grid) { force_table_grid(kRekeyDigestTable, grid); }

void modgpu_debug_set_verify_table_grid(uint32_t grid) { force_table_grid(kVerifyTable, grid); }
void modgpu_debug_set_rekey_verify_table_grid(uint32_t grid) { force_table_grid(kRekeyVerifyTable, grid); }
void modgpu_debug_set_digest_table_grid(uint32_t grid) { force_table_grid(kDigestTable, grid); }
void modgpu_debug_set_cycle_digest_table_grid(uint32_t grid) { force_table_grid(kCycleDigestTable, grid); }

// (caps the compare launches of the verify call and of the rekey verify call alike)
void modgpu_debug_set_verify_form(int grid) { g_verify_grid.store(grid <= 0 ? 0u : std::min<uint32_t>((uint32_t)grid, 4096u), std::memory_order_relaxed); }

void modgpu_debug_set_digest_grid(int grid) { g_digest_grid.store(grid <= 0 ? 0u : std::min<uint32_t>((uint32_t)grid, 4096u), std::memory_order_relaxed); }

void modgpu_debug_set_keep(uint64_t min_bytes, uint32_t mask, uint32_t run)
{
    std::lock_guard<std::mutex> lock(g_keep_mutex);
    g_keep_min = min_bytes;
    g_keep_mask = min_bytes ? mask : 0u;
    g_keep_run = min_bytes ? run : 0u;
}

void modgpu_debug_set_queue_ring(uint32_t lines)
{
    g_ring_lines.store(lines == 0 ? kQueueRing : std::min(lines, kQueueRing), std::memory_order_relaxed);
}
#endif

} // extern "C"
