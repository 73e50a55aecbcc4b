// standin_launch_xfer_list.cpp -- the LIST mode of the transfer kernels (cycle_xfer_kernel.h: XferListRec, modgpu_launch_cycle_xfer_list)
// on the CPU stand-in (hip/hip_runtime.h).  Like standin_launch_xfer.cpp, which it leaves alone: a launch is queued on the stream's
// thread and runs WHILE the library's pipelines gather into and scatter out of their slots -- chunk after chunk of the PACKED stream it
// waits for `ready` (or `abort`, or its patience), moves the chunk between its slot and the entries' device sides byte by byte, each
// byte's entry found in the plan and its state taken from the entry's base with lcg.h's arithmetic, and marks the chunk `done`.  A
// second implementation, written from the record types and lcg.h: the sanitizer runs see every byte the plan says the kernel touches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_xfer_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_list_launches[2] = {}, g_list_gave_up{0}, g_list_plan_errors{0}, g_list_segments{0};
// modgpu_shim_wedge_next_xfer_list(1): the next list "kernel" stops responding half-way -- it neither finishes its chunks nor ends,
// whatever the abort word says -- until modgpu_shim_release_wedged_xfer_list() lets the stream's thread go.  (The plain stand-in's
// wedge lives in its own file and is not visible here.)
std::atomic<int> g_wedge_next{0};
std::atomic<bool> g_wedge_release{false};

struct ListLaunch {
    CycleXferArgs a;
    bool upload;
};

// the plan as the header states it: record 0 at 0, starts strictly increasing, no null device side, the terminator at the total
bool plan_ok(const CycleXferArgs &a)
{
    if (!a.list || a.list_n == 0 || a.list[0].start != 0 || a.slot_phase != 0 || a.chunk_bytes == 0 || a.chunk_bytes % kFeedPieceBytes != 0) return false;
    for (uint32_t e = 0; e < a.list_n; ++e)
        if (!a.list[e].dev || a.list[e].start >= a.list[e + 1].start || a.list[e + 1].start - a.list[e].start >= kXferListEntryMax || a.list[e].copy > 1u) return false;
    return a.list[a.list_n].start == a.n && a.list[a.list_n].dev == nullptr;
}

void run_list(void *arg)
{
    ListLaunch *l = static_cast<ListLaunch *>(arg);
    const CycleXferArgs &a = l->a;
    const bool good = plan_ok(a);
    if (!good) g_list_plan_errors.fetch_add(1);
    const uint64_t chunk = a.chunk_bytes ? a.chunk_bytes : kFeedPieceBytes;
    const uint64_t chunks = (a.n + chunk - 1) / chunk;
    const bool wedge = g_wedge_next.exchange(0) != 0;
    bool gave_up = !good; // (a bad plan moves nothing: the call then times out or fails its model, loudly)
    uint32_t e = 0;       // the entry of the byte at hand: only ever moves forward, the stream is walked in packed order
    for (uint64_t c = 0; c < chunks && !gave_up; ++c) {
        if (wedge && c == chunks / 2) {
            while (!g_wedge_release.load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            delete l; // (nothing of the call is touched any more: the library has long abandoned it)
            return;
        }
        const auto since = std::chrono::steady_clock::now();
        while (std::atomic_ref<const uint32_t>(a.ready[c]).load(std::memory_order_acquire) == 0u) {
            const double waited_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - since).count();
            if (std::atomic_ref<const uint32_t>(*a.abort).load(std::memory_order_acquire) != 0u || waited_s * 1e8 > (double)a.patience_ticks) {
                gave_up = true;
                break;
            }
            std::this_thread::yield();
        }
        if (gave_up) break;
        const uint64_t pos = c * chunk, len = std::min<uint64_t>(chunk, a.n - pos);
        uint8_t *const h = a.slot[(c % a.pipes) * 2 + (c / a.pipes) % 2];
        uint32_t state = 0;
        bool fresh = true; // the state has to be taken from the entry's base: the first byte of a chunk, and of every entry
        for (uint64_t j = 0; j < len; ++j) {
            const uint64_t p = pos + j;
            while (a.list[e + 1].start <= p) ++e, fresh = true;
            const XferListRec &r = a.list[e];
            const uint64_t into = p - r.start;
            if (fresh) {
                state = lcg::mulmod(r.base, lcg::powmod(lcg::A, into % lcg::PERIOD));
                fresh = false;
                g_list_segments.fetch_add(1, std::memory_order_relaxed);
            }
            const uint8_t ks = r.copy ? (uint8_t)0 : (uint8_t)~state;
            if (l->upload) r.dev[into] = h[j] ^ ks;
            else h[j] = r.dev[into] ^ ks;
            state = lcg::mulmod(state, lcg::A);
        }
        std::atomic_ref<uint32_t>(a.done[c]).store(1u, std::memory_order_release);
    }
    if (gave_up) {
        g_list_gave_up.fetch_add(1);
        std::atomic_ref<uint32_t>(a.work[1]).fetch_add(1u);
    }
    g_list_launches[l->upload ? 1 : 0].fetch_add(1);
    delete l;
}
} // namespace

hipError_t modgpu_launch_cycle_xfer_list(const CycleXferArgs &a, bool upload, uint32_t, hipStream_t stream)
{
    if (a.list == nullptr || a.list_n == 0 || a.ready == nullptr) return hipErrorInvalidValue;
    shim::enqueue(stream, run_list, new ListLaunch{a, upload});
    return hipSuccess;
}

extern "C" {
unsigned long long modgpu_shim_xfer_list_launches(int upload) { return g_list_launches[upload ? 1 : 0].load(); }
unsigned long long modgpu_shim_xfer_list_gave_up(void) { return g_list_gave_up.load(); }
unsigned long long modgpu_shim_xfer_list_plan_errors(void) { return g_list_plan_errors.load(); }
unsigned long long modgpu_shim_xfer_list_segments(void) { return g_list_segments.load(); }
void modgpu_shim_wedge_next_xfer_list(int on) { g_wedge_next.store(on ? 1 : 0); }
void modgpu_shim_release_wedged_xfer_list(void) { g_wedge_release.store(true, std::memory_order_release); }
}
