// standin_launch_xfer.cpp -- the transfer kernels (cycle_xfer_kernel.h) on the CPU stand-in (hip/hip_runtime.h).  Like the host-fed
// stand-in in standin_launch.cpp: a launch is queued on the stream's thread and runs WHILE the library's pipelines fill and drain their
// slots -- chunk after chunk it waits for `ready` (or `abort`, or its patience), moves the chunk between its slot (or the caller's
// page-locked pages) and the device buffer with the product's own arithmetic (lcg.h), byte by byte, and marks it `done`.  So the
// sanitizer runs see every byte the launch arguments say the kernel reads and writes.
//
// "Device memory" here is what modgpu_shim_xfer_alloc handed out: modgpu_xfer_device_of knows those ranges and nothing else, so a host
// pointer passed as the device side is refused as the real runtime would refuse it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include "../../modulate_amd/csrc/cycle_xfer_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_xfer_launches[2] = {}, g_xfer_gave_up{0};
// modgpu_shim_wedge_next_xfer(1): the next staged transfer "kernel" stops responding half-way -- it neither finishes its chunks nor
// ends, whatever the abort word says -- until modgpu_shim_release_wedged_xfer() lets the stream's thread go.
std::atomic<int> g_wedge_next{0};
std::atomic<bool> g_wedge_release{false};

struct XferLaunch {
    CycleXferArgs a;
    bool upload;
};

void move(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t state, bool copy) // state = canonical state of src[0] / dst[0]
{
    if (copy) {
        std::memmove(dst, src, n);
        return;
    }
    for (uint64_t i = 0; i < n; ++i) {
        dst[i] = src[i] ^ (uint8_t)~state;
        state = lcg::mulmod(state, lcg::A);
    }
}

void run_xfer(void *arg)
{
    XferLaunch *l = static_cast<XferLaunch *>(arg);
    const CycleXferArgs &a = l->a;
    const bool staged = a.ready != nullptr;
    const uint64_t chunk = staged ? a.chunk_bytes : a.n;
    const uint64_t chunks = (a.n + chunk - 1) / chunk;
    const bool wedge = staged && g_wedge_next.exchange(0) != 0;
    bool gave_up = false;
    for (uint64_t c = 0; c < chunks && !gave_up; ++c) {
        if (wedge && c == chunks / 2) {
            while (!g_wedge_release.load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            delete l; // (nothing of the call is touched any more: the library has long abandoned it)
            return;
        }
        if (staged) {
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
        }
        const uint64_t pos = c * chunk, len = std::min<uint64_t>(chunk, a.n - pos);
        uint8_t *h = staged ? a.slot[(c % a.pipes) * 2 + (c / a.pipes) % 2] + a.slot_phase : a.host + pos;
        uint8_t *d = a.dev + pos;
        const uint32_t st = lcg::mulmod(a.base, lcg::powmod(lcg::A, pos % lcg::PERIOD));
        if (l->upload) move(d, h, len, st, a.copy != 0);
        else move(h, d, len, st, a.copy != 0);
        if (staged) std::atomic_ref<uint32_t>(a.done[c]).store(1u, std::memory_order_release);
    }
    if (gave_up) {
        g_xfer_gave_up.fetch_add(1);
        std::atomic_ref<uint32_t>(a.work[1]).fetch_add(1u);
    }
    g_xfer_launches[l->upload ? 1 : 0].fetch_add(1);
    delete l;
}

std::mutex g_alloc_mu;
std::map<uintptr_t, std::pair<uint64_t, int>> g_allocs; // start -> (bytes, device)
} // namespace

uint32_t modgpu_xfer_block() { return 256u; }
const char *modgpu_xfer_kernel_name(bool upload, int form)
{
    return upload ? (form == XFER_FUNNEL ? "shim xfer up funnel" : "shim xfer up") : (form == XFER_FUNNEL ? "shim xfer down funnel" : "shim xfer down");
}
// modgpu_shim_fail_next_xfer_launch(1): the next transfer launch is refused by the "runtime" -- nothing is queued
static std::atomic<int> g_fail_next_xfer_launch{0};
extern "C" void modgpu_shim_fail_next_xfer_launch(int on) { g_fail_next_xfer_launch.store(on ? 1 : 0); }
hipError_t modgpu_launch_cycle_xfer(const CycleXferArgs &a, bool upload, int, uint32_t, hipStream_t stream)
{
    if (g_fail_next_xfer_launch.exchange(0) != 0) return hipErrorLaunchFailure;
    shim::enqueue(stream, run_xfer, new XferLaunch{a, upload});
    return hipSuccess;
}
int modgpu_xfer_device_of(const void *p, uint64_t n)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lock(g_alloc_mu);
    auto it = g_allocs.upper_bound(x);
    if (it == g_allocs.begin()) return -1;
    --it;
    return x - it->first + n <= it->second.first ? it->second.second : -1;
}

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device)
{
    void *p = std::malloc(n ? n : 1);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lock(g_alloc_mu);
    g_allocs[reinterpret_cast<uintptr_t>(p)] = {n, device};
    return p;
}
void modgpu_shim_xfer_free(void *p)
{
    {
        std::lock_guard<std::mutex> lock(g_alloc_mu);
        g_allocs.erase(reinterpret_cast<uintptr_t>(p));
    }
    std::free(p);
}
unsigned long long modgpu_shim_xfer_launches(int upload) { return g_xfer_launches[upload ? 1 : 0].load(); }
unsigned long long modgpu_shim_xfer_gave_up(void) { return g_xfer_gave_up.load(); }
void modgpu_shim_wedge_next_xfer(int on) { g_wedge_next.store(on ? 1 : 0); }
void modgpu_shim_release_wedged_xfer(void) { g_wedge_release.store(true, std::memory_order_release); }
}
