// standin_launch_keep.cpp -- the keep launch (cycle_keep_kernel.h: the work-queue launch with a cache policy per chunk) on the CPU
// stand-in (hip/hip_runtime.h).  A cache policy changes no byte, so the launch is the work-queue shape's own stand-in run over the
// CycleQueueArgs part of the arguments (standin_launch.cpp: part by part from the plan alone, the ticket pair emulated); what is
// checked here is the policy itself -- a mask that is a power of two minus one, a run no longer than the period.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../modulate_amd/csrc/cycle_keep_kernel.h"

namespace {
std::atomic<unsigned long long> g_keep_launches{0}, g_keep_kept{0}, g_keep_plan_errors{0};
}

uint32_t modgpu_keep_chunk_bytes() { return 65536u; }
uint32_t modgpu_keep_block() { return 1024u; }
const char *modgpu_keep_kernel_name() { return "shim keep"; }
hipError_t modgpu_launch_cycle_keep(const CycleKeepArgs &a, uint32_t grid, hipStream_t stream)
{
    if ((a.keep_mask & (a.keep_mask + 1u)) != 0u || (uint64_t)a.keep_run > (uint64_t)a.keep_mask + 1u || a.n_parts != 1u) g_keep_plan_errors.fetch_add(1);
    g_keep_launches.fetch_add(1);
    if (a.keep_run) g_keep_kept.fetch_add(1);
    return modgpu_launch_cycle_queue(static_cast<const CycleQueueArgs &>(a), grid, stream);
}

extern "C" unsigned long long modgpu_shim_keep_launches(void) { return g_keep_launches.load(); }
extern "C" unsigned long long modgpu_shim_keep_kept(void) { return g_keep_kept.load(); }
extern "C" unsigned long long modgpu_shim_keep_plan_errors(void) { return g_keep_plan_errors.load(); }
