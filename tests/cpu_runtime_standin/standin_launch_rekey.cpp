// standin_launch_rekey.cpp -- the rekey launch (cycle_rekey_kernel.h) on the CPU stand-in (hip/hip_runtime.h).  Like
// standin_launch_to.cpp: a launch is queued on the stream's thread and does, from the launch PLAN alone (CycleRekeyArgs: each entry's
// destination body, the source byte paired with it, lead, edges and the two sets of base states), what the kernel would do -- byte by
// byte with lcg.h, both keystreams.  It reads the source and writes the destination, so the sanitizer runs see every byte the plan says
// the kernel touches.  The ticket pair is emulated as for the work-queue shape: taken at the start of the launch, cleaned and signed
// off at its end; a launch that finds its pair taken counts a collision.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_rekey_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_rekey_launches[2] = {}, g_rekey_collisions{0}, g_rekey_plan_errors{0};

struct RekeyLaunch {
    CycleRekeyArgs a;
    int form;
};

// sa, sb = canonical states of src[0] / dst[0] under the two keystreams
void span_rekey(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t sa, uint32_t sb)
{
    for (uint64_t i = 0; i < n; ++i) {
        dst[i] = src[i] ^ (uint8_t)~sa ^ (uint8_t)~sb;
        sa = lcg::mulmod(sa, lcg::A);
        sb = lcg::mulmod(sb, lcg::A);
    }
}

void run_rekey(void *arg)
{
    RekeyLaunch *l = static_cast<RekeyLaunch *>(arg);
    CycleRekeyArgs &b = l->a;
    uint32_t expect = 0;
    if (!std::atomic_ref<uint32_t>(b.queue[0]).compare_exchange_strong(expect, 1u)) g_rekey_collisions.fetch_add(1);
    std::this_thread::sleep_for(std::chrono::microseconds(200)); // a launch lasts a while: overlaps become likely
    const uint64_t chunk = modgpu_rekey_chunk_bytes();
    uint64_t total = 0;
    for (uint32_t p = 0; p < b.n_parts; ++p) {
        const CycleRekeyPart &P = b.part[p];
        const uint64_t body_bytes = P.end - P.lead, n_chunks = (P.end + chunk - 1) / chunk, first = P.lead != 0 ? 1 : 0;
        // (an entry shorter than its head has an empty body wherever the head ends)
        if (b.start[p] != total || (reinterpret_cast<uintptr_t>(P.dst_body) & (chunk - 1)) != P.lead || (body_bytes && (reinterpret_cast<uintptr_t>(P.dst_body) & 15) != 0))
            g_rekey_plan_errors.fetch_add(1);
        total += n_chunks > first ? n_chunks - first : 0;
        const uint32_t fwd = lcg::powmod(lcg::A, P.lead);
        span_rekey(P.dst_body - P.head_n, P.src_body - P.head_n, P.head_n, P.base_head[0], P.base_head[1]);
        span_rekey(P.dst_body, P.src_body, body_bytes, lcg::mulmod(P.base_body[0], fwd), lcg::mulmod(P.base_body[1], fwd));
        span_rekey(P.dst_body + body_bytes, P.src_body + body_bytes, P.tail_n, P.base_tail[0], P.base_tail[1]);
    }
    for (uint32_t p = b.n_parts; p <= (uint32_t)kCycleBatchMax; ++p)
        if (b.start[p] != total) g_rekey_plan_errors.fetch_add(1);
    std::atomic_ref<uint32_t>(b.queue[0]).store(0u);
    if (b.queue_done) std::atomic_ref<uint32_t>(*b.queue_done).store(b.queue_seq, std::memory_order_release);
    g_rekey_launches[l->form == CYCLE_REKEY_FUNNEL ? 1 : 0].fetch_add(1);
    delete l;
}
} // namespace

uint32_t modgpu_rekey_chunk_bytes() { return 65536u; }
uint32_t modgpu_rekey_block() { return 1024u; }
const char *modgpu_rekey_kernel_name(int form) { return form == CYCLE_REKEY_FUNNEL ? "shim rekey funnel" : "shim rekey"; }
hipError_t modgpu_launch_cycle_rekey(const CycleRekeyArgs &a, int form, uint32_t, hipStream_t stream)
{
    shim::enqueue(stream, run_rekey, new RekeyLaunch{a, form});
    return hipSuccess;
}

extern "C" unsigned long long modgpu_shim_rekey_launches(int form) { return form == 0 || form == 1 ? g_rekey_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_rekey_collisions(void) { return g_rekey_collisions.load(); }
extern "C" unsigned long long modgpu_shim_rekey_plan_errors(void) { return g_rekey_plan_errors.load(); }
