// standin_launch_rekey_verify.cpp -- the rekey verify launch (cycle_rekey_verify_kernel.h) on the CPU stand-in (hip/hip_runtime.h).
// Like standin_launch_verify.cpp: a launch is queued on the stream's thread and does, from the launch PLAN alone
// (CycleRekeyVerifyArgs: each entry's expect body, the source byte paired with it, lead, edges, the two sets of base states and the
// result), what the kernel would do -- byte by byte with lcg.h, both keystreams.  It READS both sides where the plan says the kernel
// reads them and writes only the result, adding the count and taking the minimum of the position as the kernel's atomics do, so the
// host planning (edges, cut chunk, the routing of degenerate keystreams, batch splitting, the order of the initialising launch and the
// compare launches) is checked on the CPU, and the sanitizer runs see every byte the plan touches.  The initialising launch is
// standin_launch_verify.cpp's.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_rekey_verify_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_rekey_verify_launches[2] = {}, g_rekey_verify_plan_errors{0};

struct RekeyVerifyLaunch {
    CycleRekeyVerifyArgs a;
    int form;
};

// sa, sb = canonical states of src[0] under the two keystreams; j0 = index in the entry of src[0]
void span_rekey_verify(const uint8_t *expect, const uint8_t *src, uint64_t n, uint32_t sa, uint32_t sb, uint64_t j0, unsigned long long &count,
                       unsigned long long &first)
{
    for (uint64_t i = 0; i < n; ++i) {
        if (expect[i] != (uint8_t)(src[i] ^ (uint8_t)~sa ^ (uint8_t)~sb)) {
            ++count;
            if (j0 + i < first) first = j0 + i;
        }
        sa = lcg::mulmod(sa, lcg::A);
        sb = lcg::mulmod(sb, lcg::A);
    }
}

void run_rekey_verify(void *arg)
{
    RekeyVerifyLaunch *l = static_cast<RekeyVerifyLaunch *>(arg);
    const CycleRekeyVerifyArgs &b = l->a;
    std::this_thread::sleep_for(std::chrono::microseconds(200)); // a launch lasts a while: overlaps become likely
    const uint64_t chunk = modgpu_rekey_verify_chunk_bytes();
    uint64_t total = 0;
    for (uint32_t p = 0; p < b.n_parts; ++p) {
        const CycleRekeyVerifyPart &P = b.part[p];
        const uint64_t body_bytes = P.end - P.lead, n_chunks = (P.end + chunk - 1) / chunk, first = P.lead != 0 ? 1 : 0;
        // (an entry shorter than its head has an empty body wherever the head ends)
        if (b.start[p] != total || (reinterpret_cast<uintptr_t>(P.expect_body) & (chunk - 1)) != P.lead ||
            (body_bytes && (reinterpret_cast<uintptr_t>(P.expect_body) & 15) != 0) || P.head_n + body_bytes + P.tail_n != P.n || n_chunks >= (1u << 24))
            g_rekey_verify_plan_errors.fetch_add(1);
        const bool funnel = body_bytes && ((reinterpret_cast<uintptr_t>(P.src_body) - reinterpret_cast<uintptr_t>(P.expect_body)) & 3) != 0;
        if (funnel && l->form != CYCLE_REKEY_VERIFY_FUNNEL) g_rekey_verify_plan_errors.fetch_add(1); // the plain form reads whole dwords
        total += n_chunks > first ? n_chunks - first : 0;
        const uint32_t fwd = lcg::powmod(lcg::A, P.lead);
        unsigned long long count = 0, lowest = kVerifyNone;
        span_rekey_verify(P.expect_body - P.head_n, P.src_body - P.head_n, P.head_n, P.base_head[0], P.base_head[1], 0, count, lowest);
        span_rekey_verify(P.expect_body, P.src_body, body_bytes, lcg::mulmod(P.base_body[0], fwd), lcg::mulmod(P.base_body[1], fwd), P.head_n, count, lowest);
        span_rekey_verify(P.expect_body + body_bytes, P.src_body + body_bytes, P.tail_n, P.base_tail[0], P.base_tail[1], P.head_n + body_bytes, count, lowest);
        // as the kernel: n stored, count added, position folded in with a minimum -- on a result the init launch has made clean
        if (P.result->mismatches != 0 || P.result->first_mismatch != kVerifyNone || P.result->reserved != 0) g_rekey_verify_plan_errors.fetch_add(1);
        P.result->n = P.n;
        P.result->mismatches += count;
        if (lowest < P.result->first_mismatch) P.result->first_mismatch = lowest;
    }
    for (uint32_t p = b.n_parts; p <= (uint32_t)kCycleBatchMax; ++p)
        if (b.start[p] != total) g_rekey_verify_plan_errors.fetch_add(1);
    g_rekey_verify_launches[l->form == CYCLE_REKEY_VERIFY_FUNNEL ? 1 : 0].fetch_add(1);
    delete l;
}
} // namespace

uint32_t modgpu_rekey_verify_chunk_bytes() { return 65536u; }
uint32_t modgpu_rekey_verify_block() { return 1024u; }
const char *modgpu_rekey_verify_kernel_name(int form) { return form == CYCLE_REKEY_VERIFY_FUNNEL ? "shim rekey verify funnel" : "shim rekey verify"; }
hipError_t modgpu_launch_cycle_rekey_verify(const CycleRekeyVerifyArgs &a, int form, uint32_t, hipStream_t stream)
{
    shim::enqueue(stream, run_rekey_verify, new RekeyVerifyLaunch{a, form});
    return hipSuccess;
}

extern "C" unsigned long long modgpu_shim_rekey_verify_launches(int form) { return form == 0 || form == 1 ? g_rekey_verify_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_rekey_verify_plan_errors(void) { return g_rekey_verify_plan_errors.load(); }
