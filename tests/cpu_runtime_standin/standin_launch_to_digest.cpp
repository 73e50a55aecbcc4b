// standin_launch_to_digest.cpp -- the digest launch of the out-of-place kernels (cycle_to_kernel.h: modgpu_launch_cycle_to_digest) on
// the CPU stand-in (hip/hip_runtime.h).  Like standin_launch_to.cpp: a launch is queued on the stream's thread and does, from the launch
// PLAN alone (CycleToArgs: each entry's body in the destination's role, the source byte paired with it, lead, edges, the three base
// states, the store mask and the record pointers), what the kernel would do -- byte by byte with lcg.h.  It reads every source byte,
// writes a destination only where the store mask says so, and ADDS onto the records (the host zeroed them in stream order), so the
// sanitizer runs see every byte the plan says the kernel touches.  No ticket pair: the plan must not carry one.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../modulate_amd/csrc/cycle_to_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_digest_launches[2] = {}, g_digest_plan_errors{0}, g_digest_stored{0};

struct DigestLaunch {
    CycleToArgs a;
    int form;
};

// out[i] = src[i] ^ keystream (state = canonical state of src[0]; identity: out = src), stored if `dst`, summed with byte i weighing j0 + i
void span_digest(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t state, bool identity, uint64_t j0, uint64_t &s1, uint64_t &s2)
{
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t out = identity ? src[i] : (uint8_t)(src[i] ^ (uint8_t)~state);
        if (!identity) state = lcg::mulmod(state, lcg::A);
        if (dst) dst[i] = out;
        s1 += out;
        s2 = (s2 + ((j0 + i) % kDigestMod) * out) % kDigestMod;
    }
}

void run_digest(void *arg)
{
    DigestLaunch *l = static_cast<DigestLaunch *>(arg);
    const CycleToArgs &b = l->a;
    const uint64_t chunk = modgpu_to_chunk_bytes();
    const bool identity = (b.digest & CYCLE_TO_DIGEST_IDENTITY) != 0;
    if (!(b.digest & CYCLE_TO_DIGEST_ON) || b.queue || b.queue_done || b.n_parts < 1 || b.n_parts > (uint32_t)kCycleBatchMax || (b.store_mask >> b.n_parts) != 0)
        g_digest_plan_errors.fetch_add(1);
    uint64_t total = 0;
    for (uint32_t p = 0; p < b.n_parts; ++p) {
        const CycleToPart &P = b.part[p];
        const bool store = ((b.store_mask >> p) & 1u) != 0;
        const uint64_t body_bytes = P.end - P.lead, n_chunks = (P.end + chunk - 1) / chunk, first = P.lead != 0 ? 1 : 0;
        if (b.start[p] != total || (reinterpret_cast<uintptr_t>(P.dst_body) & (chunk - 1)) != P.lead || (body_bytes != 0 && (reinterpret_cast<uintptr_t>(P.dst_body) & 15) != 0) || // (an entry that ends before its first aligned byte has no body)
            !b.result[p] || (reinterpret_cast<uintptr_t>(b.result[p]) & 7) != 0 || (!store && P.dst_body != P.src_body))
            g_digest_plan_errors.fetch_add(1);
        total += n_chunks > first ? n_chunks - first : 0;
        uint64_t s1 = 0, s2 = 0;
        uint8_t *const d = store ? P.dst_body : nullptr;
        span_digest(d ? d - P.head_n : nullptr, P.src_body - P.head_n, P.head_n, P.base_head, identity, 0, s1, s2);
        span_digest(d, P.src_body, body_bytes, identity ? 0u : lcg::mulmod(P.base_body, lcg::powmod(lcg::A, P.lead)), identity, P.head_n, s1, s2);
        span_digest(d ? d + body_bytes : nullptr, P.src_body + body_bytes, P.tail_n, P.base_tail, identity, P.head_n + body_bytes, s1, s2);
        if (store) g_digest_stored.fetch_add(1);
        std::atomic_ref<unsigned long long>(b.result[p]->s1).fetch_add(s1 % kDigestMod);
        std::atomic_ref<unsigned long long>(b.result[p]->s2).fetch_add(s2);
        std::atomic_ref<unsigned long long>(b.result[p]->n).fetch_add(P.head_n + body_bytes + P.tail_n);
    }
    for (uint32_t p = b.n_parts; p <= (uint32_t)kCycleBatchMax; ++p)
        if (b.start[p] != total) g_digest_plan_errors.fetch_add(1);
    g_digest_launches[l->form == CYCLE_TO_FUNNEL ? 1 : 0].fetch_add(1);
    delete l;
}
} // namespace

hipError_t modgpu_launch_cycle_to_digest(const CycleToArgs &a, int form, uint32_t, hipStream_t stream)
{
    DigestLaunch *l = new DigestLaunch{a, form};
    l->a.digest |= CYCLE_TO_DIGEST_ON;
    shim::enqueue(stream, run_digest, l);
    return hipSuccess;
}

extern "C" unsigned long long modgpu_shim_digest_launches(int form) { return form == 0 || form == 1 ? g_digest_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_digest_stored(void) { return g_digest_stored.load(); }
extern "C" unsigned long long modgpu_shim_digest_plan_errors(void) { return g_digest_plan_errors.load(); }
