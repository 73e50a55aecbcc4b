// standin_launch_to_digest.cpp -- the digest launch of the out-of-place kernels (cycle_to_kernel.h: modgpu_launch_cycle_to_digest) on
// the CPU stand-in (hip/hip_runtime.h).  Like standin_launch_to.cpp: a launch is queued on the stream's thread and does, from the launch
// PLAN alone (CycleToArgs: each entry's body in the destination's role, the source byte paired with it, lead, edges, the three base
// states, the store mask and the record pointers), what the kernel would do -- byte by byte with lcg.h.  It reads every source byte,
// writes a destination only where the store mask says so, and ADDS onto the records (the host zeroed them in stream order), so the
// sanitizer runs see every byte the plan says the kernel touches.  No ticket pair: the plan must not carry one.
#include "../../modulate_amd/csrc/cycle_to_kernel.h"
#include "standin_entry.h"

namespace {
namespace E = standin_entry;
std::atomic<unsigned long long> g_digest_launches[2] = {}, g_digest_plan_errors{0}, g_digest_stored{0};

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

void run_digest(CycleToArgs &b, int form)
{
    const bool identity = (b.digest & CYCLE_TO_DIGEST_IDENTITY) != 0;
    if (!(b.digest & CYCLE_TO_DIGEST_ON) || b.queue || b.queue_done || b.n_parts < 1 || b.n_parts > (uint32_t)kCycleBatchMax || (b.store_mask >> b.n_parts) != 0)
        g_digest_plan_errors.fetch_add(1);
    g_digest_plan_errors.fetch_add(E::for_parts(b, [](const CycleToPart &P) { return P.dst_body; }, [&](uint32_t p, const CycleToPart &P, const E::Geom &g) {
        const bool store = ((b.store_mask >> p) & 1u) != 0;
        const unsigned bad = !b.result[p] || (E::at(b.result[p]) & 7) != 0 || (!store && P.dst_body != P.src_body);
        uint64_t s1 = 0, s2 = 0;
        E::for_spans(P, !identity, [&](int64_t at, uint64_t n, uint64_t j0, E::States st) { span_digest(store ? P.dst_body + at : nullptr, P.src_body + at, n, st.s[0], identity, j0, s1, s2); });
        if (store) g_digest_stored.fetch_add(1);
        std::atomic_ref<unsigned long long>(b.result[p]->s1).fetch_add(s1 % kDigestMod);
        std::atomic_ref<unsigned long long>(b.result[p]->s2).fetch_add(s2);
        std::atomic_ref<unsigned long long>(b.result[p]->n).fetch_add(P.head_n + g.body_bytes + P.tail_n);
        return bad;
    }));
    g_digest_launches[form == CYCLE_TO_FUNNEL ? 1 : 0].fetch_add(1);
}
} // namespace

hipError_t modgpu_launch_cycle_to_digest(const CycleToArgs &a, int form, uint32_t, hipStream_t stream)
{
    CycleToArgs on = a;
    on.digest |= CYCLE_TO_DIGEST_ON;
    return E::enqueue<CycleToArgs, run_digest>(on, form, stream);
}

extern "C" unsigned long long modgpu_shim_digest_launches(int form) { return form == 0 || form == 1 ? g_digest_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_digest_stored(void) { return g_digest_stored.load(); }
extern "C" unsigned long long modgpu_shim_digest_plan_errors(void) { return g_digest_plan_errors.load(); }
