// standin_launch_to.cpp -- the out-of-place launch (cycle_to_kernel.h) on the CPU stand-in (hip/hip_runtime.h).  Like standin_launch.cpp:
// a launch is queued on the stream's thread and does, from the launch PLAN alone (CycleToArgs: each entry's destination body, the
// source byte paired with it, lead, edges and the three base states), what the kernel would do -- byte by byte with lcg.h.  It reads
// the source and writes the destination, so the sanitizer runs see every byte the plan says the kernel touches.  The ticket pair is
// emulated as for the work-queue shape: taken at the start of the launch, cleaned and signed off at its end; a launch that finds its
// pair taken counts a collision.
#include "../../modulate_amd/csrc/cycle_to_kernel.h"
#include "standin_entry.h"

namespace {
namespace E = standin_entry;
std::atomic<unsigned long long> g_to_launches[2] = {}, g_to_collisions{0}, g_to_plan_errors{0};

void span_to(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t state) // state = canonical state of src[0] / dst[0]
{
    for (uint64_t i = 0; i < n; ++i) {
        dst[i] = src[i] ^ (uint8_t)~state;
        state = lcg::mulmod(state, lcg::A);
    }
}

void run_to(CycleToArgs &b, int form)
{
    if (!E::take_pair(b)) g_to_collisions.fetch_add(1);
    E::last_a_while();
    g_to_plan_errors.fetch_add(E::for_parts(b, [](const CycleToPart &P) { return P.dst_body; }, [](uint32_t, const CycleToPart &P, const E::Geom &) {
        E::for_spans(P, true, [&](int64_t at, uint64_t n, uint64_t, E::States st) { span_to(P.dst_body + at, P.src_body + at, n, st.s[0]); });
        return 0u;
    }));
    E::sign_off_pair(b);
    g_to_launches[form == CYCLE_TO_FUNNEL ? 1 : 0].fetch_add(1);
}
} // namespace

uint32_t modgpu_to_chunk_bytes() { return 65536u; }
uint32_t modgpu_to_block() { return 1024u; }
const char *modgpu_to_kernel_name(int form) { return form == CYCLE_TO_FUNNEL ? "shim to funnel" : "shim to"; }
hipError_t modgpu_launch_cycle_to(const CycleToArgs &a, int form, uint32_t, hipStream_t stream) { return E::enqueue<CycleToArgs, run_to>(a, form, stream); }

extern "C" unsigned long long modgpu_shim_to_launches(int form) { return form == 0 || form == 1 ? g_to_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_to_collisions(void) { return g_to_collisions.load(); }
extern "C" unsigned long long modgpu_shim_to_plan_errors(void) { return g_to_plan_errors.load(); }
