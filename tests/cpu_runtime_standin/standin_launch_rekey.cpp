// standin_launch_rekey.cpp -- the rekey launch (cycle_rekey_kernel.h) on the CPU stand-in (hip/hip_runtime.h).  Like
// standin_launch_to.cpp: a launch is queued on the stream's thread and does, from the launch PLAN alone (CycleRekeyArgs: each entry's
// destination body, the source byte paired with it, lead, edges and the two sets of base states), what the kernel would do -- byte by
// byte with lcg.h, both keystreams.  It reads the source and writes the destination, so the sanitizer runs see every byte the plan says
// the kernel touches.  The ticket pair is emulated as for the work-queue shape: taken at the start of the launch, cleaned and signed
// off at its end; a launch that finds its pair taken counts a collision.
#include "../../modulate_amd/csrc/cycle_rekey_kernel.h"
#include "standin_entry.h"

namespace {
namespace E = standin_entry;
std::atomic<unsigned long long> g_rekey_launches[2] = {}, g_rekey_collisions{0}, g_rekey_plan_errors{0};

// sa, sb = canonical states of src[0] / dst[0] under the two keystreams
void span_rekey(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t sa, uint32_t sb)
{
    for (uint64_t i = 0; i < n; ++i) {
        dst[i] = src[i] ^ (uint8_t)~sa ^ (uint8_t)~sb;
        sa = lcg::mulmod(sa, lcg::A);
        sb = lcg::mulmod(sb, lcg::A);
    }
}

void run_rekey(CycleRekeyArgs &b, int form)
{
    if (!E::take_pair(b)) g_rekey_collisions.fetch_add(1);
    E::last_a_while();
    g_rekey_plan_errors.fetch_add(E::for_parts(b, [](const CycleRekeyPart &P) { return P.dst_body; }, [](uint32_t, const CycleRekeyPart &P, const E::Geom &) {
        E::for_spans(P, true, [&](int64_t at, uint64_t n, uint64_t, E::States st) { span_rekey(P.dst_body + at, P.src_body + at, n, st.s[0], st.s[1]); });
        return 0u;
    }));
    E::sign_off_pair(b);
    g_rekey_launches[form == CYCLE_REKEY_FUNNEL ? 1 : 0].fetch_add(1);
}
} // namespace

uint32_t modgpu_rekey_chunk_bytes() { return 65536u; }
uint32_t modgpu_rekey_block() { return 1024u; }
const char *modgpu_rekey_kernel_name(int form) { return form == CYCLE_REKEY_FUNNEL ? "shim rekey funnel" : "shim rekey"; }
hipError_t modgpu_launch_cycle_rekey(const CycleRekeyArgs &a, int form, uint32_t, hipStream_t stream) { return E::enqueue<CycleRekeyArgs, run_rekey>(a, form, stream); }

extern "C" unsigned long long modgpu_shim_rekey_launches(int form) { return form == 0 || form == 1 ? g_rekey_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_rekey_collisions(void) { return g_rekey_collisions.load(); }
extern "C" unsigned long long modgpu_shim_rekey_plan_errors(void) { return g_rekey_plan_errors.load(); }
