// standin_launch_rekey_verify.cpp -- the rekey verify launch (cycle_rekey_verify_kernel.h) on the CPU stand-in (hip/hip_runtime.h).
// Like standin_launch_verify.cpp: a launch is queued on the stream's thread and does, from the launch PLAN alone
// (CycleRekeyVerifyArgs: each entry's expect body, the source byte paired with it, lead, edges, the two sets of base states and the
// result), what the kernel would do -- byte by byte with lcg.h, both keystreams.  It READS both sides where the plan says the kernel
// reads them and writes only the result, adding the count and taking the minimum of the position as the kernel's atomics do, so the
// host planning (edges, cut chunk, the routing of degenerate keystreams, batch splitting, the order of the initialising launch and the
// compare launches) is checked on the CPU, and the sanitizer runs see every byte the plan touches.  The initialising launch is
// standin_launch_verify.cpp's.
#include "../../modulate_amd/csrc/cycle_rekey_verify_kernel.h"
#include "standin_entry.h"

namespace {
namespace E = standin_entry;
std::atomic<unsigned long long> g_rekey_verify_launches[2] = {}, g_rekey_verify_plan_errors{0};

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

void run_rekey_verify(CycleRekeyVerifyArgs &b, int form)
{
    E::last_a_while();
    g_rekey_verify_plan_errors.fetch_add(E::for_parts(b, [](const CycleRekeyVerifyPart &P) { return P.expect_body; }, [&](uint32_t, const CycleRekeyVerifyPart &P, const E::Geom &g) {
        unsigned bad = P.head_n + g.body_bytes + P.tail_n != P.n || g.n_chunks >= (1u << 24);
        bad += E::needs_funnel(P.expect_body, P.src_body, g.body_bytes) && form != CYCLE_REKEY_VERIFY_FUNNEL;
        unsigned long long count = 0, lowest = kVerifyNone;
        E::for_spans(P, true, [&](int64_t at, uint64_t n, uint64_t j0, E::States st) { span_rekey_verify(P.expect_body + at, P.src_body + at, n, st.s[0], st.s[1], j0, count, lowest); });
        // as the kernel: n stored, count added, position folded in with a minimum -- on a result the init launch has made clean
        bad += P.result->mismatches != 0 || P.result->first_mismatch != kVerifyNone || P.result->reserved != 0;
        P.result->n = P.n;
        P.result->mismatches += count;
        if (lowest < P.result->first_mismatch) P.result->first_mismatch = lowest;
        return bad;
    }));
    g_rekey_verify_launches[form == CYCLE_REKEY_VERIFY_FUNNEL ? 1 : 0].fetch_add(1);
}
} // namespace

uint32_t modgpu_rekey_verify_chunk_bytes() { return 65536u; }
uint32_t modgpu_rekey_verify_block() { return 1024u; }
const char *modgpu_rekey_verify_kernel_name(int form) { return form == CYCLE_REKEY_VERIFY_FUNNEL ? "shim rekey verify funnel" : "shim rekey verify"; }
hipError_t modgpu_launch_cycle_rekey_verify(const CycleRekeyVerifyArgs &a, int form, uint32_t, hipStream_t stream)
{
    return E::enqueue<CycleRekeyVerifyArgs, run_rekey_verify>(a, form, stream);
}

extern "C" unsigned long long modgpu_shim_rekey_verify_launches(int form) { return form == 0 || form == 1 ? g_rekey_verify_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_rekey_verify_plan_errors(void) { return g_rekey_verify_plan_errors.load(); }
