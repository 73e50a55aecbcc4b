// standin_launch_verify.cpp -- the verify launches (cycle_verify_kernel.h) on the CPU stand-in (hip/hip_runtime.h).  Like
// standin_launch_rekey.cpp: a launch is queued on the stream's thread and does, from the launch PLAN alone (CycleVerifyArgs: each
// entry's expect body, the source byte paired with it, lead, edges, base states and result), what the kernels would do -- byte by byte
// with lcg.h.  It READS both sides where the plan says the kernel reads them and writes only the result, adding the count and taking
// the minimum of the position as the kernel's atomics do, so the host planning (edges, cut chunk, batch splitting, the order of the
// initialising launch and the compare launches) is checked on the CPU, and the sanitizer runs see every byte the plan touches.
#include "../../modulate_amd/csrc/cycle_verify_kernel.h"
#include "standin_entry.h"

namespace {
namespace E = standin_entry;
std::atomic<unsigned long long> g_verify_launches[4] = {}, g_verify_inits{0}, g_verify_plan_errors{0};

struct VerifyInit {
    CycleVerifyResult *results;
    uint64_t count;
};

// s = canonical state of src[0] (ignored by the identity forms); j0 = index in the entry of src[0]
void span_verify(const uint8_t *expect, const uint8_t *src, uint64_t n, uint32_t s, bool keyed, uint64_t j0, unsigned long long &count,
                 unsigned long long &first)
{
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t want = keyed ? (uint8_t)(src[i] ^ (uint8_t)~s) : src[i];
        if (expect[i] != want) {
            ++count;
            if (j0 + i < first) first = j0 + i;
        }
        if (keyed) s = lcg::mulmod(s, lcg::A);
    }
}

void run_verify_init(void *arg)
{
    VerifyInit *l = static_cast<VerifyInit *>(arg);
    for (uint64_t i = 0; i < l->count; ++i) l->results[i] = CycleVerifyResult{0ull, kVerifyNone, 0ull, 0ull};
    g_verify_inits.fetch_add(1);
    delete l;
}

void run_verify(CycleVerifyArgs &b, int form)
{
    const bool keyed = !(form & CYCLE_VERIFY_IDENTITY);
    E::last_a_while();
    g_verify_plan_errors.fetch_add(E::for_parts(b, [](const CycleVerifyPart &P) { return P.expect_body; }, [&](uint32_t, const CycleVerifyPart &P, const E::Geom &g) {
        unsigned bad = P.head_n + g.body_bytes + P.tail_n != P.n || g.n_chunks >= (1u << 24);
        bad += E::needs_funnel(P.expect_body, P.src_body, g.body_bytes) && !(form & CYCLE_VERIFY_FUNNEL);
        unsigned long long count = 0, lowest = kVerifyNone;
        E::for_spans(P, keyed, [&](int64_t at, uint64_t n, uint64_t j0, E::States st) { span_verify(P.expect_body + at, P.src_body + at, n, st.s[0], keyed, j0, count, lowest); });
        // as the kernel: n stored, count added, position folded in with a minimum -- on a result the init launch has made clean
        bad += P.result->mismatches != 0 || P.result->first_mismatch != kVerifyNone || P.result->reserved != 0;
        P.result->n = P.n;
        P.result->mismatches += count;
        if (lowest < P.result->first_mismatch) P.result->first_mismatch = lowest;
        return bad;
    }));
    g_verify_launches[form & 3].fetch_add(1);
}
} // namespace

uint32_t modgpu_verify_chunk_bytes() { return 65536u; }
uint32_t modgpu_verify_block() { return 1024u; }
const char *modgpu_verify_kernel_name(int form)
{
    static const char *const names[4] = {"shim verify", "shim verify funnel", "shim verify identity", "shim verify identity funnel"};
    return names[form & 3];
}
hipError_t modgpu_launch_verify_init(CycleVerifyResult *results, uint64_t count, hipStream_t stream)
{
    shim::enqueue(stream, run_verify_init, new VerifyInit{results, count});
    return hipSuccess;
}
hipError_t modgpu_launch_cycle_verify(const CycleVerifyArgs &a, int form, uint32_t, hipStream_t stream) { return E::enqueue<CycleVerifyArgs, run_verify>(a, form, stream); }

extern "C" unsigned long long modgpu_shim_verify_launches(int form) { return form >= 0 && form < 4 ? g_verify_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_verify_inits(void) { return g_verify_inits.load(); }
extern "C" unsigned long long modgpu_shim_verify_plan_errors(void) { return g_verify_plan_errors.load(); }
