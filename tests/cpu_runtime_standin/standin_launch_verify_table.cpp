// standin_launch_verify_table.cpp -- the verify table launches (cycle_verify_table_kernel.h) on the CPU stand-in (hip/hip_runtime.h).
// Each launch is queued on the stream's thread and does, from its arguments and the workspace alone, what the kernel would do -- byte
// by byte with lcg.h:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks and lays out every entry on the chunk grid of its comparand,
//           writes the plan and blk records, resets the header and the summary;
//   finish  globalises the starts, decides the status, and -- unless the call is refused, when it writes nothing more -- writes the
//           search levels (padded with ~0), compares the ragged edges and stores every entry's result whole;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent of the levels, compares
//           the chunk's span and adds to / lowers the entry's result and the summary as the kernel's atomics do.
// It READS both sides where the plan says the kernel reads them and writes only results and workspace, so the sanitizer runs see every
// byte of the workspace layout the host planned and every byte of the caller's buffers the kernels would touch.
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_verify_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_verify_table_launches[3] = {};

// k * a^e; 0 for the identity keystream: a plain compare
uint32_t base_state(uint32_t k, uint64_t e) { return k ? lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)) : 0u; }

void run_plan(VerifyTableArgs *a)
{
    a->sum->mismatches = 0;
    a->sum->first_bad_entry = kVerifyNone;
    a->sum->entries = a->n;
    a->sum->reserved = 0;
    plan(a, [&](uint64_t i, uint64_t run) {
        const CycleTableEntry E = a->entries[i];
        const Grid g = grid_of(E, E.flags);
        const uint32_t k = lcg::key_residue(E.key);
        const uint64_t o1 = E.stream_off % lcg::PERIOD + 1;
        CycleTablePlan &P = a->plan[i];
        plan_fields(P, E, g, run);
        P.base_head = base_state(k, o1);
        P.base = base_state(k, o1 + g.origin);
        P.base_tail = base_state(k, o1 + g.tail);
        return g;
    });
}

// bytes [at, at + len) of a span from its origins, s0 the origin byte's state (0: the identity keystream); j0 = index in the entry of
// the origin byte (modulo 2^64)
void span_verify(const uint8_t *exp0, const uint8_t *src0, uint64_t at, uint64_t len, uint32_t s0, uint64_t j0, unsigned long long &count,
                 unsigned long long &first)
{
    uint32_t s = s0 ? lcg::mulmod(s0, lcg::powmod(lcg::A, at % lcg::PERIOD)) : 0u;
    for (uint64_t j = 0; j < len; ++j) {
        const uint8_t want = s0 ? (uint8_t)(src0[at + j] ^ (uint8_t)~s) : src0[at + j];
        if (exp0[at + j] != want) {
            ++count;
            if (j0 + at + j < first) first = j0 + at + j;
        }
        if (s0) s = lcg::mulmod(s, lcg::A);
    }
}

void run_finish(VerifyTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t i, CycleTablePlan &P, bool ok) {
        if (!ok) return;
        const uint64_t body = P.end - P.lead;
        unsigned long long count = 0, first = kVerifyNone;
        span_verify(P.dst_origin + P.lead - P.head_n, P.src_origin + P.lead - P.head_n, 0, P.head_n, P.base_head, 0, count, first);
        span_verify(P.dst_origin + P.end, P.src_origin + P.end, 0, P.tail_n, P.base_tail, P.head_n + body, count, first);
        a->results[i] = CycleVerifyResult{count, first, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
        if (count) {
            a->sum->mismatches += count;
            if (i < a->sum->first_bad_entry) a->sum->first_bad_entry = i;
        }
    });
}

void run_stream(VerifyTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const CycleTablePlan &P = a->plan[s.entry];
        unsigned long long count = 0, first = kVerifyNone;
        span_verify(P.dst_origin, P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base, (uint64_t)P.head_n - P.lead, count, first);
        if (count) {
            a->results[s.entry].mismatches += count;
            if (first < a->results[s.entry].first_mismatch) a->results[s.entry].first_mismatch = first;
            a->sum->mismatches += count;
            if (s.entry < a->sum->first_bad_entry) a->sum->first_bad_entry = s.entry;
        }
    });
}
} // namespace

uint32_t modgpu_verify_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_verify_table_block() { return 1024u; }
const char *modgpu_verify_table_kernel_name() { return "shim verify table stream"; }
hipError_t modgpu_launch_verify_table_plan(const VerifyTableArgs &a, hipStream_t stream) { return enqueue<VerifyTableArgs, run_plan, g_verify_table_launches, 0>(a, stream); }
hipError_t modgpu_launch_verify_table_finish(const VerifyTableArgs &a, hipStream_t stream) { return enqueue<VerifyTableArgs, run_finish, g_verify_table_launches, 1>(a, stream); }
hipError_t modgpu_launch_verify_table_stream(const VerifyTableArgs &a, uint32_t, hipStream_t stream) { return enqueue<VerifyTableArgs, run_stream, g_verify_table_launches, 2>(a, stream); }

extern "C" unsigned long long modgpu_shim_verify_table_launches(int kind) { return count(g_verify_table_launches, kind); }
