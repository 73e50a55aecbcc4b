// standin_launch_rekey_verify_table.cpp -- the rekey verify table launches (cycle_rekey_verify_table_kernel.h) on the CPU stand-in
// (hip/hip_runtime.h).  Each launch is queued on the stream's thread and does, from its arguments and the workspace alone, what the
// kernel would do -- byte by byte with lcg.h, the identity keystream's state kept as 2^31-1 as the kernels keep it:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks and lays out every entry on the chunk grid of its comparand,
//           writes the plan, edge and blk records, resets the header and the summary;
//   finish  globalises the starts, decides the status, and -- unless the call is refused, when it writes nothing more -- writes the
//           search levels (padded with ~0), compares the ragged edges under both keystreams and stores every entry's result whole;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent of the levels, compares
//           the chunk's span and adds to / lowers the entry's result and the summary as the kernel's atomics do.
// It READS both sides where the plan says the kernel reads them and writes only results and workspace, so a sanitizer run sees every
// byte of the workspace layout the host planned and every byte of the caller's buffers the kernels would touch
// (tests/table_calls_main.cpp drives it).
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_rekey_verify_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_rekey_verify_table_launches[3] = {};

void run_plan(RekeyVerifyTableArgs *a)
{
    a->sum->mismatches = 0;
    a->sum->first_bad_entry = kVerifyNone;
    a->sum->entries = a->n;
    a->sum->reserved = 0;
    plan(a, [&](uint64_t i, uint64_t run) {
        const RekeyTableEntry E = a->entries[i];
        const Grid g = grid_of(E, E.flags | E.reserved);
        plan_fields(a->plan[i], E, g, run);
        a->plan[i].pad = 0;
        plan_states(a->plan[i], a->edge[i], E, g);
        return g;
    });
}

// bytes [at, at + len) of a span from its origins, the origin byte's states sa (removed) and sb (applied): the comparand must be
// src ^ ~sa ^ ~sb = src ^ sa ^ sb; j0 = index in the entry of the origin byte (modulo 2^64)
void span_verify(const uint8_t *exp0, const uint8_t *src0, uint64_t at, uint64_t len, uint32_t sa, uint32_t sb, uint64_t j0, unsigned long long &count,
                 unsigned long long &first)
{
    sa = step(sa, at);
    sb = step(sb, at);
    for (uint64_t j = 0; j < len; ++j) {
        if (exp0[at + j] != (uint8_t)(src0[at + j] ^ (uint8_t)(sa ^ sb))) {
            ++count;
            if (j0 + at + j < first) first = j0 + at + j;
        }
        sa = step(sa, 1);
        sb = step(sb, 1);
    }
}

void run_finish(RekeyVerifyTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t i, RekeyTablePlan &P, bool ok) {
        if (!ok) return;
        const RekeyTableEdge &X = a->edge[i];
        const uint64_t body = P.end - P.lead;
        unsigned long long count = 0, first = kVerifyNone;
        span_verify(P.dst_origin + P.lead - P.head_n, P.src_origin + P.lead - P.head_n, 0, P.head_n, X.head[0], X.head[1], 0, count, first);
        span_verify(P.dst_origin + P.end, P.src_origin + P.end, 0, P.tail_n, X.tail[0], X.tail[1], P.head_n + body, count, first);
        a->results[i] = CycleVerifyResult{count, first, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
        if (count) {
            a->sum->mismatches += count;
            if (i < a->sum->first_bad_entry) a->sum->first_bad_entry = i;
        }
    });
}

void run_stream(RekeyVerifyTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const RekeyTablePlan &P = a->plan[s.entry];
        unsigned long long count = 0, first = kVerifyNone;
        span_verify(P.dst_origin, P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base_from, P.base_to, (uint64_t)P.head_n - P.lead, count, first);
        if (count) {
            a->results[s.entry].mismatches += count;
            if (first < a->results[s.entry].first_mismatch) a->results[s.entry].first_mismatch = first;
            a->sum->mismatches += count;
            if (s.entry < a->sum->first_bad_entry) a->sum->first_bad_entry = s.entry;
        }
    });
}
} // namespace

uint32_t modgpu_rekey_verify_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_rekey_verify_table_block() { return 1024u; }
const char *modgpu_rekey_verify_table_kernel_name() { return "shim rekey verify table stream"; }
hipError_t modgpu_launch_rekey_verify_table_plan(const RekeyVerifyTableArgs &a, hipStream_t stream) { return enqueue<RekeyVerifyTableArgs, run_plan, g_rekey_verify_table_launches, 0>(a, stream); }
hipError_t modgpu_launch_rekey_verify_table_finish(const RekeyVerifyTableArgs &a, hipStream_t stream) { return enqueue<RekeyVerifyTableArgs, run_finish, g_rekey_verify_table_launches, 1>(a, stream); }
hipError_t modgpu_launch_rekey_verify_table_stream(const RekeyVerifyTableArgs &a, uint32_t, hipStream_t stream) { return enqueue<RekeyVerifyTableArgs, run_stream, g_rekey_verify_table_launches, 2>(a, stream); }

extern "C" unsigned long long modgpu_shim_rekey_verify_table_launches(int kind) { return count(g_rekey_verify_table_launches, kind); }
