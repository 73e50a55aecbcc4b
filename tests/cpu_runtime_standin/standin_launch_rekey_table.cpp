// standin_launch_rekey_table.cpp -- the rekey table launches (cycle_rekey_table_kernel.h) on the CPU stand-in (hip/hip_runtime.h).
// Each launch is queued on the stream's thread and does, from its arguments and the workspace alone, what the kernel would do -- byte
// by byte with lcg.h, the identity keystream's state kept as 2^31-1 as the kernels keep it:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks and lays out every entry, writes the plan, edge and blk records,
//           resets the header;
//   finish  globalises the starts, decides the status, writes the search levels (padded with ~0) and rekeys the ragged edges;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent of the levels, and
//           rekeys the chunk's span of the destination from the plan record.
// So the sanitizer runs see every byte of the workspace layout the host planned, and every byte of the caller's buffers the kernels
// would read or write.
#include "standin_table.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_rekey_table_launches[3] = {};

void run_plan(RekeyTableArgs *a)
{
    plan(a, [&](uint64_t i, uint64_t run) {
        const RekeyTableEntry E = a->entries[i];
        const Grid g = grid_of(E, E.flags | E.reserved);
        plan_fields(a->plan[i], E, g, run);
        a->plan[i].pad = 0;
        plan_states(a->plan[i], a->edge[i], E, g);
        return g;
    });
}

// bytes [at, at + len) of a span from its origin, the origin byte's states sa (removed) and sb (applied): d ^ ~sa ^ ~sb = d ^ sa ^ sb
void span_rekey(uint8_t *dst0, const uint8_t *src0, uint64_t at, uint64_t len, uint32_t sa, uint32_t sb)
{
    sa = step(sa, at);
    sb = step(sb, at);
    for (uint64_t j = 0; j < len; ++j) {
        dst0[at + j] = (uint8_t)(src0[at + j] ^ (uint8_t)(sa ^ sb));
        sa = step(sa, 1);
        sb = step(sb, 1);
    }
}

void run_finish(RekeyTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t i, RekeyTablePlan &P, bool ok) {
        if (!ok) return;
        const RekeyTableEdge &X = a->edge[i];
        span_rekey(P.dst_origin + P.lead - P.head_n, P.src_origin + P.lead - P.head_n, 0, P.head_n, X.head[0], X.head[1]);
        span_rekey(P.dst_origin + P.end, P.src_origin + P.end, 0, P.tail_n, X.tail[0], X.tail[1]);
    });
}

void run_stream(RekeyTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const RekeyTablePlan &P = a->plan[s.entry];
        span_rekey(P.dst_origin, P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base_from, P.base_to);
    });
}
} // namespace

uint32_t modgpu_rekey_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_rekey_table_block() { return 1024u; }
const char *modgpu_rekey_table_kernel_name() { return "shim rekey table stream"; }
hipError_t modgpu_launch_rekey_table_plan(const RekeyTableArgs &a, hipStream_t stream) { return enqueue<RekeyTableArgs, run_plan, g_rekey_table_launches, 0>(a, stream); }
hipError_t modgpu_launch_rekey_table_finish(const RekeyTableArgs &a, hipStream_t stream) { return enqueue<RekeyTableArgs, run_finish, g_rekey_table_launches, 1>(a, stream); }
hipError_t modgpu_launch_rekey_table_stream(const RekeyTableArgs &a, uint32_t, hipStream_t stream) { return enqueue<RekeyTableArgs, run_stream, g_rekey_table_launches, 2>(a, stream); }

extern "C" unsigned long long modgpu_shim_rekey_table_launches(int kind) { return count(g_rekey_table_launches, kind); }
