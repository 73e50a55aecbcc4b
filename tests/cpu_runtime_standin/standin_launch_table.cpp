// standin_launch_table.cpp -- the table launches (cycle_table_kernel.h) on the CPU stand-in (hip/hip_runtime.h).  Each launch is queued
// on the stream's thread and does, from its arguments and the workspace alone, what the kernel would do -- byte by byte with lcg.h:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks and lays out every entry, writes the plan and blk records, resets
//           the header;
//   finish  globalises the starts, decides the status, writes the search levels (padded with ~0) and cycles the ragged edges;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent of the levels, and
//           cycles the chunk's span of the destination from the plan record.
// So the sanitizer runs see every byte of the workspace layout the host planned, and every byte of the caller's buffers the kernels
// would read or write.
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_table_launches[3] = {};

// k * a^e; 0 for the identity keystream (key == 0 mod 2^31-1): a copy
uint32_t base_state(uint32_t k, uint64_t e) { return lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)); }

void run_plan(CycleTableArgs *a)
{
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

// bytes [at, at + len) of an entry's span from the chunk origin, state of the origin byte `base` (0: copy)
void span_cycle(uint8_t *dst0, const uint8_t *src0, uint64_t at, uint64_t len, uint32_t base)
{
    uint32_t s = base ? lcg::mulmod(base, lcg::powmod(lcg::A, at % lcg::PERIOD)) : 0;
    for (uint64_t j = 0; j < len; ++j) {
        dst0[at + j] = base ? (uint8_t)(src0[at + j] ^ (uint8_t)~s) : src0[at + j];
        s = lcg::mulmod(s, lcg::A);
    }
}

void run_finish(CycleTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t, CycleTablePlan &P, bool ok) {
        if (!ok) return;
        // the ragged edges: the head ends where the body starts, the tail starts where it ends
        span_cycle(P.dst_origin + P.lead - P.head_n, P.src_origin + P.lead - P.head_n, 0, P.head_n, P.base_head);
        span_cycle(P.dst_origin + P.end, P.src_origin + P.end, 0, P.tail_n, P.base_tail);
    });
}

void run_stream(CycleTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const CycleTablePlan &P = a->plan[s.entry];
        span_cycle(P.dst_origin, P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base);
    });
}
} // namespace

uint32_t modgpu_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_table_block() { return 1024u; }
const char *modgpu_table_kernel_name() { return "shim table stream"; }
hipError_t modgpu_launch_table_plan(const CycleTableArgs &a, hipStream_t stream) { return enqueue<CycleTableArgs, run_plan, g_table_launches, 0>(a, stream); }
hipError_t modgpu_launch_table_finish(const CycleTableArgs &a, hipStream_t stream) { return enqueue<CycleTableArgs, run_finish, g_table_launches, 1>(a, stream); }
hipError_t modgpu_launch_table_stream(const CycleTableArgs &a, uint32_t, hipStream_t stream) { return enqueue<CycleTableArgs, run_stream, g_table_launches, 2>(a, stream); }

extern "C" unsigned long long modgpu_shim_table_launches(int kind) { return count(g_table_launches, kind); }
