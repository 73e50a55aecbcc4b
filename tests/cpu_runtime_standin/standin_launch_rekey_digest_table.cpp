// standin_launch_rekey_digest_table.cpp -- the rekey digest table launches (cycle_rekey_table_kernel.h: modgpu_launch_rekey_digest_table_*)
// on the CPU stand-in (hip/hip_runtime.h).  Like standin_launch_rekey_table.cpp: each launch is queued on the stream's thread and does,
// from its arguments and the workspace alone, what the rekey table kernels do in their digest mode -- byte by byte with lcg.h, the
// identity keystream's state kept as 2^31-1:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks every entry and lays it on the chunk grid of its DESTINATION,
//           writes the plan, edge and blk records, resets the header;
//   finish  globalises the starts, decides the status, and -- unless the call is refused, when it writes nothing more -- writes the
//           search levels, rekeys the ragged edges, sums them on the call's side and stores every entry's record whole;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent, rekeys the chunk's span of
//           the destination, sums it on the call's side and ADDS the two residues to the entry's record as the kernel's atomics do.
// A span is summed before it is stored: with dst == src the input side is what was there before the call.  No row of TABLE: the loop is
// part of the rekey table TU's kernels, not a TU.
#include "standin_table.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_rekey_digest_table_launches[3] = {}, g_rekey_digest_table_plan_errors{0};

void run_plan(RekeyTableArgs *a)
{
    if (a->mode != REKEY_TABLE_DIGEST || a->side > REKEY_TABLE_SIDE_PLAIN || !a->records) g_rekey_digest_table_plan_errors.fetch_add(1);
    plan(a, [&](uint64_t i, uint64_t run) {
        const RekeyTableEntry E = a->entries[i];
        const Grid g = grid_of(E, E.flags | E.reserved);
        plan_fields(a->plan[i], E, g, run);
        a->plan[i].pad = 0;
        plan_states(a->plan[i], a->edge[i], E, g);
        return g;
    });
}

// bytes [at, at + len) of a span from its origin, the origin byte's states sa (removed) and sb (applied), rekeyed into dst0 and summed
// on `side`; j0 = index in the entry of the origin byte (modulo 2^64).  Both sums come back reduced.
void span_rekey_digest(uint8_t *dst0, const uint8_t *src0, uint64_t at, uint64_t len, uint32_t sa, uint32_t sb, uint32_t side, uint64_t j0, uint64_t &s1,
                       uint64_t &s2)
{
    sa = step(sa, at);
    sb = step(sb, at);
    for (uint64_t j = 0; j < len; ++j) {
        const uint8_t in = src0[at + j];
        const uint8_t plain = (uint8_t)(in ^ (uint8_t)~sa);
        const uint8_t out = (uint8_t)(plain ^ (uint8_t)~sb);
        const uint8_t x = side == REKEY_TABLE_SIDE_INPUT ? in : side == REKEY_TABLE_SIDE_PLAIN ? plain : out;
        s1 = (s1 + x) % kDigestTableMod;
        s2 = (s2 + ((j0 + at + j) % kDigestTableMod) * x) % kDigestTableMod;
        dst0[at + j] = out;
        sa = step(sa, 1);
        sb = step(sb, 1);
    }
}

void run_finish(RekeyTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t i, RekeyTablePlan &P, bool ok) {
        if (!ok) return;
        const RekeyTableEdge &X = a->edge[i];
        const uint64_t body = P.end - P.lead;
        uint64_t s1 = 0, s2 = 0;
        // (an empty entry's pointers may be NULL: no address is made of them)
        if (P.head_n) span_rekey_digest(P.dst_origin + P.lead - P.head_n, P.src_origin + P.lead - P.head_n, 0, P.head_n, X.head[0], X.head[1], a->side, 0, s1, s2);
        if (P.tail_n) span_rekey_digest(P.dst_origin + P.end, P.src_origin + P.end, 0, P.tail_n, X.tail[0], X.tail[1], a->side, P.head_n + body, s1, s2);
        a->records[i] = DigestTableRecord{s1, s2, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
    });
}

void run_stream(RekeyTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const RekeyTablePlan &P = a->plan[s.entry];
        if ((reinterpret_cast<uintptr_t>(P.dst_origin) & (kChunk - 1)) != 0) g_rekey_digest_table_plan_errors.fetch_add(1);
        uint64_t s1 = 0, s2 = 0;
        span_rekey_digest(P.dst_origin, P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base_from, P.base_to, a->side, (uint64_t)P.head_n - P.lead, s1, s2);
        a->records[s.entry].s1 += s1;
        a->records[s.entry].s2 += s2;
    });
}

RekeyTableArgs digest_mode(const RekeyTableArgs &a)
{
    RekeyTableArgs d = a;
    d.mode = REKEY_TABLE_DIGEST;
    return d;
}
} // namespace

hipError_t modgpu_launch_rekey_digest_table_plan(const RekeyTableArgs &a, hipStream_t stream)
{
    return enqueue<RekeyTableArgs, run_plan, g_rekey_digest_table_launches, 0>(digest_mode(a), stream);
}
hipError_t modgpu_launch_rekey_digest_table_finish(const RekeyTableArgs &a, hipStream_t stream)
{
    return enqueue<RekeyTableArgs, run_finish, g_rekey_digest_table_launches, 1>(digest_mode(a), stream);
}
hipError_t modgpu_launch_rekey_digest_table_stream(const RekeyTableArgs &a, uint32_t, hipStream_t stream)
{
    return enqueue<RekeyTableArgs, run_stream, g_rekey_digest_table_launches, 2>(digest_mode(a), stream);
}

extern "C" unsigned long long modgpu_shim_rekey_digest_table_launches(int kind) { return count(g_rekey_digest_table_launches, kind); }
extern "C" unsigned long long modgpu_shim_rekey_digest_table_plan_errors(void) { return g_rekey_digest_table_plan_errors.load(); }
