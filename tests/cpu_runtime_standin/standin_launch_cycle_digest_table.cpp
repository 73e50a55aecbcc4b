// standin_launch_cycle_digest_table.cpp -- the cycle digest table launches (cycle_table_kernel.h: modgpu_launch_cycle_digest_table_*) on
// the CPU stand-in (hip/hip_runtime.h).  Like standin_launch_table.cpp: each launch is queued on the stream's thread and does, from its
// arguments and the workspace alone, what the table kernels do in their digest mode -- byte by byte with lcg.h:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks every entry and lays it on the chunk grid of its DESTINATION,
//           writes the plan and blk records, resets the header;
//   finish  globalises the starts, decides the status, and -- unless the call is refused, when it writes nothing more -- writes the
//           search levels, cycles the ragged edges, sums them on the call's side of the XOR and stores every entry's record whole;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent, cycles the chunk's span
//           of the destination, sums it on the call's side and ADDS the two residues to the entry's record as the kernel's atomics do.
// A span is summed before it is stored: with dst == src the input side is what was there before the call.  No row of TABLE: the loop is
// part of the out-of-place table TU's kernels, not a TU.
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_cycle_digest_table_launches[3] = {}, g_cycle_digest_table_plan_errors{0};

// k * a^e; 0 for the identity keystream (key == 0 mod 2^31-1): a copy
uint32_t base_state(uint32_t k, uint64_t e) { return lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)); }

void run_plan(CycleTableArgs *a)
{
    if (a->mode != CYCLE_TABLE_DIGEST || a->side > CYCLE_TABLE_SIDE_INPUT || !a->records) g_cycle_digest_table_plan_errors.fetch_add(1);
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

// bytes [at, at + len) of a span from its origin, `base` the origin byte's state (0: a copy), cycled into dst0 and summed on `side`;
// j0 = index in the entry of the origin byte (modulo 2^64).  Both sums come back reduced.
void span_cycle_digest(uint8_t *dst0, const uint8_t *src0, uint64_t at, uint64_t len, uint32_t base, uint32_t side, uint64_t j0, uint64_t &s1, uint64_t &s2)
{
    uint32_t s = base ? lcg::mulmod(base, lcg::powmod(lcg::A, at % lcg::PERIOD)) : 0;
    for (uint64_t j = 0; j < len; ++j) {
        const uint8_t in = src0[at + j];
        const uint8_t out = base ? (uint8_t)(in ^ (uint8_t)~s) : in;
        const uint8_t x = side == CYCLE_TABLE_SIDE_INPUT ? in : out;
        s1 = (s1 + x) % kDigestTableMod;
        s2 = (s2 + ((j0 + at + j) % kDigestTableMod) * x) % kDigestTableMod;
        dst0[at + j] = out;
        s = lcg::mulmod(s, lcg::A);
    }
}

void run_finish(CycleTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t i, CycleTablePlan &P, bool ok) {
        if (!ok) return;
        const uint64_t body = P.end - P.lead;
        uint64_t s1 = 0, s2 = 0;
        // the ragged edges: the head ends where the body starts, the tail starts where it ends (an empty entry's pointers may be NULL:
        // no address is made of them)
        if (P.head_n) span_cycle_digest(P.dst_origin + P.lead - P.head_n, P.src_origin + P.lead - P.head_n, 0, P.head_n, P.base_head, a->side, 0, s1, s2);
        if (P.tail_n) span_cycle_digest(P.dst_origin + P.end, P.src_origin + P.end, 0, P.tail_n, P.base_tail, a->side, P.head_n + body, s1, s2);
        a->records[i] = DigestTableRecord{s1, s2, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
    });
}

void run_stream(CycleTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const CycleTablePlan &P = a->plan[s.entry];
        if ((reinterpret_cast<uintptr_t>(P.dst_origin) & (kChunk - 1)) != 0) g_cycle_digest_table_plan_errors.fetch_add(1);
        uint64_t s1 = 0, s2 = 0;
        span_cycle_digest(P.dst_origin, P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base, a->side, (uint64_t)P.head_n - P.lead, s1, s2);
        a->records[s.entry].s1 += s1;
        a->records[s.entry].s2 += s2;
    });
}

CycleTableArgs digest_mode(const CycleTableArgs &a)
{
    CycleTableArgs d = a;
    d.mode = CYCLE_TABLE_DIGEST;
    return d;
}
} // namespace

hipError_t modgpu_launch_cycle_digest_table_plan(const CycleTableArgs &a, hipStream_t stream)
{
    return enqueue<CycleTableArgs, run_plan, g_cycle_digest_table_launches, 0>(digest_mode(a), stream);
}
hipError_t modgpu_launch_cycle_digest_table_finish(const CycleTableArgs &a, hipStream_t stream)
{
    return enqueue<CycleTableArgs, run_finish, g_cycle_digest_table_launches, 1>(digest_mode(a), stream);
}
hipError_t modgpu_launch_cycle_digest_table_stream(const CycleTableArgs &a, uint32_t, hipStream_t stream)
{
    return enqueue<CycleTableArgs, run_stream, g_cycle_digest_table_launches, 2>(digest_mode(a), stream);
}

extern "C" unsigned long long modgpu_shim_cycle_digest_table_launches(int kind) { return count(g_cycle_digest_table_launches, kind); }
extern "C" unsigned long long modgpu_shim_cycle_digest_table_plan_errors(void) { return g_cycle_digest_table_plan_errors.load(); }
