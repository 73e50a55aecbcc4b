// standin_launch_digest_table.cpp -- the digest table launches (cycle_verify_table_kernel.h: modgpu_launch_digest_table_*) on the CPU
// stand-in (hip/hip_runtime.h).  Like standin_launch_verify_table.cpp: each launch is queued on the stream's thread and does, from its
// arguments and the workspace alone, what the verify table kernels do in their digest mode -- byte by byte with lcg.h:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks every entry and lays it on the chunk grid of its SOURCE (the
//           entry's dst is not looked at), writes the plan and blk records, resets the header; there is no summary line to reset;
//   finish  globalises the starts, decides the status, and -- unless the call is refused, when it writes nothing more -- writes the
//           search levels, sums the ragged edges and stores every entry's record whole;
//   stream  takes every chunk index below the header's total, finds its entry by the kernel's 16-ary descent, sums the chunk's span
//           and ADDS the two residues to the entry's record as the kernel's atomics do.
// It reads the sources where the plan says the kernel reads them and writes only records and workspace.  No row of TABLE: the digest
// loop is part of the verify table TU's kernels, not a TU.
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_verify_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_digest_table_launches[3] = {}, g_digest_table_plan_errors{0};

// k * a^e; 0 for the identity keystream: out = src
uint32_t base_state(uint32_t k, uint64_t e) { return k ? lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)) : 0u; }

void run_plan(VerifyTableArgs *a)
{
    if (a->mode != VERIFY_TABLE_DIGEST || a->sum || a->results || !a->records) g_digest_table_plan_errors.fetch_add(1);
    plan(a, [&](uint64_t i, uint64_t run) {
        CycleTableEntry E = a->entries[i];
        E.dst = const_cast<uint8_t *>(E.src); // the source in the destination's role: whatever dst holds is not looked at
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

// bytes [at, at + len) of a span from its origin, s0 the origin byte's state (0: the identity keystream); j0 = index in the entry of
// the origin byte (modulo 2^64).  Both sums come back reduced.
void span_digest(const uint8_t *src0, uint64_t at, uint64_t len, uint32_t s0, uint64_t j0, uint64_t &s1, uint64_t &s2)
{
    uint32_t s = s0 ? lcg::mulmod(s0, lcg::powmod(lcg::A, at % lcg::PERIOD)) : 0u;
    for (uint64_t j = 0; j < len; ++j) {
        const uint8_t out = s0 ? (uint8_t)(src0[at + j] ^ (uint8_t)~s) : src0[at + j];
        s1 = (s1 + out) % kDigestTableMod;
        s2 = (s2 + ((j0 + at + j) % kDigestTableMod) * out) % kDigestTableMod;
        if (s0) s = lcg::mulmod(s, lcg::A);
    }
}

void run_finish(VerifyTableArgs *a)
{
    finish(a, kTableMaxChunks, [&](uint64_t i, CycleTablePlan &P, bool ok) {
        if (!ok) return;
        const uint64_t body = P.end - P.lead;
        uint64_t s1 = 0, s2 = 0;
        span_digest(P.src_origin + P.lead - P.head_n, 0, P.head_n, P.base_head, 0, s1, s2);
        span_digest(P.src_origin + P.end, 0, P.tail_n, P.base_tail, P.head_n + body, s1, s2);
        a->records[i] = DigestTableRecord{s1, s2, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
    });
}

void run_stream(VerifyTableArgs *a)
{
    stream(a, [&](const Span &s) {
        const CycleTablePlan &P = a->plan[s.entry];
        if (P.dst_origin != P.src_origin || (reinterpret_cast<uintptr_t>(P.src_origin) & 15) != 0) g_digest_table_plan_errors.fetch_add(1);
        uint64_t s1 = 0, s2 = 0;
        span_digest(P.src_origin, s.off + s.cut, s.lim - s.off - s.cut, P.base, (uint64_t)P.head_n - P.lead, s1, s2);
        a->records[s.entry].s1 += s1;
        a->records[s.entry].s2 += s2;
    });
}

VerifyTableArgs digest_mode(const VerifyTableArgs &a)
{
    VerifyTableArgs d = a;
    d.mode = VERIFY_TABLE_DIGEST;
    return d;
}
} // namespace

hipError_t modgpu_launch_digest_table_plan(const VerifyTableArgs &a, hipStream_t stream) { return enqueue<VerifyTableArgs, run_plan, g_digest_table_launches, 0>(digest_mode(a), stream); }
hipError_t modgpu_launch_digest_table_finish(const VerifyTableArgs &a, hipStream_t stream) { return enqueue<VerifyTableArgs, run_finish, g_digest_table_launches, 1>(digest_mode(a), stream); }
hipError_t modgpu_launch_digest_table_stream(const VerifyTableArgs &a, uint32_t, hipStream_t stream) { return enqueue<VerifyTableArgs, run_stream, g_digest_table_launches, 2>(digest_mode(a), stream); }

extern "C" unsigned long long modgpu_shim_digest_table_launches(int kind) { return count(g_digest_table_launches, kind); }
extern "C" unsigned long long modgpu_shim_digest_table_plan_errors(void) { return g_digest_table_plan_errors.load(); }
