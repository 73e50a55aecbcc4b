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
// byte of the workspace layout the host planned and every byte of the caller's buffers the kernels would touch (no case drives it yet).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_rekey_verify_table_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_rekey_verify_table_launches[3] = {};
constexpr uint64_t kChunk = 65536;

// state of the byte e - 1 positions past the key (e = off + 1 + position); the identity keystream's is 2^31-1, whose byte is 0xFF
uint32_t state(uint32_t k, uint64_t e) { return k ? lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)) : lcg::M; }
uint32_t step(uint32_t s, uint64_t j) { return s == lcg::M ? s : lcg::mulmod(s, lcg::powmod(lcg::A, j % lcg::PERIOD)); }

void run_plan(void *arg)
{
    RekeyVerifyTableArgs *a = static_cast<RekeyVerifyTableArgs *>(arg);
    a->hdr->ticket = 0;
    a->hdr->first_bad = kTableNoBad;
    a->hdr->total = 0;
    a->sum->mismatches = 0;
    a->sum->first_bad_entry = kVerifyNone;
    a->sum->entries = a->n;
    a->sum->reserved = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        uint64_t run = 0;
        uint32_t bad_any = 0;
        for (uint64_t i = (uint64_t)b * kTableBlock; i < a->n && i < (uint64_t)(b + 1) * kTableBlock; ++i) {
            const RekeyTableEntry E = a->entries[i];
            const uint64_t d = reinterpret_cast<uintptr_t>(E.dst);
            const uint64_t head = std::min<uint64_t>(E.n, (16 - (d & 15)) & 15);
            const uint64_t words = (E.n - head) / 16;
            const uint32_t lead = (uint32_t)((d + head) & (kChunk - 1));
            const uint64_t end = lead + words * 16;
            uint64_t cnt = words ? (end + kChunk - 1) / kChunk : 0;
            const uint32_t bad = (E.n && (!E.dst || !E.src)) || E.flags != 0 || E.reserved != 0 || cnt > kTableMaxEntryChunks ? 1u : 0u;
            if (bad) cnt = 0;
            const uint32_t kf = lcg::key_residue(E.key_from), kt = lcg::key_residue(E.key_to);
            const uint64_t of = E.off_from % lcg::PERIOD + 1, ot = E.off_to % lcg::PERIOD + 1;
            const uint64_t body = head + lcg::PERIOD - lead, after = head + (words * 16) % lcg::PERIOD;
            RekeyTablePlan &P = a->plan[i];
            P.dst_origin = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(E.dst) + head - lead); // (as integers: a refused entry's pointer may be NULL)
            P.src_origin = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(E.src) + head - lead);
            P.end = end;
            P.start = run;
            P.lead = lead;
            P.chunks = (uint32_t)cnt;
            P.base_from = state(kf, of + body);
            P.base_to = state(kt, ot + body);
            P.bad = bad;
            P.head_n = (uint32_t)head;
            P.tail_n = (uint32_t)(E.n - head - words * 16);
            P.pad = 0;
            RekeyTableEdge &X = a->edge[i];
            X.head[0] = state(kf, of);
            X.head[1] = state(kt, ot);
            X.tail[0] = state(kf, of + after);
            X.tail[1] = state(kt, ot + after);
            run += cnt;
            bad_any |= bad;
        }
        a->blk[b].chunks = run;
        a->blk[b].bad = bad_any;
    }
    g_rekey_verify_table_launches[0].fetch_add(1);
    delete a;
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

void run_finish(void *arg)
{
    RekeyVerifyTableArgs *a = static_cast<RekeyVerifyTableArgs *>(arg);
    uint64_t total = 0;
    uint32_t bad = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        total += a->blk[b].chunks;
        bad |= a->blk[b].bad;
    }
    const bool ok = !bad && total <= kTableMaxChunks;
    a->hdr->total = ok ? total : 0;
    uint64_t before = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        for (uint64_t i = (uint64_t)b * kTableBlock; i < a->n && i < (uint64_t)(b + 1) * kTableBlock; ++i) {
            RekeyTablePlan &P = a->plan[i];
            const uint64_t start = before + P.start;
            if (!ok) {
                if ((P.bad || start + P.chunks > kTableMaxChunks) && i < a->hdr->first_bad) a->hdr->first_bad = i;
                continue;
            }
            P.start = start;
            for (uint32_t k = 0; k <= a->top; ++k)
                if ((i & ((1ull << (4 * k)) - 1)) == 0) a->level[k][i >> (4 * k)] = (uint32_t)start;
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
        }
        before += a->blk[b].chunks;
    }
    if (ok)
        for (uint32_t k = 0; k <= a->top; ++k)
            for (uint64_t j = a->level_n[k]; j < ((a->level_n[k] + 15) & ~15ull); ++j) a->level[k][j] = ~0u;
    g_rekey_verify_table_launches[1].fetch_add(1);
    delete a;
}

void run_stream(void *arg)
{
    RekeyVerifyTableArgs *a = static_cast<RekeyVerifyTableArgs *>(arg);
    std::this_thread::sleep_for(std::chrono::microseconds(200)); // a launch lasts a while: overlaps between streams become likely
    const uint32_t total = (uint32_t)a->hdr->total;
    for (uint32_t g = 0; g < total; ++g) {
        uint64_t j = 0;
        for (int k = (int)a->top; k >= 0; --k) { // the kernel's descent: 16 keys per level
            uint32_t c = 0;
            for (int t = 0; t < 16; ++t) c += a->level[k][16 * j + t] <= g ? 1u : 0u;
            j = 16 * j + c - 1;
        }
        const RekeyTablePlan &P = a->plan[j];
        const uint64_t c = g - P.start, off = c * kChunk, cut = c ? 0 : P.lead;
        const uint64_t lim = std::min<uint64_t>(P.end, off + kChunk);
        unsigned long long count = 0, first = kVerifyNone;
        span_verify(P.dst_origin, P.src_origin, off + cut, lim - off - cut, P.base_from, P.base_to, (uint64_t)P.head_n - P.lead, count, first);
        if (count) {
            a->results[j].mismatches += count;
            if (first < a->results[j].first_mismatch) a->results[j].first_mismatch = first;
            a->sum->mismatches += count;
            if (j < a->sum->first_bad_entry) a->sum->first_bad_entry = j;
        }
    }
    g_rekey_verify_table_launches[2].fetch_add(1);
    delete a;
}
} // namespace

uint32_t modgpu_rekey_verify_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_rekey_verify_table_block() { return 1024u; }
const char *modgpu_rekey_verify_table_kernel_name() { return "shim rekey verify table stream"; }
hipError_t modgpu_launch_rekey_verify_table_plan(const RekeyVerifyTableArgs &a, hipStream_t stream)
{
    shim::enqueue(stream, run_plan, new RekeyVerifyTableArgs(a));
    return hipSuccess;
}
hipError_t modgpu_launch_rekey_verify_table_finish(const RekeyVerifyTableArgs &a, hipStream_t stream)
{
    shim::enqueue(stream, run_finish, new RekeyVerifyTableArgs(a));
    return hipSuccess;
}
hipError_t modgpu_launch_rekey_verify_table_stream(const RekeyVerifyTableArgs &a, uint32_t, hipStream_t stream)
{
    shim::enqueue(stream, run_stream, new RekeyVerifyTableArgs(a));
    return hipSuccess;
}

extern "C" unsigned long long modgpu_shim_rekey_verify_table_launches(int kind)
{
    return kind >= 0 && kind < 3 ? g_rekey_verify_table_launches[kind].load() : 0;
}
