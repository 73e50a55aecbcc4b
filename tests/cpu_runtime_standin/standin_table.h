// standin_table.h -- what the five table stand-ins (standin_launch_{table,rekey_table,verify_table,rekey_verify_table,rekey_move_table}.cpp)
// have in common, once: an entry on the chunk grid of its destination and the device tier's refusal rule, the plan-record fields every
// kind has, the walk over the 1024-entry records, the finish launch's scaffold (totals, status, globalised starts, search levels padded
// with ~0), the 16-ary descent from a chunk to its entry and the chunk's span, the two-keystream states, and the enqueue wrappers with
// their counters.  Each stand-in keeps what is its own: its base states, what it does to a span, its edges, its results.
// A SECOND implementation of the kernels' rules, written from the record types (the *_kernel.h headers) and lcg.h alone: no device code
// is included here, so that a fault in cycle_table_impl.h shows as a difference and not twice.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_rekey_table_kernel.h" // (and through it cycle_table_kernel.h): record types and limits only
#include "../../modulate_amd/csrc/lcg.h"

namespace standin_table {
constexpr uint64_t kChunk = 65536;

inline uint64_t at(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// The two-keystream kinds' states: that of the byte e - 1 positions past the key (e = off + 1 + position); the identity keystream's is
// kept as 2^31-1, whose byte is 0xFF, as the kernels keep it
inline uint32_t state(uint32_t k, uint64_t e) { return k ? lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)) : lcg::M; }
inline uint32_t step(uint32_t s, uint64_t j) { return s == lcg::M ? s : lcg::mulmod(s, lcg::powmod(lcg::A, j % lcg::PERIOD)); }

// An entry on the chunk grid of its destination: < 16 bytes of head up to the first 16-byte word, the body's words from `lead` bytes
// into a chunk up to `end` (both from the chunk origin), its chunk count -- none if the device tier refuses the entry: a NULL pointer
// with bytes to do, something set in `must_be_zero` (flags[, reserved]), more chunks than the jump tables reach.  `origin` and `tail`
// are the stream positions, from the entry's first byte, of the chunk origin (modulo the period) and of the first byte behind the body.
struct Grid {
    uint64_t head, words, end, cnt, origin, tail;
    uint32_t lead, bad;
};
template <class Entry> Grid grid_of(const Entry &E, uint32_t must_be_zero)
{
    Grid g{};
    const uint64_t d = at(E.dst);
    g.head = std::min<uint64_t>(E.n, (16 - (d & 15)) & 15);
    g.words = (E.n - g.head) / 16;
    g.lead = (uint32_t)((d + g.head) & (kChunk - 1));
    g.end = g.lead + g.words * 16;
    g.cnt = g.words ? (g.end + kChunk - 1) / kChunk : 0;
    g.bad = (E.n && (!E.dst || !E.src)) || must_be_zero != 0 || g.cnt > kTableMaxEntryChunks ? 1u : 0u;
    if (g.bad) g.cnt = 0;
    g.origin = g.head + lcg::PERIOD - g.lead;
    g.tail = g.head + (g.words * 16) % lcg::PERIOD;
    return g;
}

// The fields every kind's plan record has; `run` = the chunks of the entries before it in its 1024-entry record
template <class Plan, class Entry> void plan_fields(Plan &P, const Entry &E, const Grid &g, uint64_t run)
{
    P.dst_origin = reinterpret_cast<uint8_t *>(at(E.dst) + g.head - g.lead); // (as integers: a refused entry's pointer may be NULL)
    P.src_origin = reinterpret_cast<const uint8_t *>(at(E.src) + g.head - g.lead);
    P.end = g.end;
    P.start = run;
    P.lead = g.lead;
    P.chunks = (uint32_t)g.cnt;
    P.bad = g.bad;
    P.head_n = (uint32_t)g.head;
    P.tail_n = (uint32_t)(E.n - g.head - g.words * 16);
}
// ... and the six states of a two-keystream kind: both streams at the chunk origin, at the head and at the tail
template <class Plan> void plan_states(Plan &P, RekeyTableEdge &X, const RekeyTableEntry &E, const Grid &g)
{
    const uint32_t kf = lcg::key_residue(E.key_from), kt = lcg::key_residue(E.key_to);
    const uint64_t of = E.off_from % lcg::PERIOD + 1, ot = E.off_to % lcg::PERIOD + 1;
    P.base_from = state(kf, of + g.origin);
    P.base_to = state(kt, ot + g.origin);
    X.head[0] = state(kf, of);
    X.head[1] = state(kt, ot);
    X.tail[0] = state(kf, of + g.tail);
    X.tail[1] = state(kt, ot + g.tail);
}

// The plan launch: resets the header, then takes every entry through entry(i, run) -> Grid, one 1024-entry record after the other, and
// writes the record's chunk count and whether one of its entries is bad (the record's other fields, if it has any, are entry's)
template <class Args, class PerEntry> void plan(Args *a, PerEntry entry)
{
    a->hdr->ticket = 0;
    a->hdr->first_bad = kTableNoBad;
    a->hdr->total = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        uint64_t run = 0;
        uint32_t bad = 0;
        for (uint64_t i = (uint64_t)b * kTableBlock; i < a->n && i < (uint64_t)(b + 1) * kTableBlock; ++i) {
            const Grid g = entry(i, run);
            run += g.cnt;
            bad |= g.bad;
        }
        a->blk[b].chunks = run;
        a->blk[b].bad = bad;
    }
}

// The finish launch: the total over the records and the status -- refused if an entry is bad or the chunks pass `room`, and then the
// lowest entry that is bad or whose chunks end beyond it is named --; unless refused, every entry's start globalised and written into
// the search levels, each level padded with ~0 to a multiple of 16.  entry(i, P, ok) follows for every entry, refused call or not.
template <class Args, class PerEntry> void finish(Args *a, uint64_t room, PerEntry entry)
{
    uint64_t total = 0;
    uint32_t bad = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        total += a->blk[b].chunks;
        bad |= a->blk[b].bad;
    }
    const bool ok = !bad && total <= room;
    a->hdr->total = ok ? total : 0;
    uint64_t before = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        for (uint64_t i = (uint64_t)b * kTableBlock; i < a->n && i < (uint64_t)(b + 1) * kTableBlock; ++i) {
            auto &P = a->plan[i];
            const uint64_t start = before + P.start;
            if (!ok && (P.bad || start + P.chunks > room) && i < a->hdr->first_bad) a->hdr->first_bad = i;
            if (ok) {
                P.start = start;
                for (uint32_t k = 0; k <= a->top; ++k)
                    if ((i & ((1ull << (4 * k)) - 1)) == 0) a->level[k][i >> (4 * k)] = (uint32_t)start;
            }
            entry(i, P, ok);
        }
        before += a->blk[b].chunks;
    }
    if (ok)
        for (uint32_t k = 0; k <= a->top; ++k)
            for (uint64_t j = a->level_n[k]; j < ((a->level_n[k] + 15) & ~15ull); ++j) a->level[k][j] = ~0u;
}

// Global chunk g: its entry by the kernel's descent (16 keys per level), and its span [off + cut, lim) from the entry's chunk origin
struct Span {
    uint64_t entry, off, cut, lim;
};
template <class Args> Span chunk_span(const Args &a, uint32_t g)
{
    uint64_t j = 0;
    for (int k = (int)a.top; k >= 0; --k) {
        uint32_t c = 0;
        for (int t = 0; t < 16; ++t) c += a.level[k][16 * j + t] <= g ? 1u : 0u;
        j = 16 * j + c - 1;
    }
    const auto &P = a.plan[j];
    const uint64_t c = g - P.start, off = c * kChunk;
    return {j, off, c ? 0 : (uint64_t)P.lead, std::min<uint64_t>(P.end, off + kChunk)};
}
// The stream launch of a three-launch call: every chunk below the header's total, in order
template <class Args, class PerChunk> void stream(Args *a, PerChunk chunk)
{
    std::this_thread::sleep_for(std::chrono::microseconds(200)); // a launch lasts a while: overlaps between streams become likely
    const uint32_t total = (uint32_t)a->hdr->total;
    for (uint32_t g = 0; g < total; ++g) chunk(chunk_span(*a, g));
}

// A launch: Run(a copy of the arguments) queued on the stream's thread, counted in Counts[Kind] once it has run
template <class Args, void (*Run)(Args *), auto &Counts, int Kind> hipError_t enqueue(const Args &a, hipStream_t stream)
{
    shim::enqueue(
        stream,
        [](void *arg) {
            Args *p = static_cast<Args *>(arg);
            Run(p);
            Counts[Kind].fetch_add(1);
            delete p;
        },
        new Args(a));
    return hipSuccess;
}
template <size_t N> unsigned long long count(const std::atomic<unsigned long long> (&counts)[N], int kind)
{
    return kind >= 0 && kind < (int)N ? counts[kind].load() : 0;
}
} // namespace standin_table
