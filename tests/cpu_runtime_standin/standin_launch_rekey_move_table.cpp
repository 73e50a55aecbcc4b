// standin_launch_rekey_move_table.cpp -- the rekey move table launches (cycle_rekey_move_table_kernel.h) on the CPU stand-in
// (hip/hip_runtime.h).  Each launch is queued on the stream's thread and does, from its arguments and the workspace alone, what the
// kernel would do -- byte by byte with lcg.h, the identity keystream's state kept as 2^31-1 as the kernels keep it:
//   plan    reads the table from "device" memory WHEN IT RUNS, checks and lays out every entry, writes the plan, edge and blk records
//           (the previous non-empty entry and the first strictly downward / upward entry among each 1024 included), resets the header
//           and every flag;
//   finish  globalises the starts, decides the direction and the status -- each non-empty entry against the non-empty one before it --,
//           writes the search levels and rekeys the ragged ends INTO SCRATCH;
//   window  for every chunk, the chunks at lower positions whose source reads (rounded out to source dwords) meet its destination,
//           by a linear walk -- not the kernel's binary searches: the two must agree;
//   move    walks the POSITIONS in order, one chunk at a time through a buffer of its own: flag up, then the store -- and counts a
//           plan error if a chunk of the window is not flagged yet, or lies at a higher position.  A window that misses a chunk gives
//           wrong bytes here as it would on the device, since the walk stores each chunk before it loads the next;
//   place   the ragged ends from scratch into place.
// So the sanitizer runs see every byte of the workspace layout the host planned, and every byte of the caller's buffers the kernels
// would read or write.
#include "standin_table.h"

#include <vector>

#include "../../modulate_amd/csrc/cycle_rekey_move_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_move_table_launches[5] = {}, g_move_table_plan_errors{0};
constexpr uint32_t kNone = ~0u;

void run_plan(MoveTableArgs *a)
{
    a->hdr->stalled = 0;
    a->hdr->up = 0;
    for (uint64_t k = 0; k < a->cap; ++k) a->flags[k] = 0;
    uint32_t prev = 0; // 1 + the previous non-empty entry of the record (local index)
    plan(a, [&](uint64_t i, uint64_t run) {
        MoveTableBlk &B = a->blk[i / kTableBlock];
        if (i % kTableBlock == 0) {
            B = MoveTableBlk{0, 0, 0, kNone, kNone, {0, 0}};
            prev = 0;
        }
        const RekeyTableEntry E = a->entries[i];
        const Grid g = grid_of(E, E.flags | E.reserved);
        plan_fields(a->plan[i], E, g, run);
        a->plan[i].prev = prev;
        plan_states(a->plan[i], a->edge[i], E, g);
        if (E.n) {
            prev = (uint32_t)(i % kTableBlock) + 1;
            B.last = (uint32_t)i + 1;
            if (at(E.dst) < at(E.src) && B.first_down == kNone) B.first_down = (uint32_t)i;
            if (at(E.dst) > at(E.src) && B.first_up == kNone) B.first_up = (uint32_t)i;
        }
        return g;
    });
}

// bytes [at0, at0 + len) of a span from its origin into out[0 .. len), the origin byte's states sa (removed) and sb (applied)
void span_rekey(uint8_t *out, const uint8_t *src0, uint64_t at0, uint64_t len, uint32_t sa, uint32_t sb)
{
    sa = step(sa, at0);
    sb = step(sb, at0);
    for (uint64_t j = 0; j < len; ++j) {
        out[j] = (uint8_t)(src0[at0 + j] ^ (uint8_t)(sa ^ sb));
        sa = step(sa, 1);
        sb = step(sb, 1);
    }
}

void run_finish(MoveTableArgs *a)
{
    uint32_t down = kNone, up = kNone;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        down = std::min(down, a->blk[b].first_down);
        up = std::min(up, a->blk[b].first_up);
    }
    const bool upward = up < down;
    a->hdr->up = upward ? 1u : 0u;
    uint32_t last = 0; // 1 + the last non-empty entry of the earlier records
    finish(a, std::min<uint64_t>(a->cap, kTableMaxChunks), [&](uint64_t i, MoveTablePlan &P, bool ok) {
        const uint64_t b = i / kTableBlock;
        if (i % kTableBlock == 0 && b > 0 && a->blk[b - 1].last) last = a->blk[b - 1].last;
        // the direction and order rule: each non-empty entry against the non-empty one before it
        const RekeyTableEntry E = a->entries[i];
        if (E.n != 0 && !P.bad) {
            const uint64_t d = at(E.dst), s = at(E.src);
            bool breaks = upward ? d < s : d > s;
            const uint64_t q = P.prev ? b * kTableBlock + P.prev - 1 : last ? (uint64_t)last - 1 : kTableNoBad;
            if (q != kTableNoBad) {
                const RekeyTableEntry Q = a->entries[q];
                breaks = breaks || s < at(Q.src) || s - at(Q.src) < Q.n || d < at(Q.dst) || d - at(Q.dst) < Q.n;
            }
            if (breaks) a->hdr->first_bad = std::min<uint64_t>(a->hdr->first_bad, i);
        }
        if (!ok) return;
        const RekeyTableEdge &X = a->edge[i];
        uint8_t *out = a->scratch + i * kMoveTableScratch;
        span_rekey(out, P.src_origin + P.lead - P.head_n, 0, P.head_n, X.head[0], X.head[1]);
        span_rekey(out + 16, P.src_origin + P.end, 0, P.tail_n, X.tail[0], X.tail[1]);
    });
}

void run_window(MoveTableArgs *a)
{
    if (a->hdr->first_bad == kTableNoBad) {
        const uint32_t total = (uint32_t)a->hdr->total;
        const bool up = a->hdr->up != 0;
        std::vector<uint64_t> s0(total), s1(total), d0(total), d1(total);
        for (uint32_t g = 0; g < total; ++g) {
            const Span s = chunk_span(*a, g);
            d0[g] = at(a->plan[s.entry].dst_origin) + s.off + s.cut;
            d1[g] = at(a->plan[s.entry].dst_origin) + s.lim;
            s0[g] = (at(a->plan[s.entry].src_origin) + s.off + s.cut) & ~3ull;
            s1[g] = (at(a->plan[s.entry].src_origin) + s.lim + 3) & ~3ull;
        }
        for (uint32_t g = 0; g < total; ++g) {
            // walking away from g over the lower positions: the sources only move away from the destination once they have passed it
            MoveTableWin w{0, 0};
            if (!up) {
                uint32_t hi = g;
                while (hi > 0 && s0[hi - 1] >= d1[g]) --hi;
                uint32_t lo = hi;
                while (lo > 0 && s1[lo - 1] > d0[g]) --lo;
                w = {lo, hi - lo};
            } else {
                uint32_t lo = g + 1;
                while (lo < total && s1[lo] <= d0[g]) ++lo;
                uint32_t hi = lo;
                while (hi < total && s0[hi] < d1[g]) ++hi;
                w = {lo, hi - lo};
            }
            a->win[g] = w;
        }
    }
}

void run_move(MoveTableArgs *a)
{
    unsigned long long bad = 0;
    const uint32_t total = a->hdr->first_bad == kTableNoBad ? (uint32_t)a->hdr->total : 0;
    const bool up = a->hdr->up != 0;
    std::vector<uint8_t> buf(kChunk);
    for (uint32_t p = 0; p < total; ++p) {
        const uint32_t g = up ? total - 1 - p : p;
        const Span s = chunk_span(*a, g);
        const uint64_t len = s.lim - s.off - s.cut;
        span_rekey(buf.data(), a->plan[s.entry].src_origin, s.off + s.cut, len, a->plan[s.entry].base_from, a->plan[s.entry].base_to);
        a->flags[g] = 1;
        const MoveTableWin w = a->win[g];
        for (uint32_t i = 0; i < w.n; ++i) {
            const uint32_t k = w.lo + i;
            bad += k >= total || a->flags[k] == 0 || (up ? k <= g : k >= g); // not loaded yet, or not a lower position
        }
        // ... and the window misses nothing: every other chunk whose source BYTES meet this destination is in it
        for (uint32_t k = 0; k < total; ++k) {
            if (k == g) continue;
            const Span o = chunk_span(*a, k);
            const uint64_t o0 = at(a->plan[o.entry].src_origin) + o.off + o.cut, o1 = at(a->plan[o.entry].src_origin) + o.lim;
            const uint64_t d0 = at(a->plan[s.entry].dst_origin) + s.off + s.cut, d1 = at(a->plan[s.entry].dst_origin) + s.lim;
            if (o0 < d1 && o1 > d0) bad += !(k - w.lo < w.n);
        }
        std::copy(buf.begin(), buf.begin() + (ptrdiff_t)len, a->plan[s.entry].dst_origin + s.off + s.cut);
    }
    a->hdr->ticket = total;
    g_move_table_plan_errors.fetch_add(bad);
}

void run_place(MoveTableArgs *a)
{
    if (a->hdr->first_bad == kTableNoBad)
        for (uint64_t i = 0; i < a->n; ++i) {
            const MoveTablePlan &P = a->plan[i];
            const uint8_t *in = a->scratch + i * kMoveTableScratch;
            std::copy(in, in + P.head_n, P.dst_origin + P.lead - P.head_n);
            std::copy(in + 16, in + 16 + P.tail_n, P.dst_origin + P.end);
        }
}
} // namespace

uint32_t modgpu_rekey_move_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_rekey_move_table_block() { return 1024u; }
const char *modgpu_rekey_move_table_kernel_name() { return "shim rekey move table"; }
hipError_t modgpu_launch_rekey_move_table_plan(const MoveTableArgs &a, hipStream_t stream) { return enqueue<MoveTableArgs, run_plan, g_move_table_launches, 0>(a, stream); }
hipError_t modgpu_launch_rekey_move_table_finish(const MoveTableArgs &a, hipStream_t stream) { return enqueue<MoveTableArgs, run_finish, g_move_table_launches, 1>(a, stream); }
hipError_t modgpu_launch_rekey_move_table_window(const MoveTableArgs &a, hipStream_t stream) { return enqueue<MoveTableArgs, run_window, g_move_table_launches, 2>(a, stream); }
hipError_t modgpu_launch_rekey_move_table_move(const MoveTableArgs &a, uint32_t *grid, hipStream_t stream)
{
    if (*grid > 256u) *grid = 256u; // what the stand-in's device "holds at once"
    if (*grid == 0) *grid = 1;
    return enqueue<MoveTableArgs, run_move, g_move_table_launches, 3>(a, stream);
}
hipError_t modgpu_launch_rekey_move_table_place(const MoveTableArgs &a, hipStream_t stream) { return enqueue<MoveTableArgs, run_place, g_move_table_launches, 4>(a, stream); }

extern "C" unsigned long long modgpu_shim_move_table_launches(int kind) { return count(g_move_table_launches, kind); }
extern "C" unsigned long long modgpu_shim_move_table_plan_errors(void) { return g_move_table_plan_errors.load(); }
