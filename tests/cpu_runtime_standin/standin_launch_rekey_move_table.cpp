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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../../modulate_amd/csrc/cycle_rekey_move_table_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_move_table_launches[5] = {}, g_move_table_plan_errors{0};
constexpr uint64_t kChunk = 65536;
constexpr uint32_t kNone = ~0u;

uint32_t state(uint32_t k, uint64_t e) { return k ? lcg::mulmod(k, lcg::powmod(lcg::A, e % lcg::PERIOD)) : lcg::M; }
uint32_t step(uint32_t s, uint64_t j) { return s == lcg::M ? s : lcg::mulmod(s, lcg::powmod(lcg::A, j % lcg::PERIOD)); }
uint64_t at(const void *p) { return reinterpret_cast<uintptr_t>(p); }

void run_plan(void *arg)
{
    MoveTableArgs *a = static_cast<MoveTableArgs *>(arg);
    a->hdr->ticket = 0;
    a->hdr->stalled = 0;
    a->hdr->first_bad = kTableNoBad;
    a->hdr->total = 0;
    a->hdr->up = 0;
    for (uint64_t k = 0; k < a->cap; ++k) a->flags[k] = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        uint64_t run = 0;
        MoveTableBlk B{0, 0, 0, kNone, kNone, {0, 0}};
        uint32_t prev = 0;
        for (uint64_t i = (uint64_t)b * kTableBlock; i < a->n && i < (uint64_t)(b + 1) * kTableBlock; ++i) {
            const RekeyTableEntry E = a->entries[i];
            const uint64_t d = at(E.dst);
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
            MoveTablePlan &P = a->plan[i];
            P.dst_origin = reinterpret_cast<uint8_t *>(d + head - lead); // (as integers: a refused entry's pointer may be NULL)
            P.src_origin = reinterpret_cast<const uint8_t *>(at(E.src) + head - lead);
            P.end = end;
            P.start = run;
            P.lead = lead;
            P.chunks = (uint32_t)cnt;
            P.base_from = state(kf, of + body);
            P.base_to = state(kt, ot + body);
            P.bad = bad;
            P.head_n = (uint32_t)head;
            P.tail_n = (uint32_t)(E.n - head - words * 16);
            P.prev = prev;
            RekeyTableEdge &X = a->edge[i];
            X.head[0] = state(kf, of);
            X.head[1] = state(kt, ot);
            X.tail[0] = state(kf, of + after);
            X.tail[1] = state(kt, ot + after);
            run += cnt;
            B.bad |= bad;
            if (E.n) {
                prev = (uint32_t)(i - (uint64_t)b * kTableBlock) + 1;
                B.last = (uint32_t)i + 1;
                if (at(E.dst) < at(E.src) && B.first_down == kNone) B.first_down = (uint32_t)i;
                if (at(E.dst) > at(E.src) && B.first_up == kNone) B.first_up = (uint32_t)i;
            }
        }
        B.chunks = run;
        a->blk[b] = B;
    }
    g_move_table_launches[0].fetch_add(1);
    delete a;
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

void run_finish(void *arg)
{
    MoveTableArgs *a = static_cast<MoveTableArgs *>(arg);
    uint64_t total = 0;
    uint32_t bad = 0, down = kNone, up = kNone;
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        total += a->blk[b].chunks;
        bad |= a->blk[b].bad;
        down = std::min(down, a->blk[b].first_down);
        up = std::min(up, a->blk[b].first_up);
    }
    const uint64_t room = std::min<uint64_t>(a->cap, kTableMaxChunks);
    const bool ok = !bad && total <= room;
    const bool upward = up < down;
    a->hdr->total = ok ? total : 0;
    a->hdr->up = upward ? 1u : 0u;
    uint64_t before = 0;
    uint32_t last = 0; // 1 + the last non-empty entry of the earlier records
    auto refuse = [&](uint64_t i) { a->hdr->first_bad = std::min<uint64_t>(a->hdr->first_bad, i); };
    for (uint32_t b = 0; b < a->n_blk; ++b) {
        for (uint64_t i = (uint64_t)b * kTableBlock; i < a->n && i < (uint64_t)(b + 1) * kTableBlock; ++i) {
            MoveTablePlan &P = a->plan[i];
            const uint64_t start = before + P.start;
            if (!ok && (P.bad || start + P.chunks > room)) refuse(i);
            const RekeyTableEntry E = a->entries[i];
            if (E.n != 0 && !P.bad) {
                const uint64_t d = at(E.dst), s = at(E.src);
                bool breaks = upward ? d < s : d > s;
                const uint64_t q = P.prev ? (uint64_t)b * kTableBlock + P.prev - 1 : last ? (uint64_t)last - 1 : kTableNoBad;
                if (q != kTableNoBad) {
                    const RekeyTableEntry Q = a->entries[q];
                    breaks = breaks || s < at(Q.src) || s - at(Q.src) < Q.n || d < at(Q.dst) || d - at(Q.dst) < Q.n;
                }
                if (breaks) refuse(i);
            }
            if (!ok) continue;
            P.start = start;
            for (uint32_t k = 0; k <= a->top; ++k)
                if ((i & ((1ull << (4 * k)) - 1)) == 0) a->level[k][i >> (4 * k)] = (uint32_t)start;
            const RekeyTableEdge &X = a->edge[i];
            uint8_t *out = a->scratch + i * kMoveTableScratch;
            span_rekey(out, P.src_origin + P.lead - P.head_n, 0, P.head_n, X.head[0], X.head[1]);
            span_rekey(out + 16, P.src_origin + P.end, 0, P.tail_n, X.tail[0], X.tail[1]);
        }
        before += a->blk[b].chunks;
        if (a->blk[b].last) last = a->blk[b].last;
    }
    if (ok)
        for (uint32_t k = 0; k <= a->top; ++k)
            for (uint64_t j = a->level_n[k]; j < ((a->level_n[k] + 15) & ~15ull); ++j) a->level[k][j] = ~0u;
    g_move_table_launches[1].fetch_add(1);
    delete a;
}

struct Span {
    const MoveTablePlan *P;
    uint64_t off, cut, lim; // the chunk is [off + cut, lim) from the entry's origin
};
Span chunk_span(const MoveTableArgs &a, uint32_t g)
{
    uint64_t j = 0;
    for (int k = (int)a.top; k >= 0; --k) { // the kernel's descent: 16 keys per level
        uint32_t c = 0;
        for (int t = 0; t < 16; ++t) c += a.level[k][16 * j + t] <= g ? 1u : 0u;
        j = 16 * j + c - 1;
    }
    const MoveTablePlan &P = a.plan[j];
    const uint64_t c = g - P.start, off = c * kChunk;
    return {&P, off, c ? 0 : (uint64_t)P.lead, std::min<uint64_t>(P.end, off + kChunk)};
}

void run_window(void *arg)
{
    MoveTableArgs *a = static_cast<MoveTableArgs *>(arg);
    if (a->hdr->first_bad == kTableNoBad) {
        const uint32_t total = (uint32_t)a->hdr->total;
        const bool up = a->hdr->up != 0;
        std::vector<uint64_t> s0(total), s1(total), d0(total), d1(total);
        for (uint32_t g = 0; g < total; ++g) {
            const Span s = chunk_span(*a, g);
            d0[g] = at(s.P->dst_origin) + s.off + s.cut;
            d1[g] = at(s.P->dst_origin) + s.lim;
            s0[g] = (at(s.P->src_origin) + s.off + s.cut) & ~3ull;
            s1[g] = (at(s.P->src_origin) + s.lim + 3) & ~3ull;
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
    g_move_table_launches[2].fetch_add(1);
    delete a;
}

void run_move(void *arg)
{
    MoveTableArgs *a = static_cast<MoveTableArgs *>(arg);
    unsigned long long bad = 0;
    const uint32_t total = a->hdr->first_bad == kTableNoBad ? (uint32_t)a->hdr->total : 0;
    const bool up = a->hdr->up != 0;
    std::vector<uint8_t> buf(kChunk);
    for (uint32_t p = 0; p < total; ++p) {
        const uint32_t g = up ? total - 1 - p : p;
        const Span s = chunk_span(*a, g);
        const uint64_t len = s.lim - s.off - s.cut;
        span_rekey(buf.data(), s.P->src_origin, s.off + s.cut, len, s.P->base_from, s.P->base_to);
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
            const uint64_t o0 = at(o.P->src_origin) + o.off + o.cut, o1 = at(o.P->src_origin) + o.lim;
            const uint64_t d0 = at(s.P->dst_origin) + s.off + s.cut, d1 = at(s.P->dst_origin) + s.lim;
            if (o0 < d1 && o1 > d0) bad += !(k - w.lo < w.n);
        }
        std::copy(buf.begin(), buf.begin() + (ptrdiff_t)len, s.P->dst_origin + s.off + s.cut);
    }
    a->hdr->ticket = total;
    g_move_table_plan_errors.fetch_add(bad);
    g_move_table_launches[3].fetch_add(1);
    delete a;
}

void run_place(void *arg)
{
    MoveTableArgs *a = static_cast<MoveTableArgs *>(arg);
    if (a->hdr->first_bad == kTableNoBad)
        for (uint64_t i = 0; i < a->n; ++i) {
            const MoveTablePlan &P = a->plan[i];
            const uint8_t *in = a->scratch + i * kMoveTableScratch;
            std::copy(in, in + P.head_n, P.dst_origin + P.lead - P.head_n);
            std::copy(in + 16, in + 16 + P.tail_n, P.dst_origin + P.end);
        }
    g_move_table_launches[4].fetch_add(1);
    delete a;
}
} // namespace

uint32_t modgpu_rekey_move_table_chunk_bytes() { return (uint32_t)kChunk; }
uint32_t modgpu_rekey_move_table_block() { return 1024u; }
const char *modgpu_rekey_move_table_kernel_name() { return "shim rekey move table"; }
hipError_t modgpu_launch_rekey_move_table_plan(const MoveTableArgs &a, hipStream_t stream)
{
    shim::enqueue(stream, run_plan, new MoveTableArgs(a));
    return hipSuccess;
}
hipError_t modgpu_launch_rekey_move_table_finish(const MoveTableArgs &a, hipStream_t stream)
{
    shim::enqueue(stream, run_finish, new MoveTableArgs(a));
    return hipSuccess;
}
hipError_t modgpu_launch_rekey_move_table_window(const MoveTableArgs &a, hipStream_t stream)
{
    shim::enqueue(stream, run_window, new MoveTableArgs(a));
    return hipSuccess;
}
hipError_t modgpu_launch_rekey_move_table_move(const MoveTableArgs &a, uint32_t *grid, hipStream_t stream)
{
    if (*grid > 256u) *grid = 256u; // what the stand-in's device "holds at once"
    if (*grid == 0) *grid = 1;
    shim::enqueue(stream, run_move, new MoveTableArgs(a));
    return hipSuccess;
}
hipError_t modgpu_launch_rekey_move_table_place(const MoveTableArgs &a, hipStream_t stream)
{
    shim::enqueue(stream, run_place, new MoveTableArgs(a));
    return hipSuccess;
}

extern "C" unsigned long long modgpu_shim_move_table_launches(int kind) { return kind >= 0 && kind < 5 ? g_move_table_launches[kind].load() : 0; }
extern "C" unsigned long long modgpu_shim_move_table_plan_errors(void) { return g_move_table_plan_errors.load(); }
