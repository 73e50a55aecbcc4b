// cycle_rekey_move_table_kernel.hip -- a TABLE of rekey entries in device memory moved with memmove rules in one pass over HBM:
// dst_i[j] = SRC0_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j], SRC0 the memory as the call found it; a
// destination may lie on top of any entry's source.  cycle_rekey_move_table_kernel.h has the rule for the tables taken and the five
// launches.  The two-keystream block: cycle_rekey_impl.h; the jump tables and the single-state arithmetic: cycle_kernel_impl.h; both
// included and not changed.  What the table TUs have in common -- an entry on the chunk grid and its six states, the totals, the search
// levels and one level of their descent, a chunk's span, the funnel, mulmod_keep -- is cycle_table_impl.h; the plan launch's scan is this
// TU's own (it carries the last non-empty entry beside the chunk counts).
//
// Built from two shipped kernels, neither changed: the plan, the chunk grid (64 KiB chunks on absolute chunk-aligned DESTINATION
// addresses, a cut first chunk per entry), the 16-ary chunk -> entry levels, the views and the identity keystream as the state 2^31-1
// are the rekey table kernels' (cycle_rekey_table_kernel.hip); the order of a chunk's trip -- loads returned, barrier, flag up, poll,
// barrier, stores -- and the tickets drawn one at a time are the move loop's of cycle_rekey_kernel.hip.
//
// Why a position waits for lower positions only.  Downward table, positions = global chunks in table order: a chunk's
// destination starts at or below its own source, ends at or below its own source's end, and the sources of the chunks rise with the
// position -- inside an entry because the chunks do, across entries because the rule lists the entries by rising source.  A later
// chunk's source therefore starts where this chunk's source ends or above, which is at or above the end of this chunk's destination;
// rounding that start down to a source dword cannot pass the 16-byte aligned destination address paired with it.  Upward: the mirror
// image, walked from the last chunk down.  Positions are tickets only, so whoever holds a position is running, and the lowest
// unfinished position is never blocked -- whether or not the whole grid is resident.
//
// A table whose entries slide BOTH ways (modgpu_rekey_relayout_table_device) is two such tables interleaved: under the
// order rule a downward or stationary entry and an upward one never meet, destination on source.  The call runs the five launches
// twice; `sweep` in the arguments makes the plan kernel lay the entries of the other direction as empty ones and the finish kernel drop
// the direction clause and decide on unfiltered chunk counts.  The window, move and place kernels do not know of it.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_impl.h"
#include "cycle_table_impl.h"
#include "cycle_rekey_move_table_kernel.h"

namespace {

constexpr uint32_t kNone = ~0u;
constexpr uint32_t kWindowBlock = 256;

__device__ __forceinline__ uint64_t at(const void *p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }

} // namespace

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_move_table_plan(MoveTableArgs a)
{
    __shared__ uint64_t sc[kTableBlock];
    __shared__ uint32_t sl[kTableBlock];
    __shared__ uint32_t sbad, sdown, sup;
    __shared__ unsigned long long sall; // a relayout sweep: the record's chunk count with no entry filtered
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + tid;
    // sweep 1 of a relayout call keeps the stalled word of sweep 0 (no thread of this launch writes it then), and behind a stalled
    // sweep 0 it filters every entry: no chunks, nothing placed
    const bool halted = a.sweep == kRelayoutSweepUp && a.hdr->stalled != 0;
    if (blockIdx.x == 0 && tid == 0) {
        a.hdr->ticket = 0;
        if (a.sweep != kRelayoutSweepUp) a.hdr->stalled = 0;
        a.hdr->first_bad = kTableNoBad;
        a.hdr->total = 0;
        a.hdr->up = 0;
    }
    for (uint64_t k = i; k < a.cap; k += (uint64_t)gridDim.x * kTableBlock) a.flags[k] = 0;
    if (tid == 0) {
        sbad = 0;
        sdown = kNone;
        sup = kNone;
        sall = 0;
    }
    uint64_t cnt = 0, all = 0;
    uint32_t bad = 0, full = 0, way = 0; // way: 1 dst < src, 2 dst > src
    if (i < a.n) {
        const RekeyTableEntry E = a.entries[i];
        TableGrid g = table_grid(E, E.flags | E.reserved);
        bad = g.bad;
        full = E.n != 0 ? 1u : 0u;
        way = !full ? 0u : at(E.dst) < at(E.src) ? 1u : at(E.dst) > at(E.src) ? 2u : 0u;
        all = g.cnt;
        // a relayout sweep filters the entries of the other direction: laid as an empty entry, whose refusal, links and unfiltered
        // chunk count stay what they are
        if (a.sweep != 0 && (halted || (way == 2) != (a.sweep == kRelayoutSweepUp))) {
            g.head = g.words = g.tail = 0;
            g.end = g.lead;
            g.cnt = 0;
        }
        cnt = g.cnt;
        MoveTablePlan P;
        RekeyTableEdge X;
        rekey_table_plan_entry(P, X, E, g);
        P.prev = 0;
        a.plan[i] = P;
        a.edge[i] = X;
    }
    sc[tid] = cnt;
    sl[tid] = full ? tid + 1 : 0;
    __syncthreads();
    if (bad) atomicOr(&sbad, 1u);
    if (way == 1) atomicMin(&sdown, (uint32_t)i);
    if (way == 2) atomicMin(&sup, (uint32_t)i);
    if (a.sweep != 0 && all) atomicAdd(&sall, (unsigned long long)all);
    // inclusive scans over the 1024 entries (Hillis-Steele; every thread reaches every barrier): the sum of the chunk counts, and the
    // last non-empty entry at or before each
    for (uint32_t s = 1; s < kTableBlock; s <<= 1) {
        const uint64_t v = tid >= s ? sc[tid - s] : 0;
        const uint32_t l = tid >= s ? sl[tid - s] : 0;
        __syncthreads();
        sc[tid] += v;
        sl[tid] = sl[tid] > l ? sl[tid] : l;
        __syncthreads();
    }
    if (i < a.n) {
        a.plan[i].start = sc[tid] - cnt;
        a.plan[i].prev = tid ? sl[tid - 1] : 0;
    }
    if (tid == kTableBlock - 1) {
        MoveTableBlk B;
        B.chunks = sc[tid];
        B.bad = sbad;
        B.last = sl[tid] ? blockIdx.x * kTableBlock + sl[tid] : 0;
        B.first_down = sdown;
        B.first_up = sup;
        B.pad[0] = (uint32_t)sall;
        B.pad[1] = (uint32_t)(sall >> 32);
        a.blk[blockIdx.x] = B;
    }
}

// ---- finish: global starts, the direction, the order rule, the status, the search levels, the ragged ends into scratch ----------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_move_table_finish(MoveTableArgs a)
{
    __shared__ uint32_t sprev, sdown, sup;
    // a relayout sweep decides on UNFILTERED chunk counts, so that both sweeps reach one verdict: those of the records before this
    // workgroup's and of all records, and this workgroup's own entries' (read only when the call is refused, to name the entry)
    __shared__ unsigned long long sall_before, sall_total;
    __shared__ uint64_t sa[kTableBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t i = (uint64_t)b * kTableBlock + tid;
    if (tid == 0) {
        sprev = 0;
        sdown = kNone;
        sup = kNone;
        sall_before = 0;
        sall_total = 0;
    }
    if (a.sweep != 0) {
        uint64_t all = 0;
        if (i < a.n) {
            const RekeyTableEntry E = a.entries[i];
            all = table_grid(E, E.flags | E.reserved).cnt;
        }
        sa[tid] = all; // (table_totals' barriers stand between this store and the reads below)
    }
    // beside the totals: the last non-empty entry before this workgroup's, and the first entry that moves down / up
    uint32_t prev = 0, down = kNone, up = kNone;
    unsigned long long all_before = 0, all_total = 0;
    const TableTotals T = table_totals(
        a.blk, a.n_blk, b, tid,
        [&](uint32_t k, const MoveTableBlk &B) {
            if (k < b && B.last > prev) prev = B.last;
            down = B.first_down < down ? B.first_down : down;
            up = B.first_up < up ? B.first_up : up;
            const unsigned long long all = (unsigned long long)B.pad[0] | (unsigned long long)B.pad[1] << 32;
            all_total += all;
            all_before += k < b ? all : 0;
        },
        [&] {
            if (prev) atomicMax(&sprev, prev);
            if (down != kNone) atomicMin(&sdown, down);
            if (up != kNone) atomicMin(&sup, up);
            if (all_total) atomicAdd(&sall_total, all_total);
            if (all_before) atomicAdd(&sall_before, all_before);
        });
    const uint64_t room = a.cap < kTableMaxChunks ? a.cap : kTableMaxChunks;
    const bool ok = T.bad == 0 && (a.sweep != 0 ? (uint64_t)sall_total : T.total) <= room;
    // the first entry with dst != src says which way the table slides; a relayout sweep says it itself
    const bool upward = a.sweep != 0 ? a.sweep == kRelayoutSweepUp : sup < sdown;
    if (b == 0 && tid == 0) {
        a.hdr->total = ok ? T.total : 0;
        a.hdr->up = upward ? 1u : 0u;
    }
    if (i < a.n) {
        const MoveTablePlan P = a.plan[i];
        const uint64_t start = T.before + P.start;
        // refused by the plan, or the first whose chunks pass what the workspace was sized for -- in a relayout sweep, counted with no
        // entry filtered
        uint64_t upto = start + P.chunks;
        if (a.sweep != 0 && !ok) {
            upto = sall_before;
            for (uint32_t t = 0; t <= tid; ++t) upto += sa[t];
        }
        if (!ok && (P.bad || upto > room)) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        // the direction and order rule: this entry against the non-empty entry before it
        const RekeyTableEntry E = a.entries[i];
        if (E.n != 0 && !P.bad) {
            const uint64_t d = at(E.dst), s = at(E.src);
            bool breaks = a.sweep != 0 ? false : upward ? d < s : d > s; // (a relayout has no direction clause)
            const uint64_t q = P.prev ? (uint64_t)b * kTableBlock + P.prev - 1 : sprev ? (uint64_t)sprev - 1 : kTableNoBad;
            if (q != kTableNoBad) {
                const RekeyTableEntry Q = a.entries[q];
                breaks = breaks || s < at(Q.src) || s - at(Q.src) < Q.n || d < at(Q.dst) || d - at(Q.dst) < Q.n;
            }
            if (breaks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        }
        if (ok) {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k) table_set_level(a.level[k], k, a.top, i, start);
            // the < 16 bytes in front of the body and behind it under both keystreams, into scratch: nothing outside the workspace
            // has been written yet, so these are bytes of SRC0 whatever the later launches store on top of them
            const RekeyTableEdge X = a.edge[i];
            const uint8_t *sb = P.src_origin + P.lead;
            uint8_t *out = a.scratch + i * kMoveTableScratch;
            const uint64_t body = P.end - P.lead;
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                const uint32_t y = c_pow_b0.v[j];
                if (j < P.head_n) out[j] = rekey_byte(sb[(int64_t)j - P.head_n], mulmod_keep(X.head[0], y), mulmod_keep(X.head[1], y));
                if (j < P.tail_n) out[16 + j] = rekey_byte(sb[body + j], mulmod_keep(X.tail[0], y), mulmod_keep(X.tail[1], y));
            }
        }
    }
    if (ok && b == 0 && tid < 16)
        for (uint32_t k = 0; k < kTableLevels; ++k) table_pad_level(a.level[k], a.level_n[k], k, a.top, tid);
}

// ---- window: one thread per chunk ------------------------------------------------------------------------------------------------
namespace {
// destination and source of global chunk g, the source rounded out to whole source dwords
struct ChunkSpan {
    uint64_t d0, d1, s0, s1;
};
__device__ ChunkSpan chunk_span(const MoveTableArgs &a, uint32_t g)
{
    uint32_t j = 0;
    for (int k = (int)a.top; k >= 0; --k) j = table_descend(a.level[k], j, g);
    const MoveTablePlan P = a.plan[j];
    const uint64_t c = g - P.start, off = c * kChunk, cut = c ? 0 : P.lead;
    const uint64_t lim = P.end < off + kChunk ? P.end : off + kChunk;
    ChunkSpan s;
    s.d0 = at(P.dst_origin) + off + cut;
    s.d1 = at(P.dst_origin) + lim;
    s.s0 = (at(P.src_origin) + off + cut) & ~3ull;
    s.s1 = (at(P.src_origin) + lim + 3) & ~3ull;
    return s;
}
} // namespace

__global__ __launch_bounds__(kWindowBlock) void modgpu_cycle_rekey_move_table_window(MoveTableArgs a)
{
    if (a.hdr->first_bad != kTableNoBad) return;
    const uint64_t total = a.hdr->total;
    const uint64_t g64 = (uint64_t)blockIdx.x * kWindowBlock + threadIdx.x;
    if (g64 >= total) return;
    const uint32_t g = (uint32_t)g64;
    const bool up = a.hdr->up != 0;
    const ChunkSpan me = chunk_span(a, g);
    // the chunks on the side the table walks away from, this one included: their sources rise with the index
    const uint32_t A = up ? g : 0u, B = up ? (uint32_t)total : g + 1u;
    // lo: the first whose source ends above this destination's start; hi: the first whose source starts at or above its end
    uint32_t lo = A, n = B - A;
    while (n) {
        const uint32_t h = n / 2;
        if (chunk_span(a, lo + h).s1 <= me.d0) {
            lo += h + 1;
            n -= h + 1;
        } else {
            n = h;
        }
    }
    uint32_t hi = lo;
    n = B - lo;
    while (n) {
        const uint32_t h = n / 2;
        if (chunk_span(a, hi + h).s0 < me.d1) {
            hi += h + 1;
            n -= h + 1;
        } else {
            n = h;
        }
    }
    // without the chunk itself, and never a higher position: lower ones below g in a downward table, above g in an upward one
    if (up) lo = lo > g + 1u ? lo : g + 1u;
    else hi = hi < g ? hi : g;
    MoveTableWin w;
    w.lo = lo;
    w.n = hi > lo ? hi - lo : 0u;
    a.win[g] = w;
}

// ---- move ------------------------------------------------------------------------------------------------------------------------
template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) MODGPU_REKEY_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_rekey_move_table_kernel(MoveTableArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr int SAUX = AUX_SC1 | AUX_NT;
    constexpr int DEPTH = 1;
    constexpr uint32_t CHUNK = (uint32_t)U * BLOCK * lcg::WORD;
    static_assert(CHUNK == kChunk, "the plan lays entries on this chunk grid");
    constexpr uint32_t SUB = BLOCK * lcg::WORD;
    constexpr int NB = DEPTH + 1;
    const uint32_t tid = threadIdx.x;
    // 0 when the call was refused: nothing is loaded, flagged or stored
    const uint32_t total = *as_const(&a.hdr->first_bad) == kTableNoBad ? (uint32_t)*as_const(&a.hdr->total) : 0u;
    const uint32_t up = *as_const(&a.hdr->up);
    __shared__ uint32_t q_next[2]; // ticket mailbox, two words used alternately
    __shared__ uint32_t q_dead;    // the wait ran out: this workgroup stores nothing more (it still loads, flags and draws tickets)
    uint32_t trip = 0;
    const uint32_t voff = tid * lcg::WORD;
    const uint32_t lane_mul = mulmod_canon(c_tile_lo.v[tid >> 8], c_lane_pow.v[tid & 255]);

    struct View {
        uint8_t *dst0;       // the entry's chunk origin
        const uint8_t *src0; // the source byte that pairs with it
        uint64_t end;
        uint32_t lead, lo;     // global chunk lo is the entry's chunk 0
        uint32_t lane_base[2]; // per lane: both keystreams' states of this lane's word 0 in the entry's chunk 0
    };
    // (an entry the search finds has a body, so its chunk count is that of `end`; the empty view's is 0.  One scalar register less per
    // view than keeping the count: the kernel sits at its scalar budget)
    auto in = [](uint32_t g, const View &v) { return g - v.lo < (uint32_t)((v.end + CHUNK - 1) / CHUNK); };
    // the entry of chunk g < total: the last entry whose start is <= g, by a 16-ary descent of the levels
    auto search = [&](uint32_t g, View &v) {
        uint32_t j = 0;
#pragma unroll 1
        for (int k = (int)a.top; k >= 0; --k) j = table_descend(a.level[k], j, g);
        const MoveTablePlan P = *as_const(a.plan + j);
        v.dst0 = P.dst_origin;
        v.src0 = P.src_origin;
        v.end = P.end;
        v.lead = P.lead;
        v.lo = (uint32_t)P.start;
        v.lane_base[0] = mulmod_keep(P.base_from, lane_mul);
        v.lane_base[1] = mulmod_keep(P.base_to, lane_mul);
    };
    auto span = [&](uint32_t g, const View &v) { return table_span<CHUNK>(g, total, v); };
    View vb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vb[i] = View{nullptr, nullptr, 0, 0, 0, {lcg::M, lcg::M}};
    // the phase of chunk g's source in its dword: not 0 = its loads take the funnel's extra dwords
    auto phase = [&](uint32_t g, const View &v) {
        const Span s = span(g, v);
        return (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
    };
    auto load = [&](Raw(&w)[U], View &v, const View &prev, uint32_t g) {
        if (g < total && !in(g, v)) {
            if (in(g, prev)) v = prev;
            else search(g, v);
        }
        const Span s = span(g, v);
        const uint8_t *p = v.src0 + s.off + s.cut;
        const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
        // the extra dword of the last word is the aligned dword that holds the body's last source byte: num_records grows by 4
        const auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p - sh), 0, (int)(s.bytes + (sh && s.bytes ? 4u : 0u)), 0x00020000);
#pragma unroll
        for (int u = 0; u < U; ++u) w[u].d = __builtin_amdgcn_raw_buffer_load_b128(r, voff + u * SUB - s.cut, 0, AUX_NT);
        if (sh) {
#pragma unroll
            for (int u = 0; u < U; ++u) w[u].e = __builtin_amdgcn_raw_buffer_load_b32(r, voff + u * SUB - s.cut + lcg::WORD, 0, AUX_NT);
        }
    };
    uint32_t pending = 0;
    const uint32_t q_next_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_next[0];
    const uint32_t q_dead_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_dead;
    const uint32_t one = 1u;
    auto chunk_at = [&](uint32_t p) { return up != 0 && p < total ? total - 1u - p : p; };
    auto flag_up = [&](const uint32_t *f) { // thread 0; false: gave up
        if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
        const uint32_t t0 = (uint32_t)wall_clock64(); // (the bound fits 32 bits: the low word's difference is enough)
        do {
            __builtin_amdgcn_s_sleep(8);
            if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
        } while ((uint32_t)wall_clock64() - t0 < (uint32_t)kMoveTableStallTicks);
        return false;
    };
    // chunk g; gn in view vn is the NEXT chunk, whose loads are in flight behind this one's
    auto process_move = [&](Raw(&w)[U], const View &v, uint32_t g, const View &vn, uint32_t gn) {
        // the chunks this one waits for: a scalar load (the window launch wrote it: constant while this launch runs) that returns
        // while the blocks below run
        MoveTableWin wn{0, 0};
        if (g < total) wn = *as_const(a.win + g);
        const uint32_t next_fun = phase(gn, vn);
        const Span s = span(g, v);
        const uint32_t sh = (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
        auto r = __builtin_amdgcn_make_buffer_rsrc(v.dst0 + s.off + s.cut, 0, (int)s.bytes, 0x00020000);
        const uint32_t c = g - v.lo;
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        uint32_t sa = mulmod_keep(v.lane_base[0], p), sb = mulmod_keep(v.lane_base[1], p);
        u32x4 d[U];
        if (sh) {
#pragma unroll
            for (int u = 0; u < U; ++u) d[u] = funnel(w[u], sh);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) d[u] = w[u].d;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            d[u] = rekey_word(d[u], sa, sb);
            sa = mulmod_keep(sa, lcg::kTileLo.v[BLOCK / 256]);
            sb = mulmod_keep(sb, lcg::kTileLo.v[BLOCK / 256]);
        }
        // every wave waits HERE until this chunk's loads have returned: the only vector-memory instructions younger than them are the
        // next chunk's loads (U, twice that when it took the funnel).  The blocks above consumed the data, so the compiler's own waits
        // say the same; this one does not depend on where an optimiser leaves them (check_isa.py pins it in front of the barrier).
        if (next_fun) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * U) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" : : "n"(U) : "memory");
        if (tid == 0)
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * (trip & 1u)), "v"(pending) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier(); // every wave has this chunk's source in registers
        if (tid == 0 && g < total) {
            __hip_atomic_store(a.flags + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t dead;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(dead) : "v"(q_dead_lds) : "memory");
#pragma unroll 1
            for (uint32_t i = 0; i < wn.n && dead == 0; ++i) {
                if (!flag_up(a.flags + wn.lo + i)) {
                    atomicCAS(&a.hdr->stalled, 0u, 1u + g);
                    dead = 1;
                    asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_dead_lds), "v"(dead) : "memory");
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        uint32_t dd;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(dd) : "v"(q_dead_lds) : "memory");
        if (__builtin_amdgcn_readfirstlane((int)dd) == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB - s.cut, 0, SAUX);
        }
        ++trip;
    };
    auto take_published = [&]() {
        uint32_t t;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * ((trip - 1u) & 1u)) : "memory");
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)t); // tickets ARE positions
    };

    // the first DEPTH + 1 positions: one fetch EACH, a barrier apart, so that no workgroup starts with two consecutive positions
    // (cycle_rekey_kernel.hip's move loop says why)
    uint32_t cq[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        if (tid == 0) {
            pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %2, %3\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * ((uint32_t)(i + 1) & 1u)), "v"(pending), "v"(q_dead_lds), "v"(0u) : "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        uint32_t t;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * ((uint32_t)(i + 1) & 1u)) : "memory");
        cq[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    }
    if (cq[0] < total) {
        Raw w[NB][U];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) load(w[i], vb[i], vb[(i + NB - 1) % NB], chunk_at(cq[i]));
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                const int q = (p + DEPTH) % NB;
                __builtin_amdgcn_s_barrier();
                if (tid == 0) pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                load(w[q], vb[q], vb[p], chunk_at(cq[DEPTH]));
                __builtin_amdgcn_sched_barrier(0);
                process_move(w[p], vb[p], chunk_at(cq[0]), vb[q], chunk_at(cq[DEPTH]));
#pragma unroll
                for (int i = 0; i < DEPTH; ++i) cq[i] = cq[i + 1];
                cq[DEPTH] = take_published();
                if (cq[0] >= total) {
                    finished = true;
                    break;
                }
            }
        }
    }
}

// ---- place: the ragged ends from scratch into place ------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_move_table_place(MoveTableArgs a)
{
    if (a.hdr->first_bad != kTableNoBad) return;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + threadIdx.x;
    if (i >= a.n) return;
    const MoveTablePlan P = a.plan[i];
    const uint8_t *in = a.scratch + i * kMoveTableScratch;
    uint8_t *db = P.dst_origin + P.lead;
    const uint64_t body = P.end - P.lead;
#pragma unroll
    for (uint32_t j = 0; j < 15; ++j) {
        if (j < P.head_n) db[(int64_t)j - P.head_n] = in[j];
        if (j < P.tail_n) db[body + j] = in[16 + j];
    }
}

namespace {
template <int U, int BLOCK> struct MoveTableShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const MoveTableArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_rekey_move_table_kernel<U, BLOCK>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() { return table_kernel_name<U, BLOCK>("modgpu_cycle_rekey_move_table_kernel"); }
};
using MoveTableMove = MoveTableShape<4, 1024>; // the rekey kernel's shape: 64 KiB chunks
static_assert(MoveTableMove::chunk == kChunk, "one chunk size for the plan and the move");
} // namespace

uint32_t modgpu_rekey_move_table_chunk_bytes() { return MoveTableMove::chunk; }
uint32_t modgpu_rekey_move_table_block() { return MoveTableMove::block; }
const char *modgpu_rekey_move_table_kernel_name() { return MoveTableMove::name(); }
hipError_t modgpu_launch_rekey_move_table_plan(const MoveTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_move_table_plan, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_move_table_finish(const MoveTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_move_table_finish, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_relayout_plan(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream)
{
    MoveTableArgs s = a;
    s.sweep = sweep;
    hipLaunchKernelGGL(modgpu_cycle_rekey_move_table_plan, dim3(s.n_blk), dim3(kTableBlock), 0, stream, s);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_relayout_finish(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream)
{
    MoveTableArgs s = a;
    s.sweep = sweep;
    hipLaunchKernelGGL(modgpu_cycle_rekey_move_table_finish, dim3(s.n_blk), dim3(kTableBlock), 0, stream, s);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_move_table_window(const MoveTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_move_table_window, dim3((uint32_t)((a.cap + kWindowBlock - 1) / kWindowBlock)), dim3(kWindowBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_move_table_move(const MoveTableArgs &a, uint32_t *grid, hipStream_t stream)
{
    int per_cu = 0, cus = 0, dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, modgpu_cycle_rekey_move_table_kernel<4, 1024>, 1024, 0);
    if (e != hipSuccess) return e;
    const uint64_t resident = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(cus > 0 ? cus : 1);
    if (*grid > resident) *grid = (uint32_t)resident;
    if (*grid == 0) *grid = 1;
    MoveTableMove::launch(a, *grid, stream);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_move_table_place(const MoveTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_move_table_place, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
