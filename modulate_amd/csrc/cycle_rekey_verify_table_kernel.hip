// cycle_rekey_verify_table_kernel.hip -- a TABLE of rekey entries that lives in device memory, any number of them, VERIFIED in three
// launches: result_i = { #{ j : dst_i[j] != (src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j]) }, the lowest such
// j, n_i, 0 }, dst being the comparand.  Both sides are read once; nothing is written but the results and the workspace.  The
// two-keystream block: cycle_rekey_impl.h; the jump tables and the single-state arithmetic: cycle_kernel_impl.h; both included and not
// changed (this TU has a hash of its own).
//
// Three parents, joined; what they have in common -- an entry on the chunk grid and its six states, the scan, the totals, the search
// levels and one level of their descent, a chunk's span, the funnel, mulmod_keep, a lane's findings -- is
// cycle_table_impl.h, shared by the table TUs:
//   plan    the rekey table call's (cycle_rekey_table_kernel.hip): one thread per entry reads the entry where the caller left it (when
//           the launch RUNS), checks it (a NULL pointer with bytes to compare, nonzero flags or reserved, a body beyond the chunk jump
//           tables), lays it on the chunk grid of its COMPARAND, computes SIX base states -- head, body and tail for each keystream --
//           and scans the chunk counts of its 1024 entries in LDS.  Workgroup 0 resets the ticket, the status and the summary: every
//           call, and every replay of a captured one, starts clean in stream order.
//   finish  the rekey table call's prefix and levels with the verify table call's role (cycle_verify_table_kernel.hip): the call is
//           refused whole on any bad entry (no result is written, the lowest bad index goes to the status), else the < 16 ragged bytes
//           at each end are COMPARED bytewise under both keystreams and the thread stores its entry's result whole -- {edge mismatches,
//           lowest edge index or none, n, 0} -- so nothing needs clearing beforehand; an entry with dirty edges goes to the summary.
//   stream  the verify table call's: persistent 1024-thread workgroups on 64 KiB chunks of absolute chunk-aligned COMPARAND addresses
//           handed out by the workspace's ticket counter with a static prefix of two, nt loads of both sides, the v_alignbyte_b32
//           funnel on every chunk, a chunk's entry found by the 16-ary descent of scalar loads and kept in one of two packed views, the
//           per-wave flush with no LDS and no barrier.  The compare is the rekey verify kernel's (cycle_rekey_verify_kernel.hip):
//           every lane-word carries TWO states stepped from word to word, the chunk's and the lane's jumps shared, and because the
//           two-keystream block owns v[112:127] only the SOURCE is loaded a whole trip ahead (two ping-pong sets); the comparand's
//           words are asked for one by one as the compare frees their registers, one set of 16, and the test on clean data is a
//           ballot per word.
//
// Degenerate keystreams need no case of their own (the rekey table kernel's convention): an identity key's state is kept as 2^31-1,
// whose packed byte is 0xFF and whose keystream byte is 0, and every multiply that derives a state from an entry's base is mulmod_keep,
// which leaves 2^31-1 where it is.  One identity stream leaves the other, two are a plain compare, equal reduced keys at offsets equal
// mod 2^31-2 give equal states that cancel.  Every entry runs on the one stream kernel.
//
// The result protocol is the verify table kernel's: tickets only grow, so a workgroup passes each entry in ONE contiguous run; counts
// and lowest indices stay in registers, per lane, while the entry is unchanged; when it changes, and at the end, every WAVE flushes for
// itself -- nothing found: one ballot and nothing else; else its lane 0 sends one 64-bit add and one 64-bit unsigned min to the
// entry's result and the same pair to the summary.  The stream kernel contains no store of any kind.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_impl.h"
#include "cycle_table_impl.h"
#include "cycle_rekey_verify_table_kernel.h"

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_verify_table_plan(RekeyVerifyTableArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + tid;
    if (blockIdx.x == 0 && tid == 0) {
        a.hdr->ticket = 0;
        a.hdr->first_bad = kTableNoBad;
        a.hdr->total = 0;
        a.sum->mismatches = 0ull;
        a.sum->first_bad_entry = kVerifyNone;
        a.sum->entries = a.n;
        a.sum->reserved = 0ull;
    }
    uint64_t cnt = 0;
    uint32_t bad = 0;
    if (i < a.n) {
        const RekeyTableEntry E = a.entries[i];
        const TableGrid g = table_grid(E, E.flags | E.reserved); // (dst is the comparand: the chunk grid is laid on it)
        cnt = g.cnt;
        bad = g.bad;
        RekeyTablePlan P;
        RekeyTableEdge X;
        rekey_table_plan_entry(P, X, E, g);
        P.pad = 0;
        a.plan[i] = P;
        a.edge[i] = X;
    }
    table_plan_store(a.plan, a.blk, a.n, i, cnt, bad, tid);
}

// ---- finish: global starts, the status, the search levels, the ragged edges compared, every result initialised ---------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_verify_table_finish(RekeyVerifyTableArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t i = (uint64_t)b * kTableBlock + tid;
    const TableTotals T = table_totals(a.blk, a.n_blk, b, tid);
    const bool ok = T.bad == 0 && T.total <= kTableMaxChunks;
    if (b == 0 && tid == 0) a.hdr->total = ok ? T.total : 0;
    if (i < a.n) {
        const RekeyTablePlan P = a.plan[i];
        const uint64_t start = T.before + P.start;
        if (!ok) {
            // refused: no result is written; the lowest bad entry -- a refused one, or the first whose chunks pass the ticket range
            if (P.bad || start + P.chunks > kTableMaxChunks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        } else {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k) table_set_level(a.level[k], k, a.top, i, start);
            // the < 16 bytes in front of the body and behind it, compared bytewise under both keystreams; the index counts from the
            // entry's first byte
            const RekeyTableEdge X = a.edge[i];
            const uint8_t *sb = P.src_origin + P.lead;
            const uint8_t *eb = P.dst_origin + P.lead;
            const uint64_t body = P.end - P.lead;
            unsigned long long cnt = 0ull, first = kVerifyNone;
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                if (j < P.tail_n) {
                    const uint32_t y = c_pow_b0.v[j];
                    if (eb[body + j] != rekey_byte(sb[body + j], mulmod_keep(X.tail[0], y), mulmod_keep(X.tail[1], y))) {
                        ++cnt;
                        const unsigned long long at = (unsigned long long)P.head_n + body + j;
                        first = at < first ? at : first;
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                if (j < P.head_n) {
                    const uint32_t y = c_pow_b0.v[j];
                    if (eb[(int64_t)j - P.head_n] != rekey_byte(sb[(int64_t)j - P.head_n], mulmod_keep(X.head[0], y), mulmod_keep(X.head[1], y))) {
                        ++cnt;
                        first = j < first ? j : first;
                    }
                }
            }
            a.results[i] = CycleVerifyResult{cnt, first, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
            if (cnt != 0ull) {
                __hip_atomic_fetch_add(&a.sum->mismatches, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_min(&a.sum->first_bad_entry, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (ok && b == 0 && tid < 16)
        for (uint32_t k = 0; k < kTableLevels; ++k) table_pad_level(a.level[k], a.level_n[k], k, a.top, tid);
}

// ---- stream ------------------------------------------------------------------------------------------------------------------------
namespace {

// the comparand side of a chunk whose source is already on its way: the descriptor of its bytes and the cut in front of them
struct Late {
    __amdgpu_buffer_rsrc_t re;
    uint32_t cut;
};
} // namespace

template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) MODGPU_REKEY_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_rekey_verify_table_kernel(RekeyVerifyTableArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr int DEPTH = 1;
    constexpr uint32_t CHUNK = (uint32_t)U * BLOCK * lcg::WORD;
    static_assert(CHUNK == kChunk && CHUNK == 65536, "the plan lays entries on this chunk grid; a view packs two offsets in a chunk into 32 bits");
    constexpr uint32_t SUB = BLOCK * lcg::WORD;
    constexpr int NB = DEPTH + 1;
    constexpr int PREFIX = DEPTH + 1;
    const uint32_t tid = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    const uint32_t G = gridDim.x;
    const uint32_t total = (uint32_t)*as_const(&a.hdr->total); // 0 when the finish launch refused the call
    __shared__ uint32_t q_next[2];
    const uint32_t voff = tid * lcg::WORD;
    const uint32_t lane_mul = mulmod_canon(c_tile_lo.v[tid >> 8], c_lane_pow.v[tid & 255]);

    struct View {
        const uint8_t *exp0; // the comparand's chunk origin of the entry
        const uint8_t *src0; // the source byte that pairs with it
        uint32_t lo, hi;    // global chunks [lo, hi) are the entry's chunks 0 .. hi - lo - 1
        uint32_t lead_rem;  // bits 0..15: lead; bits 16..31: bytes of the last chunk, counted from its chunk origin (1 .. CHUNK), less 1
        uint32_t entry;        // bits 0..23: its index in the table (where its result is); bits 24..27: head_n
        uint32_t lane_base[2]; // per lane: both keystreams' states of this lane's word 0 in the entry's chunk 0 (2^31-1: the identity)
    };
    static_assert(kTableMaxEntries <= (1u << 24), "an entry's index and its head_n share a register");
    auto in = [](uint32_t g, const View &v) { return g - v.lo < v.hi - v.lo; };
    // the entry of chunk g < total: the last entry whose start is <= g, by a 16-ary descent of the levels
    auto search = [&](uint32_t g, View &v) {
        uint32_t j = 0;
        int k = (int)a.top;
#pragma unroll 1
        do j = table_descend(a.level[k], j, g); // (level 0 always exists)
        while (--k >= 0);
        const RekeyTablePlan P = *as_const(a.plan + j);
        v.exp0 = P.dst_origin;
        v.src0 = P.src_origin;
        v.lead_rem = table_lead_rem(P);
        v.lo = (uint32_t)P.start;
        v.hi = (uint32_t)P.start + P.chunks;
        v.entry = j | (P.head_n << 24);
        v.lane_base[0] = mulmod_keep(P.base_from, lane_mul);
        v.lane_base[1] = mulmod_keep(P.base_to, lane_mul);
    };
    // where chunk g lies: offset of its chunk from the entry's origin, the cut in front of the body (chunk 0 only), its bytes
    auto span = [&](uint32_t g, const View &v) { return table_span_packed<CHUNK>(g, total, v); };
    View vb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vb[i] = View{nullptr, nullptr, 0, 0, 0, ~0u, {lcg::M, lcg::M}};
    // The load side of a trip: chunk g's SOURCE words go out at once, a whole trip ahead, into the set the compare side is not reading;
    // what comes back is the descriptor of the chunk's comparand, whose words follow one by one as the compare side frees their
    // registers.  `prev` is the view of the chunk loaded before it.
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
        // (lanes in front of a cut first chunk's body wrap past num_records: dropped on both sides, and masked in the compare)
#pragma unroll
        for (int u = 0; u < U; ++u) w[u].d = __builtin_amdgcn_raw_buffer_load_b128(r, voff + u * SUB - s.cut, 0, AUX_NT);
        if (sh) {
#pragma unroll
            for (int u = 0; u < U; ++u) w[u].e = __builtin_amdgcn_raw_buffer_load_b32(r, voff + u * SUB - s.cut + lcg::WORD, 0, AUX_NT);
        }
        return Late{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(v.exp0 + s.off + s.cut), 0, (int)s.bytes, 0x00020000), s.cut};
    };

    // What this lane found in the entry of the chunks compared since the last flush.
    Found f{0u, kVerifyNone};
    // The workgroup leaves an entry (uniform: every wave comes here at the same chunk).  Each wave for itself, with no barrier: nothing
    // found by any lane -- nothing done; else the wave's sum and minimum, and lane 0 sends them on.
    auto flush = [&](uint32_t entry) {
        unsigned long long found = __builtin_amdgcn_ballot_w64(f.cnt != 0u);
        if (found != 0ull) {
            // cold: the wave's sum and minimum in scalar registers, one lane with findings at a time
            unsigned long long c = 0ull, m = kVerifyNone;
            do {
                const int lane = __builtin_ctzll(found);
                c += (uint32_t)__builtin_amdgcn_readlane((int)f.cnt, lane);
                const unsigned long long at = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(f.first >> 32), lane) << 32) |
                                              (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)f.first, lane);
                m = at < m ? at : m;
                found &= found - 1ull;
            } while (found != 0ull);
            if ((tid & 63u) == 0u) {
                VerifyTableSummary *sum = a.sum;
                CycleVerifyResult *res = a.results + (entry & 0xFFFFFFu);
                __hip_atomic_fetch_add(&res->mismatches, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_min(&res->first_mismatch, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&sum->mismatches, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_min(&sum->first_bad_entry, (unsigned long long)(entry & 0xFFFFFFu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            f.cnt = 0u;
            f.first = kVerifyNone;
        }
    };

    uint32_t pending = 0;
    const uint32_t q_next_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_next[0];
    const uint32_t one = 1u;
    // Compares chunk g of view v, whose comparand words are in e; `late` is the comparand of the chunk after it (g_next, already
    // located: view `next`): word u of it is asked for as soon as word u of this one has been used, so it has the rest of this trip and
    // the start of the next to arrive.  `par` = trip & 1.
    auto compare = [&](Raw(&w)[U], u32x4(&e)[U], const View &v, uint32_t g, const View &next, uint32_t g_next, const Late &late, uint32_t par) {
        const Span s = span(g, v);
        const uint32_t sh = (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
        // both keystreams' states of the lane's first word of the chunk: one chunk jump, shared
        const uint32_t c = g - v.lo;
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        uint32_t sa = mulmod_keep(v.lane_base[0], p), sb = mulmod_keep(v.lane_base[1], p);
        uint32_t low = ~0u; // (positions in a chunk are below 2^16; 64 bits only once, below)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 x = rekey_word(funnel(w[u], sh), sa, sb) ^ e[u];
            e[u] = __builtin_amdgcn_raw_buffer_load_b128(late.re, voff + u * SUB - late.cut, 0, AUX_NT);
            if (u + 1 < U) { // (one pair of states live, not U: the loads need the registers)
                sa = mulmod_keep(sa, lcg::kTileLo.v[BLOCK / 256]);
                sb = mulmod_keep(sb, lcg::kTileLo.v[BLOCK / 256]);
            }
            // a lane outside the chunk's bytes read nothing on either side: its x is the keystreams, not a finding
            const uint32_t inside = voff + (uint32_t)u * SUB - s.cut < s.bytes ? ~0u : 0u;
            x &= inside;
            // clean data costs three ORs and this test per word; the rest is for the waves that have something to report
            if (__builtin_amdgcn_ballot_w64(any_bits(x) != 0u) != 0ull) {
                if (any_bits(x) != 0u) note_word(f.cnt, low, x, voff + (uint32_t)u * SUB);
            }
        }
        if (low != ~0u) {
            // index in the entry of the byte at the chunk's origin: head_n + chunk offset - lead, modulo 2^64
            const unsigned long long j = (uint64_t)(v.entry >> 24) + s.off - (v.lead_rem & 0xFFFFu) + low;
            f.first = j < f.first ? j : f.first;
        }
        if (g_next >= total || next.entry != v.entry) flush(v.entry); // the workgroup leaves the entry (or ends)
        if (tid == 0)
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * par), "v"(pending) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    };
    auto take_published = [&](uint32_t par) {
        uint32_t t;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * par) : "memory");
        return (uint32_t)PREFIX * G + (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    };

    uint32_t cq[NB];
    static_assert(NB == 2 && DEPTH == 1, "the unrolled trip's position is the mailbox slot's parity");
    static_assert(PREFIX == NB, "the static positions are exactly the ones cq[] starts with");
#pragma unroll
    for (int i = 0; i < NB; ++i) cq[i] = blk + (uint32_t)i * G;
    if (cq[0] < total) {
        Raw w[NB][U];
        u32x4 e[U];
        {
            const Late first = load(w[0], vb[0], vb[NB - 1], cq[0]);
#pragma unroll
            for (int u = 0; u < U; ++u) e[u] = __builtin_amdgcn_raw_buffer_load_b128(first.re, voff + u * SUB - first.cut, 0, AUX_NT);
        }
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                __builtin_amdgcn_s_barrier();
                if (tid == 0) pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const Late late = load(w[(p + DEPTH) % NB], vb[(p + DEPTH) % NB], vb[p], cq[DEPTH]);
                __builtin_amdgcn_sched_barrier(0);
                compare(w[p], e, vb[p], cq[0], vb[(p + DEPTH) % NB], cq[DEPTH], late, (uint32_t)p);
#pragma unroll
                for (int i = 0; i < DEPTH; ++i) cq[i] = cq[i + 1];
                cq[DEPTH] = take_published((uint32_t)p);
                if (cq[0] >= total) {
                    finished = true;
                    break;
                }
            }
        }
    }
}

namespace {
template <int U, int BLOCK> struct RekeyVerifyTableShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const RekeyVerifyTableArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_rekey_verify_table_kernel<U, BLOCK>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() { return table_kernel_name<U, BLOCK>("modgpu_cycle_rekey_verify_table_kernel"); }
};
using RekeyVerifyTableStream = RekeyVerifyTableShape<4, 1024>; // the rekey verify kernel's shape: 64 KiB chunks
static_assert(RekeyVerifyTableStream::chunk == kChunk, "one chunk size for the plan and the stream");
} // namespace

uint32_t modgpu_rekey_verify_table_chunk_bytes() { return RekeyVerifyTableStream::chunk; }
uint32_t modgpu_rekey_verify_table_block() { return RekeyVerifyTableStream::block; }
const char *modgpu_rekey_verify_table_kernel_name() { return RekeyVerifyTableStream::name(); }
hipError_t modgpu_launch_rekey_verify_table_plan(const RekeyVerifyTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_verify_table_plan, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_verify_table_finish(const RekeyVerifyTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_verify_table_finish, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_verify_table_stream(const RekeyVerifyTableArgs &a, uint32_t grid, hipStream_t stream)
{
    RekeyVerifyTableStream::launch(a, grid, stream);
    return hipGetLastError();
}
