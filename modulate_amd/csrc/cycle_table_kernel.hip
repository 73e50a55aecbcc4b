// cycle_table_kernel.hip -- a TABLE of out-of-place entries that lives in device memory, any number of them, in three launches:
// dst_i[j] = src_i[j] ^ ks(key_i)[off_i + j].  Device code of the arithmetic, the jump tables and the keystream block:
// cycle_kernel_impl.h, included and not changed (its hash is modgpu_kernel_source_hash; this TU has its own).  What the five table TUs
// have in common -- an entry on the chunk grid, the scan, the totals, the search levels and one level of their descent, a chunk's span,
// the funnel -- is cycle_table_impl.h.
//
//   plan    one thread per entry: reads the entry where the caller left it (when the launch RUNS, not when it is queued), checks it
//           (a NULL pointer with bytes to move, nonzero flags, a body beyond the chunk jump tables), lays it on the chunk grid of its
//           destination, computes its three base states on the device (key * a^(off+1) by four byte tables), and scans the chunk
//           counts of its 1024 entries in LDS.  Workgroup 0 resets the workspace's ticket counter and status: every call starts
//           clean in stream order, with no memset on any other stream.
//   finish  one thread per entry again: every workgroup adds up the chunk counts of the 1024-entry records before its own (and of
//           all of them: the total), so the entries' starts are global without a third scan pass; then either the call is refused
//           -- a bad entry anywhere, or more chunks than 32-bit tickets hand out -- and nothing at all is written (the lowest bad
//           index goes to the status), or each entry's start goes into the search levels and its < 16 ragged bytes at either end
//           are cycled bytewise.
//   stream  the out-of-place kernel's shape (cycle_to_kernel.hip): persistent 1024-thread workgroups, 64 KiB chunks on absolute
//           chunk-aligned DESTINATION addresses handed out by a ticket counter (in the workspace) with a static prefix of two, a
//           ping-pong load pipeline, workgroup-synchronous bursts, nt loads and nt sc1 stores.  What differs: an entry's cut first
//           chunk is an ordinary ticket (its lanes in front of the body wrap past num_records), so small entries spread over the
//           chip like large ones; the v_alignbyte_b32 funnel is chosen per chunk (a uniform branch on the source's phase); a
//           chunk of an identity-key entry is copied; and a chunk's entry is FOUND rather than walked to.
//
// Finding a chunk's entry.  The table may be 100 000 entries long, so the stream launch cannot walk it.  The finish launch writes the
// entries' chunk starts as a 16-ary search structure -- level k holds the start of every 16^k-th entry, padded with ~0 to whole lines
// of 16 -- and a workgroup descends it with one s_load_dwordx16 per level (2 for 17 entries, 5 for 100 000), then loads the entry's
// CycleTablePlan with one more.  All of it is scalar memory: lgkmcnt, not vmcnt, so the descent for the chunk about to be loaded never
// waits for the loads still in flight for the chunk being computed (a vector-memory search would, and the pipeline would collapse to
// one chunk in flight).  Each workgroup keeps the views of the two chunks in its pipeline; a chunk inside one of them needs no search.
//
// The CYCLE DIGEST mode (cycle_table_kernel.h: CYCLE_TABLE_DIGEST; modgpu_cycle_digest_table_device) runs the same three kernels over
// the same table: plan is unchanged, finish also sums the ragged edges it cycles and stores every record whole, and the stream kernel
// takes its second loop -- one uniform branch apart, with registers, views and LDS of its own scope -- which stores as the first does
// and sums what it stores, or what it read.  Its protocol is written where the loop is.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_table_impl.h"
#include "cycle_table_kernel.h"

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_table_plan(CycleTableArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + tid;
    if (blockIdx.x == 0 && tid == 0) {
        a.hdr->ticket = 0;
        a.hdr->first_bad = kTableNoBad;
        a.hdr->total = 0;
    }
    uint64_t cnt = 0;
    uint32_t bad = 0;
    if (i < a.n) {
        const CycleTableEntry E = a.entries[i];
        const TableGrid g = table_grid(E, E.flags);
        cnt = g.cnt;
        bad = g.bad;
        CycleTablePlan P;
        table_plan_entry(P, E, g);
        a.plan[i] = P;
    }
    table_plan_store(a.plan, a.blk, a.n, i, cnt, bad, tid);
}

// ---- finish: global starts, the status, the search levels, the ragged edges --------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_table_finish(CycleTableArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t i = (uint64_t)b * kTableBlock + tid;
    const TableTotals T = table_totals(a.blk, a.n_blk, b, tid);
    const bool ok = T.bad == 0 && T.total <= kTableMaxChunks;
    if (b == 0 && tid == 0) a.hdr->total = ok ? T.total : 0;
    if (i < a.n) {
        const CycleTablePlan P = a.plan[i];
        const uint64_t start = T.before + P.start;
        if (!ok) {
            // refused: write nothing; the lowest bad entry -- a refused one, or the first whose chunks pass the ticket range
            if (P.bad || start + P.chunks > kTableMaxChunks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        } else {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k) table_set_level(a.level[k], k, a.top, i, start);
            // the < 16 bytes in front of the body and behind it: all loads first (dst may be src), then the stores
            const uint8_t *sb = P.src_origin + P.lead;
            uint8_t *db = P.dst_origin + P.lead;
            const uint64_t body = P.end - P.lead;
            uint8_t hb[15], tb[15];
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                if (j < P.head_n) hb[j] = sb[(int64_t)j - P.head_n];
                if (j < P.tail_n) tb[j] = sb[body + j];
            }
            const bool copy = P.base_head == 0;
            // the cycle digest mode sums them on the way, on its side of the XOR: byte j of the entry weighs j mod 65521, the head
            // starts at 0 and the tail at n - tail_n.  Each sum is below 30 * 255 * 65521 < 2^29.
            const bool input = a.side == CYCLE_TABLE_SIDE_INPUT;
            const uint32_t after = (uint32_t)(((unsigned long long)P.head_n + body) % kDigestTableMod);
            uint32_t s1 = 0u, s2 = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                if (j < P.head_n) {
                    const uint8_t o = copy ? hb[j] : cycle_byte(hb[j], mulmod_canon(P.base_head, c_pow_b0.v[j]));
                    db[(int64_t)j - P.head_n] = o;
                    const uint32_t x = input ? hb[j] : o;
                    s1 += x;
                    s2 += j * x;
                }
                if (j < P.tail_n) {
                    const uint8_t o = copy ? tb[j] : cycle_byte(tb[j], mulmod_canon(P.base_tail, c_pow_b0.v[j]));
                    db[body + j] = o;
                    const uint32_t x = input ? tb[j] : o;
                    s1 += x;
                    s2 += (after + j) % kDigestTableMod * x;
                }
            }
            // the record stored whole -- s1, s2 reduced, the entry's n, 0 --: nothing needs clearing beforehand
            if (a.mode != CYCLE_TABLE_PLAIN)
                a.records[i] = DigestTableRecord{s1, s2 % kDigestTableMod, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
        }
    }
    if (ok && b == 0 && tid < 16)
        for (uint32_t k = 0; k < kTableLevels; ++k) table_pad_level(a.level[k], a.level_n[k], k, a.top, tid);
}

// ---- stream ------------------------------------------------------------------------------------------------------------------------
template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) MODGPU_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_table_kernel(CycleTableArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr int ALG = 2;
    constexpr int SAUX = AUX_SC1 | AUX_NT;
    constexpr int DEPTH = 1;
    constexpr uint32_t CHUNK = (uint32_t)U * BLOCK * lcg::WORD;
    static_assert(CHUNK == kChunk, "the plan lays entries on this chunk grid");
    constexpr uint32_t SUB = BLOCK * lcg::WORD;
    constexpr int NB = DEPTH + 1;
    constexpr int PREFIX = DEPTH + 1;
    const uint32_t tid = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    const uint32_t G = gridDim.x;
    const uint32_t total = (uint32_t)*as_const(&a.hdr->total); // 0 when the finish launch refused the call
    __shared__ uint32_t q_next[2];
    uint32_t trip = 0;
    const uint32_t voff = tid * lcg::WORD;
    const uint32_t lane_mul = mulmod_canon(c_tile_lo.v[tid >> 8], c_lane_pow.v[tid & 255]);

    // ---- the cycle digest loop (cycle_table_kernel.h: CYCLE_TABLE_DIGEST): the loop below, which also sums every word it stores (or the
    // funnelled word it read: a.side) and adds the sums to the entry's record.  One uniform branch; the plain loop is not entered, and
    // this scope's registers, views and LDS are its own.
    // Widths (the verify table TU's digest loop has the same sums).  Per lane-word b = sum of bytes <= 4 080 and w = sum of i * byte_i <=
    // 30 600.  Per chunk a lane adds, in 32 bits, c1 = sum of b <= 16 320 and c2 = sum of (q * b + w), q < 65 536 the word's offset from
    // the chunk origin: < 1.07e9.  The chunk origin's index in the entry enters reduced (bm < 65 521): bm * c1 + c2 < 2^32.  Across
    // chunks the lane keeps 64-bit sums that grow by < 2^32 per chunk, and an entry has fewer than 2^24 chunks.
    // The grid lies on the DESTINATION: the byte at dst_origin + x is the entry's byte head_n + (x - lead), so the chunk origin's index
    // is head_n - lead + 65 536 * c -- below zero for chunk 0 of an entry with a lead; it is taken mod 65 521 as
    // (head_n + 2 * 65 521 - lead + 15 * c) mod 65 521, every term non-negative.  A lane outside the chunk's bytes -- in front of a cut
    // first chunk's body, past a ragged end -- is masked WHOLE on either side: its loads gave zeros, but 0 ^ ks is the keystream, and
    // the lane just past the end holds the funnel's extra dword.
    // Leaving an entry (or ending), the lanes' sums are reduced mod 65 521, folded per wave by DPP, and lane 63 of each wave adds the
    // wave's pair into the LDS slot of the trip's parity (< 16 * 64 * 65 521 < 2^26) BEFORE the barrier the trip has anyway; behind it
    // thread 0 reduces the slot, sends ONE pair of non-returning 64-bit adds to the entry's record and clears the slot.  The slot of the
    // other parity is the next trip's: a wave that runs ahead into a trip that flushes too does not meet thread 0's read, and the trip
    // after that is two barriers away.  No barrier is added: two per trip, as below.
    if (__builtin_expect(a.mode != CYCLE_TABLE_PLAIN, 0)) { // (laid out behind the plain loop, whose code stays where it was)
        static_assert(CHUNK == 65536, "a view packs two offsets in a chunk into 32 bits");
        __shared__ uint32_t dg_slot[4]; // [parity][s1, s2]
        struct DView {
            uint8_t *dst0;       // the entry's chunk origin
            const uint8_t *src0; // the source byte that pairs with it
            uint32_t lo, hi;     // global chunks [lo, hi)
            uint32_t lead_rem;   // bits 0..15: lead; bits 16..31: bytes of the last chunk from its chunk origin, less 1
            uint32_t entry;      // bits 0..23: index in the table; bits 24..27: head_n
            uint32_t lane_base;  // per lane; 0 in every lane = the identity keystream
        };
        static_assert(kTableMaxEntries <= (1u << 24), "an entry's index and its head_n share a register");
        auto in = [](uint32_t g, const DView &v) { return g - v.lo < v.hi - v.lo; };
        auto search = [&](uint32_t g, DView &v) {
            uint32_t j = 0;
            int k = (int)a.top;
#pragma unroll 1
            do j = table_descend(a.level[k], j, g); // (level 0 always exists)
            while (--k >= 0);
            const CycleTablePlan P = *as_const(a.plan + j);
            v.dst0 = P.dst_origin;
            v.src0 = P.src_origin;
            v.lead_rem = table_lead_rem(P);
            v.lo = (uint32_t)P.start;
            v.hi = (uint32_t)P.start + P.chunks;
            v.entry = j | (P.head_n << 24);
            v.lane_base = mulmod_canon(P.base, lane_mul);
        };
        auto span = [&](uint32_t g, const DView &v) { return table_span_packed<CHUNK>(g, total, v); };
        DView vb[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) vb[i] = DView{nullptr, nullptr, 0, 0, 0, ~0u, 1};
        // chunk g into one buffer of the ping-pong, as the plain loop's: the funnel's extra dword only where the source needs it
        auto load = [&](Raw(&w)[U], DView &v, const DView &prev, uint32_t g) {
            if (g < total && !in(g, v)) {
                if (in(g, prev)) v = prev;
                else search(g, v);
            }
            const Span s = span(g, v);
            const uint8_t *p = v.src0 + s.off + s.cut;
            const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
            const auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p - sh), 0, (int)(s.bytes + (sh && s.bytes ? 4u : 0u)), 0x00020000);
#pragma unroll
            for (int u = 0; u < U; ++u) w[u].d = __builtin_amdgcn_raw_buffer_load_b128(r, voff + u * SUB - s.cut, 0, AUX_NT);
            if (sh) {
#pragma unroll
                for (int u = 0; u < U; ++u) w[u].e = __builtin_amdgcn_raw_buffer_load_b32(r, voff + u * SUB - s.cut + lcg::WORD, 0, AUX_NT);
            }
        };

        unsigned long long a1 = 0ull, a2 = 0ull; // the lane's sums over the entry its workgroup is in
        const DotWeights wt = dot_weights();
        // the side as a lane mask in a VGPR (all ones: the word as read), so that choosing the summed word is one v_bfi_b32 per dword and
        // holds no scalar register pair over the loop: as a condition it cost the kernel an SGPR spill
        uint32_t input;
        asm("v_mov_b32 %0, %1" : "=v"(input) : "s"(a.side == CYCLE_TABLE_SIDE_INPUT ? ~0u : 0u));
        // ... and the static prefix's width in a VGPR: thread 0 publishes the next POSITION (prefix + ticket), not the ticket, so the
        // grid's size holds no scalar register over the loop either
        uint32_t prefix;
        asm("v_mov_b32 %0, %1" : "=v"(prefix) : "s"((uint32_t)PREFIX * G));
        uint32_t pending = 0;
        const uint32_t q_next_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_next[0];
        const uint32_t slot_lds =(uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&dg_slot[0];
        const uint32_t one = 1u, zero = 0u;
        if (tid == 0) // both slots start clean; the first trip's barrier lies between this and their first use
            asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %1 offset:4\n\tds_write_b32 %0, %1 offset:8\n\tds_write_b32 %0, %1 offset:12\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         :
                         : "v"(slot_lds), "v"(zero)
                         : "memory");
        // chunk g of view v; g_next (view `next`) is the chunk the workgroup stores after it; `par` = trip & 1
        auto sum_store = [&](Raw(&w)[U], const DView &v, uint32_t g, const DView &next, uint32_t g_next, uint32_t par) {
            const Span s = span(g, v);
            const uint32_t sh = (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
            const uint32_t c = g - v.lo; // < 2^24
            u32x4 d[U];
            uint32_t c1 = 0u, c2 = 0u;
            // one word's sums, of the side the records are of; a lane outside the chunk's bytes contributes nothing
            auto add_word = [&](const u32x4 &x, int u) {
                const uint32_t q = voff + (uint32_t)u * SUB;
                uint32_t b, ws;
                word_sums(x, wt, b, ws);
                const bool inside = q - s.cut < s.bytes;
                b = inside ? b : 0u;
                ws = inside ? ws : 0u;
                c1 += b;
                c2 += q * b + ws;
            };
            if (__builtin_amdgcn_readfirstlane((int)v.lane_base) != 0) {
                uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
                p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
                uint32_t st = mulmod_canon(v.lane_base, p);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const u32x4 x = funnel(w[u], sh);
                    d[u] = cycle_word<ALG>(x, st);
                    if (u + 1 < U) st = mulmod_canon(st, lcg::kTileLo.v[BLOCK / 256]);
                    u32x4 y;
                    y.x = (input & x.x) | (~input & d[u].x);
                    y.y = (input & x.y) | (~input & d[u].y);
                    y.z = (input & x.z) | (~input & d[u].z);
                    y.w = (input & x.w) | (~input & d[u].w);
                    add_word(y, u);
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    d[u] = funnel(w[u], sh);
                    add_word(d[u], u);
                }
            }
            // index in the entry of the byte at the chunk's origin, mod 65 521: head_n - lead + CHUNK * c, CHUNK mod 65 521 = 15
            const uint32_t idxm = ((v.entry >> 24) + 2u * kDigestTableMod - (v.lead_rem & 0xFFFFu)) % kDigestTableMod;
            const uint32_t bm = (idxm + (CHUNK % kDigestTableMod) * c) % kDigestTableMod;
            a1 += c1;
            a2 += (unsigned long long)(bm * c1 + c2);
            const bool leaving = g_next >= total || next.entry != v.entry; // (uniform) the workgroup leaves the entry, or ends
            if (leaving) {
                const uint32_t r1 = wave_sum_lane63(digest_red(a1)), r2 = wave_sum_lane63(digest_red(a2));
                a1 = a2 = 0ull;
                if ((tid & 63u) == 63u)
                    asm volatile("ds_add_u32 %0, %1\n\tds_add_u32 %0, %2 offset:4\n\ts_waitcnt lgkmcnt(0)" : : "v"(slot_lds + 8u * par), "v"(r1), "v"(r2) : "memory");
            }
            if (tid == 0)
                asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * par), "v"(prefix + pending) : "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // (the destination's descriptor is made behind the barrier: made in front of it, it holds four scalar registers over the sums)
            auto r = __builtin_amdgcn_make_buffer_rsrc(v.dst0 + s.off + s.cut, 0, (int)s.bytes, 0x00020000);
#pragma unroll
            for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB - s.cut, 0, SAUX);
            if (leaving && tid == 0) {
                uint32_t t1, t2;
                asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:4\n\ts_waitcnt lgkmcnt(0)\n\t"
                             "ds_write_b32 %2, %3\n\tds_write_b32 %2, %3 offset:4\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(t1), "=&v"(t2)
                             : "v"(slot_lds + 8u * par), "v"(zero)
                             : "memory");
                DigestTableRecord *rec = a.records + (v.entry & 0xFFFFFFu);
                __hip_atomic_fetch_add(&rec->s1, (unsigned long long)(t1 % kDigestTableMod), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&rec->s2, (unsigned long long)(t2 % kDigestTableMod), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        auto take_published = [&](uint32_t par) {
            uint32_t t;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * par) : "memory");
            return (uint32_t)__builtin_amdgcn_readfirstlane((int)t); // (a position: thread 0 added the prefix)
        };
        uint32_t cq[NB];
        static_assert(NB == 2 && DEPTH == 1 && PREFIX == NB, "the unrolled trip's position is the mailbox slot's and the sums' slot's parity");
#pragma unroll
        for (int i = 0; i < NB; ++i) cq[i] = blk + (uint32_t)i * G;
        if (cq[0] < total) {
            Raw w[NB][U];
            load(w[0], vb[0], vb[1], cq[0]);
            bool finished = false;
            while (!finished) {
#pragma unroll
                for (int p = 0; p < NB; ++p) {
                    __builtin_amdgcn_s_barrier();
                    if (tid == 0) pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    load(w[(p + DEPTH) % NB], vb[(p + DEPTH) % NB], vb[p], cq[DEPTH]);
                    __builtin_amdgcn_sched_barrier(0);
                    sum_store(w[p], vb[p], cq[0], vb[(p + DEPTH) % NB], cq[DEPTH], (uint32_t)p);
                    cq[0] = cq[1];
                    cq[DEPTH] = take_published((uint32_t)p);
                    if (cq[0] >= total) {
                        finished = true;
                        break;
                    }
                }
            }
        }
        return;
    }

    struct View {
        uint8_t *dst0;       // the entry's chunk origin
        const uint8_t *src0; // the source byte that pairs with it
        uint64_t end;
        uint32_t lead, lo, hi; // global chunks [lo, hi) are the entry's chunks 0 .. hi - lo - 1
        uint32_t base;         // 0: a copy
        uint32_t lane_base;    // per lane: state of this lane's word 0 in the entry's chunk 0
    };
    auto in = [](uint32_t g, const View &v) { return g - v.lo < v.hi - v.lo; };
    // the entry of chunk g < total: the last entry whose start is <= g, by a 16-ary descent of the levels
    auto search = [&](uint32_t g, View &v) {
        uint32_t j = 0;
#pragma unroll 1
        for (int k = (int)a.top; k >= 0; --k) j = table_descend(a.level[k], j, g);
        const CycleTablePlan P = *as_const(a.plan + j);
        v.dst0 = P.dst_origin;
        v.src0 = P.src_origin;
        v.end = P.end;
        v.lead = P.lead;
        v.lo = (uint32_t)P.start;
        v.hi = (uint32_t)P.start + P.chunks;
        v.base = P.base;
        v.lane_base = mulmod_canon(P.base, lane_mul);
    };
    // where chunk g lies: offset of its chunk from the entry's origin, the cut in front of the body (chunk 0 only), its bytes
    auto span = [&](uint32_t g, const View &v) { return table_span<CHUNK>(g, total, v); };
    View vb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vb[i] = View{nullptr, nullptr, 0, 0, 0, 0, 0, 1};
    // chunk g into buffer q; vb[r] is the view of the chunk loaded before it
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
    const uint32_t one = 1u;
    auto process_store = [&](Raw(&w)[U], const View &v, uint32_t g) {
        const Span s = span(g, v);
        const uint32_t sh = (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
        auto r = __builtin_amdgcn_make_buffer_rsrc(v.dst0 + s.off + s.cut, 0, (int)s.bytes, 0x00020000);
        u32x4 d[U];
        if (v.base != 0) {
            const uint32_t c = g - v.lo;
            uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
            p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
            uint32_t st = mulmod_canon(v.lane_base, p);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = cycle_word<ALG>(funnel(w[u], sh), st);
                st = mulmod_canon(st, lcg::kTileLo.v[BLOCK / 256]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) d[u] = funnel(w[u], sh);
        }
        if (tid == 0)
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * (trip & 1u)), "v"(pending) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB - s.cut, 0, SAUX);
        ++trip;
    };
    auto take_published = [&]() {
        uint32_t t;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * ((trip - 1u) & 1u)) : "memory");
        return (uint32_t)PREFIX * G + (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    };

    uint32_t cq[NB];
    static_assert(PREFIX == NB, "the static positions are exactly the ones cq[] starts with");
#pragma unroll
    for (int i = 0; i < NB; ++i) cq[i] = blk + (uint32_t)i * G;
    if (cq[0] < total) {
        Raw w[NB][U];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) load(w[i], vb[i], vb[(i + NB - 1) % NB], cq[i]);
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                __builtin_amdgcn_s_barrier();
                if (tid == 0) pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                load(w[(p + DEPTH) % NB], vb[(p + DEPTH) % NB], vb[p], cq[DEPTH]);
                __builtin_amdgcn_sched_barrier(0);
                process_store(w[p], vb[p], cq[0]);
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

namespace {
template <int U, int BLOCK> struct TableShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const CycleTableArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_table_kernel<U, BLOCK>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() { return table_kernel_name<U, BLOCK>("modgpu_cycle_table_kernel"); }
};
using TableStream = TableShape<4, 1024>; // the work-queue kernel's measured shape: 64 KiB chunks
static_assert(TableStream::chunk == kChunk, "one chunk size for the plan and the stream");
} // namespace

uint32_t modgpu_table_chunk_bytes() { return TableStream::chunk; }
uint32_t modgpu_table_block() { return TableStream::block; }
const char *modgpu_table_kernel_name() { return TableStream::name(); }
hipError_t modgpu_launch_table_plan(const CycleTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_table_plan, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_table_finish(const CycleTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_table_finish, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_table_stream(const CycleTableArgs &a, uint32_t grid, hipStream_t stream)
{
    TableStream::launch(a, grid, stream);
    return hipGetLastError();
}
// the cycle digest table call: the same kernels, the mode set (side and records are the caller's)
namespace {
CycleTableArgs digest_mode(const CycleTableArgs &a)
{
    CycleTableArgs d = a;
    d.mode = CYCLE_TABLE_DIGEST;
    return d;
}
} // namespace
hipError_t modgpu_launch_cycle_digest_table_plan(const CycleTableArgs &a, hipStream_t stream) { return modgpu_launch_table_plan(digest_mode(a), stream); }
hipError_t modgpu_launch_cycle_digest_table_finish(const CycleTableArgs &a, hipStream_t stream) { return modgpu_launch_table_finish(digest_mode(a), stream); }
hipError_t modgpu_launch_cycle_digest_table_stream(const CycleTableArgs &a, uint32_t grid, hipStream_t stream)
{
    return modgpu_launch_table_stream(digest_mode(a), grid, stream);
}
