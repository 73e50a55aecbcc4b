// cycle_rekey_table_kernel.hip -- a TABLE of rekey entries that lives in device memory, any number of them, in three launches:
// dst_i[j] = src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j], the plaintext only in registers.  The two-keystream
// block: cycle_rekey_impl.h; the jump tables and the single-state arithmetic: cycle_kernel_impl.h; both included and not changed (their
// hashes are the rekey kernel's and the roofline kernel's; this TU has its own).  What the table TUs have in common -- an entry on the
// chunk grid and its six states, the scan, the totals, the search levels and one level of their descent, a chunk's span, the funnel,
// mulmod_keep -- is cycle_table_impl.h.
//
// The structure is the table call's (cycle_table_kernel.hip), the stream body the rekey kernel's (cycle_rekey_kernel.hip):
//   plan    one thread per entry: reads the entry where the caller left it (when the launch RUNS), checks it (a NULL pointer with bytes
//           to move, nonzero flags or reserved, a body beyond the chunk jump tables), lays it on the chunk grid of its destination,
//           computes SIX base states on the device -- head, body and tail for each of the two keystreams, key * a^(off+1) by four byte
//           tables -- and scans the chunk counts of its 1024 entries in LDS.  Workgroup 0 resets the workspace's ticket and status.
//   finish  one thread per entry: the entries' starts made global, the call refused whole on any bad entry (nothing written, the
//           lowest bad index into the status), else the search levels and the < 16 ragged bytes at each end under both keystreams.
//   stream  persistent 1024-thread workgroups on 64 KiB chunks of absolute chunk-aligned DESTINATION addresses handed out by the
//           workspace's ticket counter with a static prefix of two, a ping-pong load pipeline, nt loads and nt sc1 stores, the
//           v_alignbyte_b32 funnel chosen per chunk; a chunk's entry is found by the table call's 16-ary descent of scalar loads and
//           kept in one of two views; every lane-word carries two states, both counted from the same chunk origin, so the chunk and
//           lane jumps are shared and each keystream costs its own multiply.
//
// The identity keystream (a key == 0 mod 2^31-1).  Its state is kept as 2^31-1 rather than 0: the block turns that state into the
// packed byte 0xFF for every byte of the word (2^31-1 times any power of a folds to 2^31-1 again, with no carry), and the keystream
// byte is its complement, 0.  Every multiply that derives a state from an entry's base is mulmod_keep, which leaves 2^31-1 where
// mulmod_canon would give 0.  So no entry needs a case of its own: an identity stream drops out of the XOR, two of them make a copy,
// and the same reduced key at offsets equal mod 2^31-2 gives two equal states that cancel -- all bit-exact with the rekey call, whose
// host routes those entries to the out-of-place kernel or a copy.
//
// The REKEY DIGEST mode (cycle_rekey_table_kernel.h: REKEY_TABLE_DIGEST; modgpu_rekey_digest_table_device) runs the same three kernels
// over the same table: plan is unchanged, finish also sums the ragged edges it rekeys and stores every record whole, and the stream
// kernel takes its second loop -- one uniform branch apart, with registers, views and LDS of its own scope -- which stores as the first
// does and sums the stored word, the word it read, or the plaintext between the two keystreams.  Its protocol is written where the loop is.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_impl.h"
#include "cycle_table_impl.h"
#include "cycle_rekey_table_kernel.h"

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_table_plan(RekeyTableArgs a)
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
        const RekeyTableEntry E = a.entries[i];
        const TableGrid g = table_grid(E, E.flags | E.reserved);
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

// ---- finish: global starts, the status, the search levels, the ragged edges --------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_table_finish(RekeyTableArgs a)
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
            // refused: write nothing; the lowest bad entry -- a refused one, or the first whose chunks pass the ticket range
            if (P.bad || start + P.chunks > kTableMaxChunks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        } else {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k) table_set_level(a.level[k], k, a.top, i, start);
            // the < 16 bytes in front of the body and behind it under both keystreams: all loads first (dst may be src), then the stores
            const RekeyTableEdge X = a.edge[i];
            const uint8_t *sb = P.src_origin + P.lead;
            uint8_t *db = P.dst_origin + P.lead;
            const uint64_t body = P.end - P.lead;
            uint8_t hb[15], tb[15];
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                if (j < P.head_n) hb[j] = sb[(int64_t)j - P.head_n];
                if (j < P.tail_n) tb[j] = sb[body + j];
            }
            if (a.mode == REKEY_TABLE_PLAIN) {
#pragma unroll
                for (uint32_t j = 0; j < 15; ++j) {
                    const uint32_t y = c_pow_b0.v[j];
                    if (j < P.head_n) db[(int64_t)j - P.head_n] = rekey_byte(hb[j], mulmod_keep(X.head[0], y), mulmod_keep(X.head[1], y));
                    if (j < P.tail_n) db[body + j] = rekey_byte(tb[j], mulmod_keep(X.tail[0], y), mulmod_keep(X.tail[1], y));
                }
            } else {
                // the rekey digest mode sums them on the way, on its side: byte j of the entry weighs j mod 65521, the head starts at
                // 0 and the tail at n - tail_n.  The plaintext byte is d ^ ~state_from (an identity key keeps 2^31-1: keystream byte 0).
                // Each sum is below 30 * 255 * 65521 < 2^29.
                const uint32_t after = (uint32_t)(((unsigned long long)P.head_n + body) % kDigestTableMod);
                uint32_t s1 = 0u, s2 = 0u;
                auto pick = [&](uint8_t d, uint8_t o, uint32_t sf) {
                    return (uint32_t)(a.side == REKEY_TABLE_SIDE_INPUT ? d : a.side == REKEY_TABLE_SIDE_PLAIN ? (uint8_t)(d ^ (uint8_t)~sf) : o);
                };
#pragma unroll
                for (uint32_t j = 0; j < 15; ++j) {
                    const uint32_t y = c_pow_b0.v[j];
                    if (j < P.head_n) {
                        const uint32_t sf = mulmod_keep(X.head[0], y);
                        const uint8_t o = rekey_byte(hb[j], sf, mulmod_keep(X.head[1], y));
                        db[(int64_t)j - P.head_n] = o;
                        const uint32_t x = pick(hb[j], o, sf);
                        s1 += x;
                        s2 += j * x;
                    }
                    if (j < P.tail_n) {
                        const uint32_t sf = mulmod_keep(X.tail[0], y);
                        const uint8_t o = rekey_byte(tb[j], sf, mulmod_keep(X.tail[1], y));
                        db[body + j] = o;
                        const uint32_t x = pick(tb[j], o, sf);
                        s1 += x;
                        s2 += (after + j) % kDigestTableMod * x;
                    }
                }
                // the record stored whole -- s1, s2 reduced, the entry's n, 0 --: nothing needs clearing beforehand
                a.records[i] = DigestTableRecord{s1, s2 % kDigestTableMod, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
            }
        }
    }
    if (ok && b == 0 && tid < 16)
        for (uint32_t k = 0; k < kTableLevels; ++k) table_pad_level(a.level[k], a.level_n[k], k, a.top, tid);
}

// ---- stream ------------------------------------------------------------------------------------------------------------------------

template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) MODGPU_REKEY_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_rekey_table_kernel(RekeyTableArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
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

    // ---- the rekey digest loop (cycle_rekey_table_kernel.h: REKEY_TABLE_DIGEST): the loop below, which also sums one word per word it
    // stores -- the stored word, the funnelled word it read, or the plaintext between the two keystreams (a.side) -- and adds the sums to
    // the entry's record.  One uniform branch; the plain loop is not entered, and this scope's registers, views and LDS are its own.
    // The summed word.  x is the funnelled source word, wa / wb the packed state words of the block, each the COMPLEMENT of its
    // keystream.  Stored: x ^ wa ^ wb (the complements cancel); plaintext: x ^ wa ^ ~0; input: x.  One form, three uniform masks in
    // VGPRs: x ^ (wa & ma) ^ (wb & mb) ^ cm -- two v_bitop3_b32 0x78 (p ^ (q & r)) and one v_xor_b32 per dword; the stored word keeps its
    // own three-input XOR, so the guard's count of 0x96 stays one per dword of a block.
    // Widths, the chunk origin's index, the masked lanes, the fold and its protocol are the cycle digest loop's, word for word
    // (cycle_table_kernel.hip): 32-bit c1 / c2 per chunk, 64-bit lane sums across chunks, the origin's index reduced as
    // (head_n + 2 * 65521 - lead + 15 * c) mod 65521, a lane outside the chunk's bytes masked WHOLE (its loads gave zeros, but 0 ^ ks is
    // the keystream), and at a change of entry the DPP ladder to lane 63, one ds_add_u32 pair per wave into the slot of the trip's
    // parity BEFORE the barrier the trip has anyway, then thread 0's pair of non-returning 64-bit adds.  No barrier is added.
    // Both states of a view go through mulmod_keep, as in the plain loop: no key pair is a case of its own.
    if (__builtin_expect(a.mode != REKEY_TABLE_PLAIN, 0)) { // (laid out behind the plain loop, whose code stays where it was)
        static_assert(CHUNK == 65536, "a view packs two offsets in a chunk into 32 bits");
        __shared__ uint32_t dg_slot[4]; // [parity][s1, s2]
        struct DView {
            uint8_t *dst0;         // the entry's chunk origin
            const uint8_t *src0;   // the source byte that pairs with it
            uint32_t lo, hi;       // global chunks [lo, hi)
            uint32_t lead_rem;     // bits 0..15: lead; bits 16..31: bytes of the last chunk from its chunk origin, less 1
            uint32_t entry;        // bits 0..23: index in the table; bits 24..27: head_n
            uint32_t lane_base[2]; // per lane: both keystreams' states of this lane's word 0 in the entry's chunk 0
        };
        static_assert(kTableMaxEntries <= (1u << 24), "an entry's index and its head_n share a register");
        auto in = [](uint32_t g, const DView &v) { return g - v.lo < v.hi - v.lo; };
        auto search = [&](uint32_t g, DView &v) {
            uint32_t j = 0;
            int k = (int)a.top;
#pragma unroll 1
            do j = table_descend(a.level[k], j, g); // (level 0 always exists)
            while (--k >= 0);
            const RekeyTablePlan P = *as_const(a.plan + j);
            v.dst0 = P.dst_origin;
            v.src0 = P.src_origin;
            v.lead_rem = table_lead_rem(P);
            v.lo = (uint32_t)P.start;
            v.hi = (uint32_t)P.start + P.chunks;
            v.entry = j | (P.head_n << 24);
            v.lane_base[0] = mulmod_keep(P.base_from, lane_mul);
            v.lane_base[1] = mulmod_keep(P.base_to, lane_mul);
        };
        auto span = [&](uint32_t g, const DView &v) { return table_span_packed<CHUNK>(g, total, v); };
        DView vb[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) vb[i] = DView{nullptr, nullptr, 0, 0, 0, ~0u, {lcg::M, lcg::M}};
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
        // the side as three lane masks in VGPRs, so that choosing the summed word holds no scalar register over the loop (the block
        // alone takes sixteen for its constants), and the static prefix's width in a fourth: thread 0 publishes the next POSITION
        uint32_t ma, mb, cm, prefix;
        asm("v_mov_b32 %0, %1" : "=v"(ma) : "s"(a.side == REKEY_TABLE_SIDE_INPUT ? 0u : ~0u));
        asm("v_mov_b32 %0, %1" : "=v"(mb) : "s"(a.side == REKEY_TABLE_SIDE_OUTPUT ? ~0u : 0u));
        asm("v_mov_b32 %0, %1" : "=v"(cm) : "s"(a.side == REKEY_TABLE_SIDE_PLAIN ? ~0u : 0u));
        asm("v_mov_b32 %0, %1" : "=v"(prefix) : "s"((uint32_t)PREFIX * G));
        uint32_t pending = 0;
        const uint32_t q_next_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_next[0];
        const uint32_t slot_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&dg_slot[0];
        const uint32_t one = 1u, zero = 0u;
        if (tid == 0) // both slots start clean; the first trip's barrier lies between this and their first use
            asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %1 offset:4\n\tds_write_b32 %0, %1 offset:8\n\tds_write_b32 %0, %1 offset:12\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         :
                         : "v"(slot_lds), "v"(zero)
                         : "memory");
        // p ^ (q & r): v_bitop3_b32's truth table 0xF0 ^ (0xCC & 0xAA)
        auto xor_and = [](uint32_t p, uint32_t q, uint32_t r) {
            uint32_t o;
            asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x78" : "=v"(o) : "v"(p), "v"(q), "v"(r));
            return o;
        };
        // chunk g of view v; g_next (view `next`) is the chunk the workgroup stores after it; `par` = trip & 1
        auto sum_store = [&](Raw(&w)[U], const DView &v, uint32_t g, const DView &next, uint32_t g_next, uint32_t par) {
            const Span s = span(g, v);
            const uint32_t sh = (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
            const uint32_t c = g - v.lo; // < 2^24
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
            uint32_t c1 = 0u, c2 = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t wa[4], wb[4];
                ks_word2_carry(sa, sb, wa, wb);
                u32x4 y;
                y.x = xor_and(xor_and(d[u].x, wa[0], ma), wb[0], mb) ^ cm;
                y.y = xor_and(xor_and(d[u].y, wa[1], ma), wb[1], mb) ^ cm;
                y.z = xor_and(xor_and(d[u].z, wa[2], ma), wb[2], mb) ^ cm;
                y.w = xor_and(xor_and(d[u].w, wa[3], ma), wb[3], mb) ^ cm;
                d[u].x = xor3(d[u].x, wa[0], wb[0]);
                d[u].y = xor3(d[u].y, wa[1], wb[1]);
                d[u].z = xor3(d[u].z, wa[2], wb[2]);
                d[u].w = xor3(d[u].w, wa[3], wb[3]);
                // one word's sums; a lane outside the chunk's bytes contributes nothing
                const uint32_t q = voff + (uint32_t)u * SUB;
                uint32_t b, ws;
                word_sums(y, wt, b, ws);
                const bool inside = q - s.cut < s.bytes;
                b = inside ? b : 0u;
                ws = inside ? ws : 0u;
                c1 += b;
                c2 += q * b + ws;
                if (u + 1 < U) {
                    sa = mulmod_keep(sa, lcg::kTileLo.v[BLOCK / 256]);
                    sb = mulmod_keep(sb, lcg::kTileLo.v[BLOCK / 256]);
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
        uint32_t lead, lo, hi;  // global chunks [lo, hi) are the entry's chunks 0 .. hi - lo - 1
        uint32_t lane_base[2]; // per lane: both keystreams' states of this lane's word 0 in the entry's chunk 0
    };
    auto in = [](uint32_t g, const View &v) { return g - v.lo < v.hi - v.lo; };
    // the entry of chunk g < total: the last entry whose start is <= g, by a 16-ary descent of the levels
    auto search = [&](uint32_t g, View &v) {
        uint32_t j = 0;
#pragma unroll 1
        for (int k = (int)a.top; k >= 0; --k) j = table_descend(a.level[k], j, g);
        const RekeyTablePlan P = *as_const(a.plan + j);
        v.dst0 = P.dst_origin;
        v.src0 = P.src_origin;
        v.end = P.end;
        v.lead = P.lead;
        v.lo = (uint32_t)P.start;
        v.hi = (uint32_t)P.start + P.chunks;
        v.lane_base[0] = mulmod_keep(P.base_from, lane_mul);
        v.lane_base[1] = mulmod_keep(P.base_to, lane_mul);
    };
    // where chunk g lies: offset of its chunk from the entry's origin, the cut in front of the body (chunk 0 only), its bytes
    auto span = [&](uint32_t g, const View &v) { return table_span<CHUNK>(g, total, v); };
    View vb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vb[i] = View{nullptr, nullptr, 0, 0, 0, 0, {lcg::M, lcg::M}};
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
        // both keystreams' states of this lane's U words: one chunk jump, shared
        const uint32_t c = g - v.lo;
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        uint32_t sa = mulmod_keep(v.lane_base[0], p), sb = mulmod_keep(v.lane_base[1], p);
        // the funnel only where the chunk's source is not dword-aligned (a uniform branch): the pass is VALU-bound, and the rekey
        // kernel's plain form has no v_alignbyte_b32 either
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
template <int U, int BLOCK> struct RekeyTableShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const RekeyTableArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_rekey_table_kernel<U, BLOCK>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() { return table_kernel_name<U, BLOCK>("modgpu_cycle_rekey_table_kernel"); }
};
using RekeyTableStream = RekeyTableShape<4, 1024>; // the rekey kernel's shape: 64 KiB chunks
static_assert(RekeyTableStream::chunk == kChunk, "one chunk size for the plan and the stream");
} // namespace

uint32_t modgpu_rekey_table_chunk_bytes() { return RekeyTableStream::chunk; }
uint32_t modgpu_rekey_table_block() { return RekeyTableStream::block; }
const char *modgpu_rekey_table_kernel_name() { return RekeyTableStream::name(); }
hipError_t modgpu_launch_rekey_table_plan(const RekeyTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_table_plan, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_table_finish(const RekeyTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_rekey_table_finish, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_rekey_table_stream(const RekeyTableArgs &a, uint32_t grid, hipStream_t stream)
{
    RekeyTableStream::launch(a, grid, stream);
    return hipGetLastError();
}
// the rekey digest table call: the same kernels, the mode set (side and records are the caller's)
namespace {
RekeyTableArgs digest_mode(const RekeyTableArgs &a)
{
    RekeyTableArgs d = a;
    d.mode = REKEY_TABLE_DIGEST;
    return d;
}
} // namespace
hipError_t modgpu_launch_rekey_digest_table_plan(const RekeyTableArgs &a, hipStream_t stream) { return modgpu_launch_rekey_table_plan(digest_mode(a), stream); }
hipError_t modgpu_launch_rekey_digest_table_finish(const RekeyTableArgs &a, hipStream_t stream) { return modgpu_launch_rekey_table_finish(digest_mode(a), stream); }
hipError_t modgpu_launch_rekey_digest_table_stream(const RekeyTableArgs &a, uint32_t grid, hipStream_t stream)
{
    return modgpu_launch_rekey_table_stream(digest_mode(a), grid, stream);
}
