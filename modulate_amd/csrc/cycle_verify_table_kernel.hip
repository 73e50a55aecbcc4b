// cycle_verify_table_kernel.hip -- a TABLE of verify entries that lives in device memory, any number of them, in three launches:
// result_i = { #{ j : dst_i[j] != (src_i[j] ^ ks(key_i)[off_i + j]) }, the lowest such j, n_i, 0 }, dst being the comparand.  Both sides
// are read once; nothing is written but the results and the workspace.  Device code of the arithmetic, the jump tables and the keystream
// block: cycle_kernel_impl.h, included and not changed (this TU has a hash of its own).
//
// The structure is the table call's (cycle_table_kernel.hip): what the two have in common -- an entry on the chunk grid, the scan, the
// totals, the search levels and one level of their descent, a chunk's span, the funnel -- and a lane's findings
// are cycle_table_impl.h, shared by the table TUs; the compare is the verify kernel's (cycle_verify_kernel.hip):
//   plan    one thread per entry: reads the entry where the caller left it (when the launch RUNS), checks it (a NULL pointer with bytes
//           to compare, nonzero flags, a body beyond the chunk jump tables), lays it on the chunk grid of its COMPARAND, computes its
//           three base states, scans the chunk counts of its 1024 entries in LDS.  Workgroup 0 resets the ticket, the status and the
//           summary: every call, and every replay of a captured one, starts clean in stream order.
//   finish  one thread per entry: the entries' starts made global, the call refused whole on any bad entry (no result is written, the
//           lowest bad index goes to the status), else the search levels, and the < 16 ragged bytes at each end COMPARED bytewise.
//           The thread stores its entry's result whole -- {edge mismatches, lowest edge index or none, n, 0} -- so nothing needs
//           clearing beforehand; an entry with dirty edges goes to the summary here.
//   stream  persistent 1024-thread workgroups on 64 KiB chunks of absolute chunk-aligned COMPARAND addresses handed out by the
//           workspace's ticket counter with a static prefix of two, a ping-pong load pipeline behind the workgroup barrier, nt loads of
//           both sides, the v_alignbyte_b32 funnel and the identity key chosen per chunk (uniform branches), a chunk's entry found by
//           the table call's 16-ary descent of scalar loads and kept in one of two views.  Per lane-word x = src ^ ks ^ expect; lanes
//           outside the chunk's bytes (both loads dropped by the range check: x would be the keystream) are masked; one OR per dword
//           and one ballot per chunk on clean data; only a wave that saw a nonzero OR counts nonzero bytes and takes the lowest index.
//
// The result protocol.  Tickets only grow, so a workgroup's chunks come in increasing order and it passes each entry in ONE contiguous
// run.  Counts and lowest indices stay in registers, per lane, while the entry of the chunk being compared is unchanged; when it
// changes, and at the end, every WAVE flushes for itself: a wave none of whose lanes found anything (one ballot) does nothing, a wave
// with findings folds them in scalar registers (v_readlane_b32 of the lanes that have some) and its lane 0 sends one 64-bit add and one 64-bit unsigned min to the entry's
// result and the same pair (the count; the entry's index) to the summary.  No LDS is allocated for it and NO barrier is added: the test
// on clean data is one ballot per change of entry, so a table of 100 000 one-chunk entries pays a compare and a branch per chunk, and a
// clean table of any size issues no atomic but the ticket fetches.  The stream kernel contains no store of any kind.
//
// The DIGEST mode (cycle_verify_table_kernel.h: VERIFY_TABLE_DIGEST; modgpu_digest_table_device) runs the same three kernels over the
// same kind of table with `dst` ignored: plan lays the grid on the SOURCE, finish sums the ragged edges and stores every record whole,
// and the stream kernel takes its second loop -- one uniform branch apart, with registers, views and LDS of its own scope -- which
// reads one side, sums what the cipher makes of it and adds to the entry's record.  Its protocol is written where the loop is.
//
// The CHECK mode (VERIFY_TABLE_CHECK; modgpu_digest_check_device) is the finish kernel alone, launched without a table: one thread per
// digest RECORD, closed and compared with a manifest of Adler-32 values.  One uniform branch at the top of finish; written where the
// digest mode's arithmetic is.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_table_impl.h"
#include "cycle_verify_table_kernel.h"

// ---- the digest mode's arithmetic (cycle_verify_table_kernel.h: DigestTableRecord) -------------------------------------------------
namespace {
// (the word sums, the reduction and the wave fold are cycle_table_impl.h's: the out-of-place table TU's digesting loop has the same)
// The < 16 bytes in front of an entry's body and behind it, summed bytewise; byte j of the entry weighs j mod 65521.  Each sum is
// below 30 * 255 * 65521 < 2^29.  The record is whole: s1, s2 reduced, the entry's n, 0.
__device__ __forceinline__ DigestTableRecord digest_edges(const CycleTablePlan &P)
{
    const uint8_t *sb = P.src_origin + P.lead;
    const uint64_t body = P.end - P.lead;
    const bool plain = P.base_head == 0;
    const uint32_t after = (uint32_t)(((unsigned long long)P.head_n + body) % kDigestTableMod);
    uint32_t s1 = 0u, s2 = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 15; ++j) {
        if (j < P.tail_n) {
            const uint8_t s = sb[body + j];
            const uint32_t out = plain ? s : cycle_byte(s, mulmod_canon(P.base_tail, c_pow_b0.v[j]));
            s1 += out;
            s2 += (after + j) % kDigestTableMod * out;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 15; ++j) {
        if (j < P.head_n) {
            const uint8_t s = sb[(int64_t)j - P.head_n];
            const uint32_t out = plain ? s : cycle_byte(s, mulmod_canon(P.base_head, c_pow_b0.v[j]));
            s1 += out;
            s2 += j * out;
        }
    }
    return DigestTableRecord{s1, s2 % kDigestTableMod, (unsigned long long)P.head_n + body + P.tail_n, 0ull};
}

// ---- the check mode (cycle_verify_table_kernel.h: VERIFY_TABLE_CHECK; modgpu_digest_check_device) ----------------------------------
// A record closed as modgpu_digest_adler32 closes it: the residues first, then A = (1 + s1) % m, B = (n + n * s1 - s2) % m.  In 32 bits:
// n * s1 <= 65520^2 < 2^32, and the sum behind it is below 3 m.
__device__ __forceinline__ uint32_t digest_close(const DigestTableRecord &r)
{
    constexpr uint32_t m = kDigestTableMod;
    const uint32_t s1 = (uint32_t)(r.s1 % m), s2 = (uint32_t)(r.s2 % m), n = (uint32_t)(r.n % m);
    const uint32_t A = (1u + s1) % m;
    const uint32_t B = (n + n * s1 % m + m - s2) % m;
    return B << 16 | A;
}
// One thread per record.  No LDS, no barrier; a clean manifest sends no atomic.  Workgroups are whole waves (kTableBlock % 64 == 0), so
// a wave's 64 entries are one word of the bitmap; a wave none of whose entries exists (its first is >= n) stores nothing.
__device__ __forceinline__ void digest_check(const VerifyTableArgs &a)
{
    static_assert(kTableBlock % 64 == 0, "a wave's entries are one word of the bitmap");
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + tid;
    const bool first = blockIdx.x == 0 && tid == 0;
    // the producer was refused (one scalar load, uniform for the grid): its records are whatever the caller left there
    if (a.producer && *as_const(&a.producer->first_bad) != kTableNoBad) {
        if (first) {
            a.check->n = a.n;
            a.check->reserved = 1ull;
        }
        return;
    }
    bool bad = false;
    if (i < a.n) {
        const DigestTableRecord r = a.records[i];
        bad = digest_close(r) != a.expect[i];
    }
    const unsigned long long word = __builtin_amdgcn_ballot_w64(bad);
    const uint64_t i0 = i & ~63ull; // the wave's first entry
    if ((tid & 63u) == 0u && i0 < a.n) {
        if (a.bad_bits) a.bad_bits[i0 >> 6] = word;
        if (word != 0ull) {
            __hip_atomic_fetch_add(&a.check->mismatches, (unsigned long long)__builtin_popcountll(word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&a.check->first_mismatch, (unsigned long long)(i0 + (uint64_t)__builtin_ctzll(word)), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (first) a.check->n = a.n; // (a field no atomic touches)
}
} // namespace

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_verify_table_plan(VerifyTableArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + tid;
    if (blockIdx.x == 0 && tid == 0) {
        a.hdr->ticket = 0;
        a.hdr->first_bad = kTableNoBad;
        a.hdr->total = 0;
        if (a.mode == VERIFY_TABLE_COMPARE) { // (a digest call has no summary line)
            a.sum->mismatches = 0ull;
            a.sum->first_bad_entry = kVerifyNone;
            a.sum->entries = a.n;
            a.sum->reserved = 0ull;
        }
    }
    uint64_t cnt = 0;
    uint32_t bad = 0;
    if (i < a.n) {
        CycleTableEntry E = a.entries[i];
        // a digest entry's dst is not looked at: the source takes its place, and the chunk grid is laid on the source
        if (a.mode != VERIFY_TABLE_COMPARE) E.dst = const_cast<uint8_t *>(E.src);
        const TableGrid g = table_grid(E, E.flags); // (dst is the comparand: the chunk grid is laid on it)
        cnt = g.cnt;
        bad = g.bad;
        CycleTablePlan P;
        table_plan_entry(P, E, g);
        a.plan[i] = P;
    }
    table_plan_store(a.plan, a.blk, a.n, i, cnt, bad, tid);
}

// ---- finish: global starts, the status, the search levels, the ragged edges compared, every result initialised ---------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_verify_table_finish(VerifyTableArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t i = (uint64_t)b * kTableBlock + tid;
    if (__builtin_expect(a.mode == VERIFY_TABLE_CHECK, 0)) { // (uniform) modgpu_digest_check_device: records against a manifest, no table
        digest_check(a);
        return;
    }
    const TableTotals T = table_totals(a.blk, a.n_blk, b, tid);
    const bool ok = T.bad == 0 && T.total <= kTableMaxChunks;
    if (b == 0 && tid == 0) a.hdr->total = ok ? T.total : 0;
    if (i < a.n) {
        const CycleTablePlan P = a.plan[i];
        const uint64_t start = T.before + P.start;
        if (!ok) {
            // refused: no result is written; the lowest bad entry -- a refused one, or the first whose chunks pass the ticket range
            if (P.bad || start + P.chunks > kTableMaxChunks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        } else {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k) table_set_level(a.level[k], k, a.top, i, start);
            if (a.mode != VERIFY_TABLE_COMPARE) {
                a.records[i] = digest_edges(P); // the < 16 bytes at either end summed, the record stored whole: nothing needs clearing
            } else {
                // the < 16 bytes in front of the body and behind it, compared bytewise; the index counts from the entry's first byte
                const uint8_t *sb = P.src_origin + P.lead;
                const uint8_t *eb = P.dst_origin + P.lead;
                const uint64_t body = P.end - P.lead;
                const bool plain = P.base_head == 0;
                unsigned long long cnt = 0ull, first = kVerifyNone;
#pragma unroll
                for (uint32_t j = 0; j < 15; ++j) {
                    if (j < P.tail_n) {
                        const uint8_t s = sb[body + j];
                        const uint8_t want = plain ? s : cycle_byte(s, mulmod_canon(P.base_tail, c_pow_b0.v[j]));
                        if (eb[body + j] != want) {
                            ++cnt;
                            const unsigned long long at = (unsigned long long)P.head_n + body + j;
                            first = at < first ? at : first;
                        }
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < 15; ++j) {
                    if (j < P.head_n) {
                        const uint8_t s = sb[(int64_t)j - P.head_n];
                        const uint8_t want = plain ? s : cycle_byte(s, mulmod_canon(P.base_head, c_pow_b0.v[j]));
                        if (eb[(int64_t)j - P.head_n] != want) {
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
    }
    if (ok && b == 0 && tid < 16)
        for (uint32_t k = 0; k < kTableLevels; ++k) table_pad_level(a.level[k], a.level_n[k], k, a.top, tid);
}

// ---- stream ------------------------------------------------------------------------------------------------------------------------
template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) MODGPU_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_verify_table_kernel(VerifyTableArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr int ALG = 2;
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

    // ---- the digest loop (cycle_verify_table_kernel.h: VERIFY_TABLE_DIGEST): the loop below with ONE load stream and sums in place of
    // the compare.  One uniform branch; the verify loop is not entered, and this scope's registers and LDS are its own.
    // Widths (cycle_to_kernel.hip's digest loop has the same sums).  Per lane-word b = sum of bytes <= 4 080 and w = sum of i * byte_i <=
    // 30 600.  Per chunk a lane adds, in 32 bits, c1 = sum of b <= 16 320 and c2 = sum of (q * b + w), q < 65 536 the word's offset from
    // the chunk origin: < 1.07e9.  The chunk origin's index in the entry enters reduced (bm < 65 521): bm * c1 + c2 < 2^32.  Across
    // chunks the lane keeps 64-bit sums that grow by < 2^32 per chunk, and an entry has fewer than 2^24 chunks.
    // Leaving an entry (or ending), the lanes' sums are reduced mod 65 521, folded per wave by DPP, and lane 63 of each wave adds the
    // wave's pair into the LDS slot of the trip's parity (< 16 * 64 * 65 521 < 2^26) BEFORE the barrier the trip has anyway; behind it
    // thread 0 reduces the slot, sends ONE pair of non-returning 64-bit adds to the entry's record and clears the slot.  The slot of the
    // other parity is the next trip's: a wave that runs ahead into a trip that flushes too (a table of one-chunk entries flushes at
    // every chunk) does not meet thread 0's read, and the trip after that is two barriers away.  No barrier is added.
    if (__builtin_expect(a.mode != VERIFY_TABLE_COMPARE, 0)) { // (laid out behind the verify loop, whose code stays where it was)
        __shared__ uint32_t dg_slot[4]; // [parity][s1, s2]
        struct DView {
            const uint8_t *src0; // the source's chunk origin of the entry
            uint32_t lo, hi;     // global chunks [lo, hi)
            uint32_t lead_rem;   // as the verify loop's
            uint32_t entry;      // bits 0..23: index in the table; bits 24..27: head_n
            uint32_t lane_base;  // per lane; 0 in every lane = the identity keystream
        };
        auto in = [](uint32_t g, const DView &v) { return g - v.lo < v.hi - v.lo; };
        auto search = [&](uint32_t g, DView &v) {
            uint32_t j = 0;
            int k = (int)a.top;
#pragma unroll 1
            do j = table_descend(a.level[k], j, g);
            while (--k >= 0);
            const CycleTablePlan P = *as_const(a.plan + j);
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
        for (int i = 0; i < NB; ++i) vb[i] = DView{nullptr, 0, 0, 0, ~0u, 1};
        // chunk g into one buffer of the ping-pong.  The body's source is 16-byte aligned (the plan laid the grid on it): no funnel.
        // Lanes in front of a cut first chunk's body wrap past num_records: dropped, and masked in the sums.
        auto load = [&](u32x4(&w)[U], DView &v, const DView &prev, uint32_t g) {
            if (g < total && !in(g, v)) {
                if (in(g, prev)) v = prev;
                else search(g, v);
            }
            const Span s = span(g, v);
            const auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(v.src0 + s.off + s.cut), 0, (int)s.bytes, 0x00020000);
#pragma unroll
            for (int u = 0; u < U; ++u) w[u] = __builtin_amdgcn_raw_buffer_load_b128(r, voff + u * SUB - s.cut, 0, AUX_NT);
        };

        unsigned long long a1 = 0ull, a2 = 0ull; // the lane's sums over the entry its workgroup is in
        const DotWeights wt = dot_weights();
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
        // chunk g of view v; g_next (view `next`) is the chunk the workgroup sums after it; `par` = trip & 1
        auto sum = [&](u32x4(&w)[U], const DView &v, uint32_t g, const DView &next, uint32_t g_next, uint32_t par) {
            const Span s = span(g, v);
            const uint32_t c = g - v.lo; // < 2^24
            u32x4 d[U];
            if (__builtin_amdgcn_readfirstlane((int)v.lane_base) != 0) {
                uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
                p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
                uint32_t st = mulmod_canon(v.lane_base, p);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    d[u] = cycle_word<ALG>(w[u], st);
                    if (u + 1 < U) st = mulmod_canon(st, lcg::kTileLo.v[BLOCK / 256]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) d[u] = w[u];
            }
            // index in the entry of the byte at the chunk's origin, mod 65 521: head_n - lead + CHUNK * c, CHUNK mod 65 521 = 15
            const uint32_t lead = v.lead_rem & 0xFFFFu;
            const uint32_t idxm = ((v.entry >> 24) + 2u * kDigestTableMod - lead) % kDigestTableMod;
            const uint32_t bm = (idxm + (CHUNK % kDigestTableMod) * c) % kDigestTableMod;
            uint32_t c1 = 0u, c2 = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = voff + (uint32_t)u * SUB;
                uint32_t b, ws;
                word_sums(d[u], wt, b, ws);
                // a lane outside the chunk's bytes read zeros: its d is the keystream, not output
                const bool inside = q - s.cut < s.bytes;
                b = inside ? b : 0u;
                ws = inside ? ws : 0u;
                c1 += b;
                c2 += q * b + ws;
            }
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
                asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * par), "v"(pending) : "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
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
            return (uint32_t)PREFIX * G + (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        };
        uint32_t cq[NB];
        static_assert(NB == 2 && DEPTH == 1 && PREFIX == NB, "the unrolled trip's position is the mailbox slot's and the sums' slot's parity");
#pragma unroll
        for (int i = 0; i < NB; ++i) cq[i] = blk + (uint32_t)i * G;
        if (cq[0] < total) {
            u32x4 w[NB][U];
            load(w[0], vb[0], vb[1], cq[0]);
            bool finished = false;
            while (!finished) {
#pragma unroll
                for (int p = 0; p < NB; ++p) {
                    __builtin_amdgcn_s_barrier();
                    if (tid == 0) pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    load(w[(p + DEPTH) % NB], vb[(p + DEPTH) % NB], vb[p], cq[DEPTH]);
                    __builtin_amdgcn_sched_barrier(0);
                    sum(w[p], vb[p], cq[0], vb[(p + DEPTH) % NB], cq[DEPTH], (uint32_t)p);
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
        const uint8_t *exp0; // the comparand's chunk origin of the entry
        const uint8_t *src0; // the source byte that pairs with it
        uint32_t lo, hi;    // global chunks [lo, hi) are the entry's chunks 0 .. hi - lo - 1
        uint32_t lead_rem;  // bits 0..15: lead; bits 16..31: bytes of the last chunk, counted from its chunk origin (1 .. CHUNK), less 1
        uint32_t entry;        // bits 0..23: its index in the table (where its result is); bits 24..27: head_n
        uint32_t lane_base;    // per lane: state of this lane's word 0 in the entry's chunk 0; 0 in every lane = the identity keystream
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
        const CycleTablePlan P = *as_const(a.plan + j);
        v.exp0 = P.dst_origin;
        v.src0 = P.src_origin;
        v.lead_rem = table_lead_rem(P);
        v.lo = (uint32_t)P.start;
        v.hi = (uint32_t)P.start + P.chunks;
        v.entry = j | (P.head_n << 24);
        v.lane_base = mulmod_canon(P.base, lane_mul);
    };
    // where chunk g lies: offset of its chunk from the entry's origin, the cut in front of the body (chunk 0 only), its bytes
    auto span = [&](uint32_t g, const View &v) { return table_span_packed<CHUNK>(g, total, v); };
    View vb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) vb[i] = View{nullptr, nullptr, 0, 0, 0, ~0u, 1};
    // chunk g, both sides, into one buffer of the ping-pong; `prev` is the view of the chunk loaded before it
    auto load = [&](Raw(&w)[U], u32x4(&e)[U], View &v, const View &prev, uint32_t g) {
        if (g < total && !in(g, v)) {
            if (in(g, prev)) v = prev;
            else search(g, v);
        }
        const Span s = span(g, v);
        const uint8_t *p = v.src0 + s.off + s.cut;
        const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
        // the extra dword of the last word is the aligned dword that holds the body's last source byte: num_records grows by 4
        const auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p - sh), 0, (int)(s.bytes + (sh && s.bytes ? 4u : 0u)), 0x00020000);
        const auto re = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(v.exp0 + s.off + s.cut), 0, (int)s.bytes, 0x00020000);
        // (lanes in front of a cut first chunk's body wrap past num_records: dropped on both sides, and masked in the compare)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            w[u].d = __builtin_amdgcn_raw_buffer_load_b128(r, voff + u * SUB - s.cut, 0, AUX_NT);
            e[u] = __builtin_amdgcn_raw_buffer_load_b128(re, voff + u * SUB - s.cut, 0, AUX_NT);
        }
        if (sh) {
#pragma unroll
            for (int u = 0; u < U; ++u) w[u].e = __builtin_amdgcn_raw_buffer_load_b32(r, voff + u * SUB - s.cut + lcg::WORD, 0, AUX_NT);
        }
    };

    // What this lane found in the entry of the chunks compared since the last flush.
    Found f{0u, kVerifyNone};
    // The workgroup leaves an entry (uniform: every wave comes here at the same chunk): each wave flushes for itself, with no barrier.
    // (The summary is the line behind the header: a.sum.)
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
                VerifyTableSummary *sum = reinterpret_cast<VerifyTableSummary *>(a.hdr + 1); // (the line behind the header: a.sum)
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
    // chunk g of view v; g_next (already located: view `next`) is the chunk the workgroup compares after it; `par` = trip & 1
    auto compare = [&](Raw(&w)[U], u32x4(&e)[U], const View &v, uint32_t g, const View &next, uint32_t g_next, uint32_t par) {
        const Span s = span(g, v);
        const uint32_t sh = (uint32_t)(uintptr_t)(v.src0 + s.off + s.cut) & 3u;
        // the keystream only where the key is not the identity (a uniform branch); the funnel's shift is 0 for a dword-aligned source
        u32x4 x[U];
        if (__builtin_amdgcn_readfirstlane((int)v.lane_base) != 0) {
            const uint32_t c = g - v.lo;
            uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
            p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
            uint32_t st = mulmod_canon(v.lane_base, p);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u] = cycle_word<ALG>(funnel(w[u], sh), st);
                if (u + 1 < U) st = mulmod_canon(st, lcg::kTileLo.v[BLOCK / 256]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = funnel(w[u], sh);
        }
        uint32_t acc = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // a lane outside the chunk's bytes read nothing on either side: its x is the keystream, not a finding
            const uint32_t inside = voff + (uint32_t)u * SUB - s.cut < s.bytes ? ~0u : 0u;
            x[u] = (x[u] ^ e[u]) & inside;
            acc |= any_bits(x[u]);
        }
        // index in the entry of the byte at the chunk's origin: head_n + chunk offset - lead, modulo 2^64
        const uint64_t idx0 = (uint64_t)(v.entry >> 24) + s.off - (v.lead_rem & 0xFFFFu);
        // clean data costs the ORs above and this test; the rest is for the waves that have something to report
        if (__builtin_amdgcn_ballot_w64(acc != 0u) != 0ull) {
            uint32_t low = ~0u; // (positions in a chunk are below 2^16; 64 bits only once, below)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (any_bits(x[u]) != 0u) note_word(f.cnt, low, x[u], voff + (uint32_t)u * SUB);
            if (low != ~0u) {
                const unsigned long long j = idx0 + low;
                f.first = j < f.first ? j : f.first;
            }
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
        u32x4 e[NB][U];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) load(w[i], e[i], vb[i], vb[(i + NB - 1) % NB], cq[i]);
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                __builtin_amdgcn_s_barrier();
                if (tid == 0) pending = __hip_atomic_fetch_add(&a.hdr->ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                load(w[(p + DEPTH) % NB], e[(p + DEPTH) % NB], vb[(p + DEPTH) % NB], vb[p], cq[DEPTH]);
                __builtin_amdgcn_sched_barrier(0);
                compare(w[p], e[p], vb[p], cq[0], vb[(p + DEPTH) % NB], cq[DEPTH], (uint32_t)p);
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
template <int U, int BLOCK> struct VerifyTableShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const VerifyTableArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_verify_table_kernel<U, BLOCK>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() { return table_kernel_name<U, BLOCK>("modgpu_cycle_verify_table_kernel"); }
};
using VerifyTableStream = VerifyTableShape<4, 1024>; // the verify kernel's shape: 64 KiB chunks
static_assert(VerifyTableStream::chunk == kChunk, "one chunk size for the plan and the stream");
} // namespace

uint32_t modgpu_verify_table_chunk_bytes() { return VerifyTableStream::chunk; }
uint32_t modgpu_verify_table_block() { return VerifyTableStream::block; }
const char *modgpu_verify_table_kernel_name() { return VerifyTableStream::name(); }
hipError_t modgpu_launch_verify_table_plan(const VerifyTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_verify_table_plan, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_verify_table_finish(const VerifyTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(modgpu_cycle_verify_table_finish, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
hipError_t modgpu_launch_verify_table_stream(const VerifyTableArgs &a, uint32_t grid, hipStream_t stream)
{
    VerifyTableStream::launch(a, grid, stream);
    return hipGetLastError();
}
// the digest table call: the same kernels, the mode set
namespace {
VerifyTableArgs digest_mode(const VerifyTableArgs &a)
{
    VerifyTableArgs d = a;
    d.mode = VERIFY_TABLE_DIGEST;
    return d;
}
} // namespace
hipError_t modgpu_launch_digest_table_plan(const VerifyTableArgs &a, hipStream_t stream) { return modgpu_launch_verify_table_plan(digest_mode(a), stream); }
hipError_t modgpu_launch_digest_table_finish(const VerifyTableArgs &a, hipStream_t stream) { return modgpu_launch_verify_table_finish(digest_mode(a), stream); }
hipError_t modgpu_launch_digest_table_stream(const VerifyTableArgs &a, uint32_t grid, hipStream_t stream)
{
    return modgpu_launch_verify_table_stream(digest_mode(a), grid, stream);
}
// the digest check: the finish kernel alone, in its check mode
hipError_t modgpu_launch_digest_check(const DigestTableRecord *records, const uint32_t *expect, uint64_t n, const CycleTableHdr *producer,
                                      CycleVerifyResult *summary, unsigned long long *bad_bits, hipStream_t stream)
{
    VerifyTableArgs a{};
    a.n = n;
    a.n_blk = (uint32_t)((n + kTableBlock - 1) / kTableBlock);
    a.mode = VERIFY_TABLE_CHECK;
    a.records = const_cast<DigestTableRecord *>(records); // (only read)
    a.expect = expect;
    a.bad_bits = bad_bits;
    a.producer = producer;
    a.check = summary;
    hipLaunchKernelGGL(modgpu_cycle_verify_table_finish, dim3(a.n_blk), dim3(kTableBlock), 0, stream, a);
    return hipGetLastError();
}
