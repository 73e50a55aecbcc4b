// cycle_to_kernel.hip -- the out-of-place form of the work-queue kernel: dst[j] = src[j] ^ ks[stream_off + j] in ONE pass over
// HBM (read src once, write dst once), src left intact.  Device code of the arithmetic, the jump tables and the keystream block:
// cycle_kernel_impl.h, included and not changed (its hash is modgpu_kernel_source_hash; this TU has its own).
//
// Shape: modgpu_cycle_queue_kernel's (cycle_kernel_impl.h has the reasoning) -- persistent 1024-thread workgroups, 64 KiB chunks on
// absolute chunk-aligned addresses handed out by a ticket counter with a static prefix of two, a ping-pong load pipeline,
// workgroup-synchronous bursts, nt loads and nt sc1 stores, the table of entries in the kernel arguments.  What differs:
//   * the chunk grid is laid on the DESTINATION (stores are whole aligned lines); the source of a chunk is the same span shifted by
//     (src - dst), which may have any byte phase;
//   * every entry's ragged edges (< 16 bytes) and its cut first chunk read the source and write the destination;
//   * no helper workgroups (optional per the design: the out-of-place pass is not the one the roofline is tuned on).
// Source descriptors are sized so that a lane's 16-byte body word never straddles num_records: the hardware range check only ever
// drops whole lanes past a ragged end, as in the in-place kernel.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel_impl.h"
#include "cycle_to_kernel.h"

#include <cstdio>

namespace {

// < 16 bytes before / after an entry's aligned destination body, bytewise, by 32 lanes of one workgroup
__device__ __forceinline__ void cycle_edges_to(const CycleToPart &P, uint64_t body_bytes, uint32_t tid)
{
    if (tid < P.head_n) {
        uint32_t s = P.base_head;
        for (uint32_t j = 0; j < tid; ++j) s = mulmod_canon(s, lcg::A);
        (P.dst_body - P.head_n)[tid] = cycle_byte((P.src_body - P.head_n)[tid], s);
    } else if (tid >= 16 && tid < 32 && tid - 16 < P.tail_n) {
        const uint32_t t = tid - 16;
        uint32_t s = P.base_tail;
        for (uint32_t j = 0; j < t; ++j) s = mulmod_canon(s, lcg::A);
        P.dst_body[body_bytes + t] = cycle_byte(P.src_body[body_bytes + t], s);
    }
}

// The source side of one chunk: a descriptor and, for the funnel form, the byte shift inside a dword.
//   plain   descriptor based at the source's own address (any phase); one dwordx4 per lane-word
//   funnel  descriptor based at the dword below it, `sh` = that distance (0..3); a dwordx4 and the dword after it per lane-word,
//           joined with v_alignbyte_b32.  The extra dword of the last word is the aligned dword that holds the body's last
//           source byte, so num_records grows by 4 whenever sh != 0 and never reaches past the source's own dwords.
struct SrcRsrc {
    __amdgpu_buffer_rsrc_t r;
    uint32_t sh;
};
template <bool FUNNEL> __device__ __forceinline__ SrcRsrc src_rsrc(const uint8_t *p, uint32_t bytes)
{
    if constexpr (FUNNEL) {
        const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
        // (an empty span -- a chunk past the last entry -- keeps num_records 0: nothing of it is read)
        return {__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p - sh), 0, (int)(bytes + (sh && bytes ? 4u : 0u)), 0x00020000), sh};
    } else {
        return {__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p), 0, (int)bytes, 0x00020000), 0u};
    }
}
struct Raw {
    u32x4 d;
    uint32_t e; // funnel form: the dword after d
};
template <bool FUNNEL> __device__ __forceinline__ void load_src(Raw &w, const SrcRsrc &s, uint32_t o)
{
    w.d = __builtin_amdgcn_raw_buffer_load_b128(s.r, o, 0, AUX_NT);
    if constexpr (FUNNEL) w.e = __builtin_amdgcn_raw_buffer_load_b32(s.r, o + lcg::WORD, 0, AUX_NT);
}
template <bool FUNNEL> __device__ __forceinline__ u32x4 src_word(const Raw &w, uint32_t sh)
{
    if constexpr (!FUNNEL) {
        return w.d;
    } else {
        u32x4 d;
        d.x = __builtin_amdgcn_alignbyte(w.d.y, w.d.x, sh);
        d.y = __builtin_amdgcn_alignbyte(w.d.z, w.d.y, sh);
        d.z = __builtin_amdgcn_alignbyte(w.d.w, w.d.z, sh);
        d.w = __builtin_amdgcn_alignbyte(w.e, w.d.w, sh);
        return d;
    }
}

} // namespace

template <int U, int BLOCK, bool FUNNEL>
__global__ __launch_bounds__(BLOCK) MODGPU_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_to_kernel(CycleToArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr int ALG = 2;                 // the three-instruction keystream (ks_word_carry)
    constexpr int SAUX = AUX_SC1 | AUX_NT; // stores: write-through, streaming
    constexpr int DEPTH = 1;               // chunks of loads in flight ahead of the one being computed
    constexpr uint32_t CHUNK = (uint32_t)U * BLOCK * lcg::WORD;
    constexpr uint32_t SUB = BLOCK * lcg::WORD;
    constexpr int NB = DEPTH + 1;
    constexpr int PREFIX = DEPTH + 1; // static chunks per workgroup (b, b+G); then tickets
    const uint32_t tid = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    const uint32_t G = gridDim.x;
    const uint32_t n_parts = a.n_parts;
    const uint32_t total = a.start[kCycleBatchMax];
    __shared__ uint32_t q_next[2]; // ticket mailbox, two words used alternately (modgpu_cycle_queue_kernel says why)
    uint32_t trip = 0;
    const uint32_t voff = tid * lcg::WORD;
    const uint32_t lane_mul = mulmod_canon(c_tile_lo.v[tid >> 8], c_lane_pow.v[tid & 255]);

    struct View {
        uint8_t *origin;           // dst_body - lead
        const uint8_t *src_origin; // src_body - lead
        uint64_t end;
        uint32_t lo, hi;
        uint32_t first;
        uint32_t lane_base;
        uint32_t part; // the entry's index (the digest loop looks its record up by it)
    };
    auto locate = [&](uint32_t g, View &v) {
        if (g - v.lo < v.hi - v.lo) return;
        uint32_t p = 0;
#pragma unroll 1
        for (uint32_t i = 1; i < n_parts; ++i) p += g >= a.start[i] ? 1u : 0u;
        const CycleToPart &P = a.part[p];
        v.origin = P.dst_body - P.lead;
        v.src_origin = P.src_body - P.lead;
        v.end = P.end;
        v.first = P.lead != 0 ? 1u : 0u;
        v.lo = a.start[p];
        v.hi = a.start[p + 1];
        v.lane_base = mulmod_canon(P.base_body, lane_mul);
        v.part = p;
    };
    auto chunk_off = [&](uint32_t g, const View &v) { return (uint64_t)(v.first + (g - v.lo)) * CHUNK; };
    auto chunk_left = [&](uint32_t g, const View &v) {
        const uint64_t o = chunk_off(g, v);
        const uint64_t left = g < v.hi && o < v.end ? v.end - o : 0; // past the last entry: zero-size descriptors
        return (uint32_t)(left < CHUNK ? left : CHUNK);
    };
    auto states = [&](uint32_t g, const View &v, uint32_t(&s)[U]) {
        const uint32_t c = v.first + (g - v.lo);
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        s[0] = mulmod_canon(v.lane_base, p);
#pragma unroll
        for (int u = 1; u < U; ++u) s[u] = mulmod_canon(s[u - 1], lcg::kTileLo.v[BLOCK / 256]);
    };
    View vl{nullptr, nullptr, 0, 0, 0, 0, 1, 0}, vs{nullptr, nullptr, 0, 0, 0, 0, 1, 0}; // load side, store side
    auto load = [&](Raw(&w)[U], uint32_t g) {
        locate(g, vl);
        const SrcRsrc rs = src_rsrc<FUNNEL>(vl.src_origin + chunk_off(g, vl), chunk_left(g, vl));
#pragma unroll
        for (int u = 0; u < U; ++u) load_src<FUNNEL>(w[u], rs, voff + u * SUB);
    };

    // ---- the digest loop (cycle_to_kernel.h): out is summed -- and, for an entry with a destination, stored exactly as the stream loop
    // stores it.  One uniform branch at the top of the kernel; the stream loop below is not entered.
    // Widths.  A dword's byte sum and position sum are one v_dot4_u32_u8 each (weights 0x01010101; 0x03020100 + 4k for dword k of the
    // word).  Per lane-word b = sum of bytes <= 16 * 255 = 4 080 and w = sum of i * byte_i <= 120 * 255 = 30 600.  Per chunk a lane
    // adds, in 32 bits, c1 = sum of b <= 4 * 4 080 = 16 320 and c2 = sum of (q * b + w), q < 65 536 the word's offset in the chunk:
    // <= 4 * (65 520 * 4 080 + 30 600) < 1.07e9.  The chunk origin's index in the entry enters reduced (bm < 65 521, stepped by
    // CHUNK mod 65 521 per chunk): bm * c1 + c2 < 1.07e9 + 1.07e9 < 2^32.  Across chunks the lane keeps 64-bit sums that grow by
    // < 2^32 per chunk: good for 2^32 chunks per visit of an entry, and an entry has fewer than 2^24.  Leaving an entry, every lane
    // reduces its two sums mod 65 521 and adds them into LDS (32-bit: 1 024 * 65 520 < 2^27); thread 0 reduces again and sends one pair.
    // Through LDS and not per wave: one pair per workgroup instead of sixteen, and a wave fold needs either DPP code of its own or a
    // lane index (v_mbcnt, which this TU's guard reads as a rewritten ticket atomic).
    if (a.digest != 0u) {
        const bool ident = (a.digest & CYCLE_TO_DIGEST_IDENTITY) != 0u;
        __shared__ uint32_t dg_red[2];
        unsigned long long a1 = 0ull, a2 = 0ull; // the lane's sums over the entry its workgroup is in
        if (tid == 0) dg_red[0] = dg_red[1] = 0u;
        __syncthreads();
        // the workgroup leaves an entry (uniform); n_add: the entry's n, from the workgroup that owns its edges
        auto flush = [&](CycleToDigest *res, unsigned long long n_add) {
            const uint32_t r1 = (uint32_t)(a1 % kDigestMod), r2 = (uint32_t)(a2 % kDigestMod);
            if (r1 != 0u) atomicAdd(&dg_red[0], r1);
            if (r2 != 0u) atomicAdd(&dg_red[1], r2);
            a1 = a2 = 0ull;
            __syncthreads();
            if (tid == 0) {
                const unsigned long long t1 = dg_red[0] % kDigestMod, t2 = dg_red[1] % kDigestMod;
                if (t1 != 0ull) __hip_atomic_fetch_add(&res->s1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t2 != 0ull) __hip_atomic_fetch_add(&res->s2, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (n_add != 0ull) __hip_atomic_fetch_add(&res->n, n_add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                dg_red[0] = dg_red[1] = 0u;
            }
            __syncthreads();
        };
        // byte sum and position sum (byte i of the word weighs i) of one 16-byte word
        auto word_sums = [](const u32x4 &d, uint32_t &b, uint32_t &w) {
            b = __builtin_amdgcn_udot4(d.x, 0x01010101u, 0u, false);
            b = __builtin_amdgcn_udot4(d.y, 0x01010101u, b, false);
            b = __builtin_amdgcn_udot4(d.z, 0x01010101u, b, false);
            b = __builtin_amdgcn_udot4(d.w, 0x01010101u, b, false);
            w = __builtin_amdgcn_udot4(d.x, 0x03020100u, 0u, false);
            w = __builtin_amdgcn_udot4(d.y, 0x07060504u, w, false);
            w = __builtin_amdgcn_udot4(d.z, 0x0B0A0908u, w, false);
            w = __builtin_amdgcn_udot4(d.w, 0x0F0E0D0Cu, w, false);
        };

        // edges, cut first chunk and n of entry p: workgroup p, before the stream starts (cold code)
        for (uint32_t p = blk; p < n_parts; p += G) {
            const CycleToPart &P = a.part[p];
            const bool store = ((a.store_mask >> p) & 1u) != 0u;
            const uint64_t body_bytes = P.end - P.lead;
            if (tid < 32) {
                // < 16 bytes before / after the body, bytewise (cycle_edges_to); byte j of the entry weighs j
                const bool head = tid < P.head_n, tail = tid >= 16 && tid - 16 < P.tail_n;
                if (head || tail) {
                    const uint32_t t = head ? tid : tid - 16;
                    const uint64_t at = head ? 0 : body_bytes;               // from the body's start
                    const uint8_t *sp = head ? P.src_body - P.head_n : P.src_body;
                    uint8_t out = sp[at + t];
                    if (!ident) {
                        uint32_t s = head ? P.base_head : P.base_tail;
                        for (uint32_t j = 0; j < t; ++j) s = mulmod_canon(s, lcg::A);
                        out = cycle_byte(out, s);
                    }
                    if (store) (head ? P.dst_body - P.head_n : P.dst_body)[at + t] = out;
                    const uint64_t j = head ? (uint64_t)t : (uint64_t)P.head_n + body_bytes + t;
                    a1 += out;
                    a2 += (j % kDigestMod) * out;
                }
            }
            if (P.lead != 0 && body_bytes != 0) {
                const uint32_t inside = (uint32_t)(P.end < CHUNK ? body_bytes : CHUNK - P.lead);
                auto rd = __builtin_amdgcn_make_buffer_rsrc(P.dst_body, 0, (int)inside, 0x00020000);
                const SrcRsrc rs = src_rsrc<FUNNEL>(P.src_body, inside);
                uint32_t su = ident ? 0u : mulmod_canon(P.base_body, lane_mul);
#pragma unroll 1
                for (uint32_t u = 0; u < (uint32_t)U; ++u) {
                    const uint32_t o = voff + u * SUB - P.lead; // lanes in front of the body wrap past num_records: dropped, and masked below
                    Raw w;
                    load_src<FUNNEL>(w, rs, o);
                    u32x4 d = src_word<FUNNEL>(w, rs.sh);
                    if (!ident) {
                        d = cycle_word<ALG>(d, su);
                        su = mulmod_canon(su, lcg::kTileLo.v[BLOCK / 256]);
                    }
                    if (store) __builtin_amdgcn_raw_buffer_store_b128(d, rd, o, 0, SAUX);
                    if (o < inside) { // (a lane outside read zeros: its d is the keystream, not output)
                        uint32_t b, ws;
                        word_sums(d, b, ws);
                        a1 += b;
                        a2 += (P.head_n + o) * b + ws; // < 65 552 * 4 080 + 30 600: 32 bits
                    }
                }
            }
            flush(a.result[p], (uint64_t)P.head_n + body_bytes + P.tail_n);
        }

        CycleToDigest *res = nullptr; // of the entry the sums are being kept for
        bool store = false;
        uint32_t idxm = 0u; // index in the entry of the byte at the chunk origin (head_n - lead), mod 65 521
        auto sum = [&](Raw(&w)[U], uint32_t g) {
            if (g - vs.lo >= vs.hi - vs.lo) {
                if (res) flush(res, 0ull); // the workgroup moves on to another entry
                locate(g, vs);
                const CycleToPart &P = a.part[vs.part];
                res = a.result[vs.part];
                store = ((a.store_mask >> vs.part) & 1u) != 0u;
                idxm = (P.head_n + kDigestMod - P.lead % kDigestMod) % kDigestMod;
            }
            const uint64_t o = chunk_off(g, vs);
            const uint32_t left = chunk_left(g, vs);
            const uint32_t c = vs.first + (g - vs.lo);                          // < 2^24
            const uint32_t bm = (idxm + (CHUNK % kDigestMod) * c) % kDigestMod; // (CHUNK mod 65 521 = 15: 32 bits hold it)
            const uint32_t sh = FUNNEL ? (uint32_t)(uintptr_t)(vs.src_origin + o) & 3u : 0u;
            u32x4 d[U];
            if (ident) {
#pragma unroll
                for (int u = 0; u < U; ++u) d[u] = src_word<FUNNEL>(w[u], sh);
            } else {
                uint32_t s[U];
                states(g, vs, s);
#pragma unroll
                for (int u = 0; u < U; ++u) d[u] = cycle_word<ALG>(src_word<FUNNEL>(w[u], sh), s[u]);
            }
            if (store) { // (uniform) a workgroup-synchronous burst, as in the stream loop: every wave's stores leave together
                auto r = __builtin_amdgcn_make_buffer_rsrc(vs.origin + o, 0, (int)left, 0x00020000);
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
#pragma unroll
                for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB, 0, SAUX);
            }
            uint32_t c1 = 0u, c2 = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = voff + (uint32_t)u * SUB;
                uint32_t b, ws;
                word_sums(d[u], b, ws);
                // a lane past the ragged end of the entry's last chunk read zeros: its d is the keystream, not output
                const bool in = q < left;
                b = in ? b : 0u;
                ws = in ? ws : 0u;
                c1 += b;
                c2 += q * b + ws;
            }
            a1 += c1;
            a2 += bm * c1 + c2;
        };
        uint32_t g = blk;
        if (g < total) {
            Raw w[2][U];
            load(w[0], g);
            bool finished = false;
            while (!finished) {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    __builtin_amdgcn_s_barrier();
                    load(w[p ^ 1], g + G); // (past the last chunk: zero-size descriptors, nothing is read)
                    __builtin_amdgcn_sched_barrier(0);
                    sum(w[p], g);
                    g += G;
                    if (g >= total) {
                        finished = true;
                        break;
                    }
                }
            }
            flush(res, 0ull);
        }
        return; // no ticket was drawn: nothing to sign off
    }
    // edges and cut first chunk of entry p: workgroup p, before the stream starts (cold code)
    for (uint32_t p = blk; p < n_parts; p += G) {
        const CycleToPart &P = a.part[p];
        const uint64_t body_bytes = P.end - P.lead;
        if (tid < 32) cycle_edges_to(P, body_bytes, tid);
        if (P.lead != 0 && body_bytes != 0) {
            const uint32_t inside = (uint32_t)(P.end < CHUNK ? body_bytes : CHUNK - P.lead);
            auto rd = __builtin_amdgcn_make_buffer_rsrc(P.dst_body, 0, (int)inside, 0x00020000);
            const SrcRsrc rs = src_rsrc<FUNNEL>(P.src_body, inside);
            uint32_t su = mulmod_canon(P.base_body, lane_mul);
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)U; ++u) {
                const uint32_t o = voff + u * SUB - P.lead; // lanes in front of the body wrap past num_records: dropped
                Raw w;
                load_src<FUNNEL>(w, rs, o);
                const u32x4 d = cycle_word<ALG>(src_word<FUNNEL>(w, rs.sh), su);
                __builtin_amdgcn_raw_buffer_store_b128(d, rd, o, 0, SAUX);
                su = mulmod_canon(su, lcg::kTileLo.v[BLOCK / 256]);
            }
        }
    }

    // lane 0's ticket traffic: a plain returning atomic, waited for only where it is published (TU built with
    // -mllvm -amdgpu-atomic-optimizer-strategy=None); the LDS mailbox in ds_ assembly (a volatile C++ access would be FLAT)
    uint32_t pending = 0;
    const uint32_t q_next_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_next[0];
    const uint32_t one = 1u;
    auto process_store = [&](Raw(&w)[U], uint32_t g) {
        locate(g, vs);
        const uint64_t o = chunk_off(g, vs);
        auto r = __builtin_amdgcn_make_buffer_rsrc(vs.origin + o, 0, (int)chunk_left(g, vs), 0x00020000);
        const uint32_t sh = FUNNEL ? (uint32_t)(uintptr_t)(vs.src_origin + o) & 3u : 0u;
        uint32_t s[U];
        states(g, vs, s);
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = cycle_word<ALG>(src_word<FUNNEL>(w[u], sh), s[u]);
        if (tid == 0)
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * (trip & 1u)), "v"(pending) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB, 0, SAUX);
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
        for (int i = 0; i < DEPTH; ++i) load(w[i], cq[i]);
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                __builtin_amdgcn_s_barrier();
                if (tid == 0) pending = __hip_atomic_fetch_add(a.queue, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                load(w[(p + DEPTH) % NB], cq[DEPTH]);
                __builtin_amdgcn_sched_barrier(0);
                process_store(w[p], cq[0]);
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
    // leave: the last workgroup out resets the pair, then signs off in the host-visible word
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(a.queue + 1, 1u) == G - 1) {
            __hip_atomic_store(a.queue, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.queue + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.queue_done) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(a.queue_done, a.queue_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

namespace {
template <int U, int BLOCK, bool FUNNEL> struct ToShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const CycleToArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_to_kernel<U, BLOCK, FUNNEL>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() // as a profiler prints it
    {
        static char buf[96];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_to_kernel<%d, %d, %s>", U, BLOCK, FUNNEL ? "true" : "false");
        (void)n;
        return buf;
    }
};
// the work-queue kernel's measured shape (cycle_kernel.hip: 1024 threads x 4 words = 64 KiB chunks)
using ToPlain = ToShape<4, 1024, false>;
using ToFunnel = ToShape<4, 1024, true>;
static_assert(ToPlain::chunk == ToFunnel::chunk, "one chunk size for both forms");
} // namespace

uint32_t modgpu_to_chunk_bytes() { return ToPlain::chunk; }
uint32_t modgpu_to_block() { return ToPlain::block; }
const char *modgpu_to_kernel_name(int form) { return form == CYCLE_TO_FUNNEL ? ToFunnel::name() : ToPlain::name(); }
hipError_t modgpu_launch_cycle_to(const CycleToArgs &a, int form, uint32_t grid, hipStream_t stream)
{
    if (form == CYCLE_TO_FUNNEL) ToFunnel::launch(a, grid, stream);
    else ToPlain::launch(a, grid, stream);
    return hipGetLastError();
}
hipError_t modgpu_launch_cycle_to_digest(const CycleToArgs &a, int form, uint32_t grid, hipStream_t stream)
{
    CycleToArgs d = a;
    d.digest |= CYCLE_TO_DIGEST_ON;
    return modgpu_launch_cycle_to(d, form, grid, stream);
}
