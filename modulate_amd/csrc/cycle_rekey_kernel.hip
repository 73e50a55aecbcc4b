// cycle_rekey_kernel.hip -- REKEY in one pass over HBM: dst[j] = src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j] (read
// src once, write dst once, the plaintext only in registers).  The two-keystream block: cycle_rekey_impl.h; the jump tables and the
// single-state arithmetic: cycle_kernel_impl.h, included and not changed.
//
// Shape: the out-of-place kernel's (cycle_to_kernel.hip) -- persistent 1024-thread workgroups, 64 KiB chunks on absolute chunk-aligned
// DESTINATION addresses handed out by tickets from the work-queue ring with a static prefix of two, a ping-pong load pipeline,
// workgroup-synchronous bursts, nt loads and nt sc1 stores, a source of any phase read through the v_alignbyte_b32 funnel, every
// entry's ragged edges and its cut first chunk done before the stream starts, the table of entries in the kernel arguments.  What
// differs: every lane-word carries TWO states, one per keystream.  Both count positions from the same chunk origin, so a chunk's jump
// (a^(CHUNK*c), three table lookups) and a lane's (a^(16*lane)) are shared and each state costs one more multiply; offsets that differ
// in any way -- other phases mod 16 included -- only change the two base states the host computes.
// The keystream arithmetic doubles, so the pass may be bound by VALU issue rather than by HBM; the grid is the host's choice
// (cycle_rekey_kernel.h: the work-queue kernel's 200 workgroups, or one per CU on all 256; DESIGN.md 4.7 has the A/B).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_impl.h"
#include "cycle_rekey_kernel.h"

#include <cstdio>

namespace {

// < 16 bytes before / after an entry's aligned destination body, bytewise, by 32 lanes of one workgroup
__device__ __forceinline__ void rekey_edges(const CycleRekeyPart &P, uint64_t body_bytes, uint32_t tid)
{
    if (tid < P.head_n) {
        uint32_t sa = P.base_head[0], sb = P.base_head[1];
        for (uint32_t j = 0; j < tid; ++j) {
            sa = mulmod_canon(sa, lcg::A);
            sb = mulmod_canon(sb, lcg::A);
        }
        (P.dst_body - P.head_n)[tid] = rekey_byte((P.src_body - P.head_n)[tid], sa, sb);
    } else if (tid >= 16 && tid < 32 && tid - 16 < P.tail_n) {
        const uint32_t t = tid - 16;
        uint32_t sa = P.base_tail[0], sb = P.base_tail[1];
        for (uint32_t j = 0; j < t; ++j) {
            sa = mulmod_canon(sa, lcg::A);
            sb = mulmod_canon(sb, lcg::A);
        }
        P.dst_body[body_bytes + t] = rekey_byte(P.src_body[body_bytes + t], sa, sb);
    }
}

// The source side of one chunk (the out-of-place kernel's reader, cycle_to_kernel.hip):
//   plain   descriptor based at the source's own address, whose phase differs from the destination's by whole dwords
//   funnel  descriptor based at the dword below it, `sh` = that distance (1..3); a dwordx4 and the dword after it per lane-word,
//           joined with v_alignbyte_b32.  The extra dword of the last word is the aligned dword that holds the body's last source
//           byte, so num_records grows by 4 whenever sh != 0 and never reaches past the source's own dwords.
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
__global__ __launch_bounds__(BLOCK) MODGPU_REKEY_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_rekey_kernel(CycleRekeyArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
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

    // edges and cut first chunk of entry p: workgroup p, before the stream starts (cold code)
    for (uint32_t p = blk; p < n_parts; p += G) {
        const CycleRekeyPart &P = a.part[p];
        const uint64_t body_bytes = P.end - P.lead;
        if (tid < 32) rekey_edges(P, body_bytes, tid);
        if (P.lead != 0 && body_bytes != 0) {
            const uint32_t inside = (uint32_t)(P.end < CHUNK ? body_bytes : CHUNK - P.lead);
            auto rd = __builtin_amdgcn_make_buffer_rsrc(P.dst_body, 0, (int)inside, 0x00020000);
            const SrcRsrc rs = src_rsrc<FUNNEL>(P.src_body, inside);
            uint32_t sa = mulmod_canon(P.base_body[0], lane_mul), sb = mulmod_canon(P.base_body[1], lane_mul);
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)U; ++u) {
                const uint32_t o = voff + u * SUB - P.lead; // lanes in front of the body wrap past num_records: dropped
                Raw w;
                load_src<FUNNEL>(w, rs, o);
                const u32x4 d = rekey_word(src_word<FUNNEL>(w, rs.sh), sa, sb);
                __builtin_amdgcn_raw_buffer_store_b128(d, rd, o, 0, SAUX);
                sa = mulmod_canon(sa, lcg::kTileLo.v[BLOCK / 256]);
                sb = mulmod_canon(sb, lcg::kTileLo.v[BLOCK / 256]);
            }
        }
    }

    struct View {
        uint8_t *origin;           // dst_body - lead
        const uint8_t *src_origin; // src_body - lead
        uint64_t end;
        uint32_t lo, hi;
        uint32_t first;
        uint32_t lane_base[2];
    };
    auto locate = [&](uint32_t g, View &v) {
        if (g - v.lo < v.hi - v.lo) return;
        uint32_t p = 0;
#pragma unroll 1
        for (uint32_t i = 1; i < n_parts; ++i) p += g >= a.start[i] ? 1u : 0u;
        const CycleRekeyPart &P = a.part[p];
        v.origin = P.dst_body - P.lead;
        v.src_origin = P.src_body - P.lead;
        v.end = P.end;
        v.first = P.lead != 0 ? 1u : 0u;
        v.lo = a.start[p];
        v.hi = a.start[p + 1];
        v.lane_base[0] = mulmod_canon(P.base_body[0], lane_mul);
        v.lane_base[1] = mulmod_canon(P.base_body[1], lane_mul);
    };
    auto chunk_off = [&](uint32_t g, const View &v) { return (uint64_t)(v.first + (g - v.lo)) * CHUNK; };
    auto chunk_left = [&](uint32_t g, const View &v) {
        const uint64_t o = chunk_off(g, v);
        const uint64_t left = g < v.hi && o < v.end ? v.end - o : 0; // past the last entry: zero-size descriptors
        return (uint32_t)(left < CHUNK ? left : CHUNK);
    };
    // both keystreams' states of this lane's U words: one chunk jump, shared
    auto states = [&](uint32_t g, const View &v, uint32_t(&sa)[U], uint32_t(&sb)[U]) {
        const uint32_t c = v.first + (g - v.lo);
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        sa[0] = mulmod_canon(v.lane_base[0], p);
        sb[0] = mulmod_canon(v.lane_base[1], p);
#pragma unroll
        for (int u = 1; u < U; ++u) {
            sa[u] = mulmod_canon(sa[u - 1], lcg::kTileLo.v[BLOCK / 256]);
            sb[u] = mulmod_canon(sb[u - 1], lcg::kTileLo.v[BLOCK / 256]);
        }
    };
    View vl{nullptr, nullptr, 0, 0, 0, 0, {1, 1}}, vs{nullptr, nullptr, 0, 0, 0, 0, {1, 1}}; // load side, store side
    auto load = [&](Raw(&w)[U], uint32_t g) {
        locate(g, vl);
        const SrcRsrc rs = src_rsrc<FUNNEL>(vl.src_origin + chunk_off(g, vl), chunk_left(g, vl));
#pragma unroll
        for (int u = 0; u < U; ++u) load_src<FUNNEL>(w[u], rs, voff + u * SUB);
    };
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
        uint32_t sa[U], sb[U];
        states(g, vs, sa, sb);
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = rekey_word(src_word<FUNNEL>(w[u], sh), sa[u], sb[u]);
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

    // ---- the MOVE loop (cycle_rekey_kernel.h): the destination partly overlaps the source.  The stream loop's pipeline with two things
    // added per chunk, both between the moment its source is in registers and its stores: the chunk's "loaded" flag goes up, and the
    // flags of the chunks whose source reads meet this chunk's destination are waited for.  The hazard is write-after-read only: no
    // reader needs a byte another workgroup wrote, so only the flags need agent scope, and nothing needs a fence -- the loads a flag
    // speaks for have RETURNED when it is stored (their data went through the two-keystream block in front of the barrier), and the
    // stores it permits are issued behind the poll (a release fence would only drain wave 0's loads of the NEXT chunk).
    // Positions are tickets only, drawn in rising order, the first two where the workgroup starts: whoever holds a position is running, a position waits for
    // lower ones only, so the lowest unfinished position is never blocked -- whether or not the whole grid is resident.
    __shared__ uint32_t q_dead; // the wait ran out: this workgroup stores nothing more (it still loads, flags and draws tickets)
    const uint32_t q_dead_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_dead;
    auto chunk_at = [&](uint32_t p) { return a.move_down != 0 && p < total ? total - 1u - p : p; };
    auto flag_up = [&](const uint32_t *f) { // thread 0; false: gave up
        if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
        const uint32_t t0 = (uint32_t)wall_clock64(); // (the bound fits 32 bits: the low word's difference is enough)
        do {
            __builtin_amdgcn_s_sleep(8);
            if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
        } while ((uint32_t)wall_clock64() - t0 < (uint32_t)kRekeyMoveStallTicks);
        return false;
    };
    // (one entry, lead 0, no edges: the views of the stream loop shrink to the entry's three words, which saves their scalar registers)
    const CycleRekeyPart &M = a.part[0];
    auto move_left = [&](uint32_t g) {
        const uint64_t o = (uint64_t)g * CHUNK;
        const uint64_t left = g < total && o < M.end ? M.end - o : 0; // past the end: zero-size descriptors
        return (uint32_t)(left < CHUNK ? left : CHUNK);
    };
    auto load_move = [&](Raw(&w)[U], uint32_t g) {
        const SrcRsrc rs = src_rsrc<FUNNEL>(M.src_body + (uint64_t)g * CHUNK, move_left(g));
#pragma unroll
        for (int u = 0; u < U; ++u) load_src<FUNNEL>(w[u], rs, voff + u * SUB);
    };
    auto process_move = [&](Raw(&w)[U], uint32_t g) {
        auto r = __builtin_amdgcn_make_buffer_rsrc(M.dst_body + (uint64_t)g * CHUNK, 0, (int)move_left(g), 0x00020000);
        const uint32_t sh = FUNNEL ? (uint32_t)(uintptr_t)M.src_body & 3u : 0u; // (CHUNK is a multiple of 4)
        uint32_t sa[U], sb[U];
        states(g, vs, sa, sb); // (of vs only lo, first and the lane's bases: set where the loop starts)
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = rekey_word(src_word<FUNNEL>(w[u], sh), sa[u], sb[u]);
        // every wave waits HERE until this chunk's loads have returned: the only vector-memory instructions younger than them are the
        // next chunk's loads (U, twice that in the funnel form).  The blocks above consume the data, so the compiler's own waits say
        // the same; this one does not depend on where an optimiser leaves them (check_isa.py pins it in front of the barrier).
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(FUNNEL ? 2 * U : U) : "memory");
        if (tid == 0)
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * (trip & 1u)), "v"(pending) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier(); // every wave has this chunk's source in registers
        if (tid == 0 && g < total) {
            __hip_atomic_store(a.move_flags + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t dead;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(dead) : "v"(q_dead_lds) : "memory");
#pragma unroll 1
            for (uint32_t i = 0; i < a.move_win_n && dead == 0; ++i) {
                const uint32_t k = g + (uint32_t)a.move_win_lo + i; // (below chunk 0: wraps past total)
                if (k < total && !flag_up(a.move_flags + k)) {
                    atomicCAS(a.move_status, 0u, 1u + g);
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
            for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB, 0, SAUX);
        }
        ++trip;
    };

    uint32_t cq[NB];
    static_assert(PREFIX == NB, "the static positions are exactly the ones cq[] starts with");
    if (a.move_flags != nullptr) {
        // the first DEPTH + 1 positions: one fetch EACH, a barrier apart.  (One fetch of two would give a workgroup two CONSECUTIVE
        // positions; with a shift below a chunk, position p waits for p - 1's flag, which goes up only once its workgroup has stored the
        // position before it -- every workgroup's first store would wait for its neighbour's, a chain as long as the grid (DESIGN.md
        // 4.14 has the figures).  A barrier apart, the other workgroups' first fetches come in between.)
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (tid == 0) {
                pending = __hip_atomic_fetch_add(a.queue, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %2, %3\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * ((uint32_t)(i + 1) & 1u)), "v"(pending), "v"(q_dead_lds), "v"(0u) : "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            uint32_t t;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * ((uint32_t)(i + 1) & 1u)) : "memory");
            cq[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        }
        if (cq[0] < total) {
            vs.lane_base[0] = mulmod_canon(M.base_body[0], lane_mul);
            vs.lane_base[1] = mulmod_canon(M.base_body[1], lane_mul);
            Raw w[NB][U];
#pragma unroll
            for (int i = 0; i < DEPTH; ++i) load_move(w[i], chunk_at(cq[i]));
            bool finished = false;
            while (!finished) {
#pragma unroll
                for (int p = 0; p < NB; ++p) {
                    __builtin_amdgcn_s_barrier();
                    if (tid == 0) pending = __hip_atomic_fetch_add(a.queue, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    load_move(w[(p + DEPTH) % NB], chunk_at(cq[DEPTH]));
                    __builtin_amdgcn_sched_barrier(0);
                    process_move(w[p], chunk_at(cq[0]));
#pragma unroll
                    for (int i = 0; i < DEPTH; ++i) cq[i] = cq[i + 1];
                    cq[DEPTH] = take_published() - (uint32_t)PREFIX * G; // tickets ARE positions here
                    if (cq[0] >= total) {
                        finished = true;
                        break;
                    }
                }
            }
        }
    } else {
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
    } // (the stream loop keeps its indentation: it is the out-of-place kernel's, line for line)
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
template <int U, int BLOCK, bool FUNNEL> struct RekeyShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const CycleRekeyArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_rekey_kernel<U, BLOCK, FUNNEL>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() // as a profiler prints it
    {
        static char buf[96];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_rekey_kernel<%d, %d, %s>", U, BLOCK, FUNNEL ? "true" : "false");
        (void)n;
        return buf;
    }
};
// the out-of-place kernel's shape (1024 threads x 4 words = 64 KiB chunks): its chunk grid, tables and ticket ring are shared
using RekeyPlain = RekeyShape<4, 1024, false>;
using RekeyFunnel = RekeyShape<4, 1024, true>;
static_assert(RekeyPlain::chunk == RekeyFunnel::chunk, "one chunk size for both forms");
} // namespace

uint32_t modgpu_rekey_chunk_bytes() { return RekeyPlain::chunk; }
uint32_t modgpu_rekey_block() { return RekeyPlain::block; }
const char *modgpu_rekey_kernel_name(int form) { return form == CYCLE_REKEY_FUNNEL ? RekeyFunnel::name() : RekeyPlain::name(); }
hipError_t modgpu_launch_cycle_rekey(const CycleRekeyArgs &a, int form, uint32_t grid, hipStream_t stream)
{
    if (form == CYCLE_REKEY_FUNNEL) RekeyFunnel::launch(a, grid, stream);
    else RekeyPlain::launch(a, grid, stream);
    return hipGetLastError();
}
hipError_t modgpu_launch_cycle_rekey_move(const CycleRekeyArgs &a, int form, uint32_t *grid, hipStream_t stream)
{
    int per_cu = 0, cus = 0, dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess)
        e = form == CYCLE_REKEY_FUNNEL ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, modgpu_cycle_rekey_kernel<4, 1024, true>, 1024, 0)
                                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, modgpu_cycle_rekey_kernel<4, 1024, false>, 1024, 0);
    if (e != hipSuccess) return e;
    const uint64_t resident = (uint64_t)(per_cu > 0 ? per_cu : 1) * (uint64_t)(cus > 0 ? cus : 1);
    if (*grid > resident) *grid = (uint32_t)resident;
    if (*grid == 0) *grid = 1;
    return modgpu_launch_cycle_rekey(a, form, *grid, stream);
}
