// cycle_keep_kernel.hip -- the work-queue kernel with a cache policy per chunk: chunks at a fixed, address-derived set of positions
// are stored `sc1` (write-through, allocating in the 256 MiB Infinity Cache), all others `nt sc1` as modgpu_cycle_queue_kernel stores
// every chunk.  The next pass over the same memory -- decrypt after encrypt, a verify or a rekey after a cycle -- then finds the
// resident chunks on-die, loads (`nt`, which hit what is there) and stores alike, while DRAM works on the rest.
//
// The kernel below is a COPY of modgpu_cycle_queue_kernel<U, BLOCK> (cycle_kernel_impl.h, whose text is pinned by
// modgpu_kernel_source_hash and is included here unchanged for the arithmetic, the jump tables and the keystream block): the table of
// up to 16 parts, the helpers, the ticket mailbox, the barriers, the cut first chunk and the edges are the original's, line by line
// (`diff` against it shows the five places that differ).  What differs:
//   * the arguments are CycleKeepArgs: CycleQueueArgs plus keep_mask (a power of two minus one) and keep_run;
//   * a trip's store burst exists twice behind a wave-uniform scalar test, once per trip, of the chunk's absolute address:
//         ((addr >> 16) & keep_mask) < keep_run   ->  AUX_SC1          (resident)
//         otherwise                               ->  AUX_SC1 | AUX_NT (streaming, the original's policy)
//     no division, no per-lane work; keep_run = 0 is the original's policy exactly.
// Loads stay nt everywhere; the cut first chunk and the ragged edges stay streaming.  Residency is a property of the ADDRESS, not of
// the call: a later call over a sub-range, at another stream offset or under another key finds the same lines.
// keep_mask = 255: 64 KiB chunks resident out of every 16 MiB, keep_run of them (a strided slice, spread over the launch); a mask
// as large as the buffer with a large run: one contiguous slice.  DESIGN.md 4.1 / 5 / 10 have the measurement.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel_impl.h"
#include "cycle_keep_kernel.h"

#include <cstdio>

template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) MODGPU_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_keep_kernel(CycleKeepArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr int ALG = 2;                   // the three-instruction keystream (ks_word_carry)
    constexpr int SAUX = AUX_SC1 | AUX_NT;   // stores: write-through, streaming
    constexpr int KAUX = AUX_SC1;            // stores of a RESIDENT chunk: write-through, allocating in the Infinity Cache
    constexpr int DEPTH = 1;                 // chunks of loads in flight ahead of the one being computed
    constexpr uint32_t CHUNK = (uint32_t)U * BLOCK * lcg::WORD;
    constexpr uint32_t SUB = BLOCK * lcg::WORD;
    static_assert(CHUNK == 1u << 16, "the residency test reads the chunk's number off address bits 16 and up");
    constexpr int NB = DEPTH + 1;     // register buffers: one being computed, DEPTH being loaded
    constexpr int PREFIX = DEPTH + 1; // static chunks per workgroup: the ticket fetched in trip j is loaded in trip j + 1 and computed in trip j + PREFIX
    const uint32_t tid = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    const uint32_t G = gridDim.x;
    const uint32_t Gm = a.main_groups != 0 && a.main_groups < G ? a.main_groups : G; // main workgroups; [Gm, G) are helpers (below)
    const uint32_t n_parts = a.n_parts;
    const uint32_t total = a.start[kCycleBatchMax]; // (unused entries of start[] hold the total as well)
    // Two LDS words, used alternately: a trip's ticket is written before that trip's barrier and read after it, and
    // the same word is written again two trips later -- i.e. behind the NEXT trip's barrier, which no wave can reach
    // before it has done this trip's read.  (With a single word, correctness would lean on the other barrier, the
    // one in front of the loads, which is a tuning choice: without it a wave held up between this barrier and its
    // read can be overtaken by lane 0's next write -- tools/tune_cycle's INVALID row shows what that looks like.)
    __shared__ uint32_t q_next[2];
    uint32_t trip = 0;
    const uint32_t voff = tid * lcg::WORD;
    // a^(4096*(tid/256)) * a^(16*(tid%256)): this lane's word 0 relative to the start of any chunk
    const uint32_t lane_mul = mulmod_canon(c_tile_lo.v[tid >> 8], c_lane_pow.v[tid & 255]);

    // Ragged edges (< 16 bytes before / after a part's aligned body) and the part's first chunk when the body is not
    // chunk-aligned: workgroup p does them for part p, before the stream starts (cold code).  Chunks sit on ABSOLUTE
    // chunk-aligned addresses, so that first chunk is cut at the front: descriptor based at the body, per-lane offset minus
    // `lead`; lanes in front of the body get a negative offset, which wraps far past num_records, so the hardware range check
    // drops their loads and stores.  It is not part of the chunk index space.
    for (uint32_t p = blk; p < n_parts; p += G) {
        const CycleQueuePart &P = a.part[p];
        const uint64_t body_bytes = P.end - P.lead;
        if (tid < 32) cycle_edges(P.body - P.head_n, P.head_n, P.base_head, P.body + body_bytes, P.tail_n, P.base_tail, tid);
        if (P.lead != 0 && body_bytes != 0) {
            const uint64_t inside = P.end < CHUNK ? body_bytes : CHUNK - P.lead;
            auto r = __builtin_amdgcn_make_buffer_rsrc(P.body, 0, (int)inside, 0x00020000);
            uint32_t su = mulmod_canon(P.base_body, lane_mul);
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)U; ++u) {
                const uint32_t o = voff + u * SUB - P.lead;
                u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, AUX_NT);
                d = cycle_word<ALG>(d, su);
                __builtin_amdgcn_raw_buffer_store_b128(d, r, o, 0, SAUX);
                su = mulmod_canon(su, lcg::kTileLo.v[BLOCK / 256]);
            }
        }
    }

    // the part a global chunk index lies in, as far as the loop needs it
    struct View {
        uint8_t *origin;    // body - lead
        uint64_t end;
        uint32_t lo, hi;    // global indices [lo, hi) map to the part's chunks first + (g - lo)
        uint32_t first;     // 1 if the part's chunk 0 is the cut one (done above)
        uint32_t lane_base; // per lane: state of this lane's word 0 in the part's chunk 0
    };
    auto locate = [&](uint32_t g, View &v) {
        if (g - v.lo < v.hi - v.lo) return; // lo <= g < hi
        uint32_t p = 0;
#pragma unroll 1
        for (uint32_t i = 1; i < n_parts; ++i) p += g >= a.start[i] ? 1u : 0u; // (empty parts share their start with the next one: skipped)
        const CycleQueuePart &P = a.part[p];
        v.origin = P.body - P.lead;
        v.end = P.end;
        v.first = P.lead != 0 ? 1u : 0u;
        v.lo = a.start[p];
        v.hi = a.start[p + 1];
        v.lane_base = mulmod_canon(P.base_body, lane_mul);
    };
    auto rsrc_at = [&](uint32_t g, const View &v) {
        const uint64_t o = (uint64_t)(v.first + (g - v.lo)) * CHUNK;
        const uint64_t left = g < v.hi && o < v.end ? v.end - o : 0; // past the last part: zero-size descriptor, loads give 0, stores drop
        return __builtin_amdgcn_make_buffer_rsrc(v.origin + o, 0, (int)(left < CHUNK ? left : CHUNK), 0x00020000);
    };
    // states of this lane's U words in chunk g: the part's chunk c multiplies lane_base by a^(CHUNK*c), c < 2^24 (host)
    auto states = [&](uint32_t g, const View &v, uint32_t(&s)[U]) {
        const uint32_t c = v.first + (g - v.lo);
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        s[0] = mulmod_canon(v.lane_base, p);
#pragma unroll
        for (int u = 1; u < U; ++u) s[u] = mulmod_canon(s[u - 1], lcg::kTileLo.v[BLOCK / 256]);
    };
    View vl{nullptr, 0, 0, 0, 0, 1}, vs{nullptr, 0, 0, 0, 0, 1}; // load side, store side
    auto load = [&](u32x4(&d)[U], uint32_t g) {
        locate(g, vl);
        auto r = rsrc_at(g, vl);
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = __builtin_amdgcn_raw_buffer_load_b128(r, voff + u * SUB, 0, AUX_NT);
    };
    // Lane 0's ticket traffic.  The returning atomic is a plain compiler-visible atomic, so the compiler counts it
    // in its own s_waitcnt vmcnt(N) bookkeeping and waits for the value only where it is published, behind the
    // trip's arithmetic (with the next chunk's loads, issued after it, still in flight).  This needs the TU built with  -mllvm -amdgpu-atomic-optimizer-strategy=None : the default
    // "atomic optimizer" rewrites it into a wave-aggregated atomic followed at once by s_waitcnt vmcnt(0),
    // i.e. the wave would sit out the atomic's round trip and every load it has in flight, each trip.
    // The LDS word is accessed with ds_write / ds_read in assembly: a volatile C++ access to a __shared__
    // variable becomes a FLAT access, which waits on vmcnt as well as lgkmcnt.
    uint32_t pending = 0; // lane 0: the ticket in flight
    const uint32_t q_next_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&q_next[0];
    const uint32_t one = 1u;
    // one trip: chunk g's words are in d; compute, publish the ticket fetched at the start of this trip, barrier, store burst
    auto process_store = [&](u32x4(&d)[U], uint32_t g) {
        locate(g, vs);
        auto r = rsrc_at(g, vs);
        // resident or streaming: a property of the chunk's ABSOLUTE address (scalar, once per trip)
        const uint64_t addr = (uint64_t)reinterpret_cast<uintptr_t>(vs.origin) + (uint64_t)(vs.first + (g - vs.lo)) * CHUNK;
        const bool resident = ((uint32_t)(addr >> 16) & a.keep_mask) < a.keep_run;
        uint32_t s[U];
        states(g, vs, s);
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = cycle_word<ALG>(d[u], s[u]);
        if (tid == 0) // (the LDS write has landed before the barrier releases the readers)
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(q_next_lds + 4u * (trip & 1u)), "v"(pending) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        if (resident) { // (the cache policy is an immediate of the instruction: two bursts behind a scalar branch)
#pragma unroll
            for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB, 0, KAUX);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) __builtin_amdgcn_raw_buffer_store_b128(d[u], r, voff + u * SUB, 0, SAUX);
        }
        ++trip;
    };
    auto take_published = [&]() { // every lane, after the trip's barrier (trip already counted: the word is (trip-1)&1)
        uint32_t t;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(q_next_lds + 4u * ((trip - 1u) & 1u)) : "memory");
        return (uint32_t)PREFIX * Gm + (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    };

    // A workgroup's chunk sequence: positions 0 .. PREFIX-1 are static (b, b+Gm), position j + PREFIX is the
    // ticket fetched in trip j.  cq[] holds positions k .. k+DEPTH at the start of trip k: cq[0] is computed,
    // cq[DEPTH] is loaded now, the ones between are already in flight.
    uint32_t cq[NB];
    static_assert(PREFIX == NB, "the static positions are exactly the ones cq[] starts with");
    bool active = true;
    if (blk < Gm) {
#pragma unroll
        for (int i = 0; i < NB; ++i) cq[i] = blk + (uint32_t)i * Gm;
    } else {
        // A HELPER workgroup.  With the chip's clock where it normally is (2.1-2.2 GHz) the 25-per-32-CU main workgroups
        // saturate HBM and more streams only hurt (-1.8 % at one per CU).  For the first ~10 ms after load onset,
        // though, power management holds the shader clock at 1.2-1.7 GHz, and there the main workgroups run out of
        // ARITHMETIC (profiles/r03_first_pass.txt): the idle CUs' SIMDs are then worth more than the tidy memory
        // pattern (flat 6.85 TB/s with a workgroup on every CU against a dip to 6.2-6.4).  So the idle CUs get a
        // workgroup each that looks at the clock ONCE, when it starts -- shader-clock ticks (s_memtime) per 2 us of the
        // constant 100 MHz counter (s_memrealtime) -- and either joins, taking its first PREFIX chunks and all later
        // ones from the ticket counter, or leaves at once.  (Helpers that stay and keep watching the clock were tried:
        // correct, but with 56 workgroups standing by the main ones ran 15 % slower at full clock --
        // profiles/r03_tune_dvfs.txt keeps that row.)
        uint32_t t = 0xFFFFFFFFu;
        if (tid == 0) {
            const uint64_t t0 = wall_clock64(), c0 = clock64();
            uint64_t t1;
            do {
                __builtin_amdgcn_s_sleep(4);
                t1 = wall_clock64();
            } while (t1 - t0 < 200);
            const uint64_t mhz = ((clock64() - c0) * 100) / (t1 - t0);
            if (mhz < a.helper_below_mhz) t = __hip_atomic_fetch_add(a.queue, (uint32_t)PREFIX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            q_next[0] = t;
        }
        __syncthreads();
        t = q_next[0];
        __syncthreads(); // (the loop below writes q_next[0] again, in its first trip)
        active = t != 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < NB; ++i) cq[i] = (uint32_t)PREFIX * Gm + t + (uint32_t)i;
    }
    if (active && cq[0] < total) {
        u32x4 d[NB][U];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) load(d[i], cq[i]);
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                __builtin_amdgcn_s_barrier();
                // the ticket for the NEXT trip's load burst: fetched now, published behind this trip's arithmetic
                if (tid == 0) pending = __hip_atomic_fetch_add(a.queue, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                load(d[(p + DEPTH) % NB], cq[DEPTH]);
                __builtin_amdgcn_sched_barrier(0);
                process_store(d[p], cq[0]);
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
    // leave: this workgroup's ticket atomics have all returned; the last workgroup out resets the pair and then
    // tells the host (a word in host-coherent memory) that the pair may be handed to another launch
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(a.queue + 1, 1u) == G - 1) {
            __hip_atomic_store(a.queue, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.queue + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.queue_done) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // both zeroes have been performed device-wide
                __hip_atomic_store(a.queue_done, a.queue_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

namespace {
template <int U, int BLOCK> struct KeepShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const CycleKeepArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_keep_kernel<U, BLOCK>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() // as a profiler prints it
    {
        static char buf[96];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_keep_kernel<%d, %d>", U, BLOCK);
        (void)n;
        return buf;
    }
};
// the work-queue kernel's shape (cycle_kernel.hip: 1024 threads x 4 words = 64 KiB chunks)
using Keep = KeepShape<4, 1024>;
} // namespace

uint32_t modgpu_keep_chunk_bytes() { return Keep::chunk; }
uint32_t modgpu_keep_block() { return Keep::block; }
const char *modgpu_keep_kernel_name() { return Keep::name(); }
hipError_t modgpu_launch_cycle_keep(const CycleKeepArgs &a, uint32_t grid, hipStream_t stream)
{
    Keep::launch(a, grid, stream);
    return hipGetLastError();
}
