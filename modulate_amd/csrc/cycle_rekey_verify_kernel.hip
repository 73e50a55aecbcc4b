// cycle_rekey_verify_kernel.hip -- the rekey verify kernel: mismatches = #{ j : expect[j] != (src[j] ^ ks(key_from)[off_from + j] ^
// ks(key_to)[off_to + j]) } and the lowest such j -- the bytes the rekey kernel would have written, compared and not written -- in ONE
// pass that reads both buffers once and writes nothing but the entry's 32-byte result.  The two-keystream block: cycle_rekey_impl.h;
// the jump tables and the single-state arithmetic: cycle_kernel_impl.h; both included and not changed (this TU has a hash of its own).
//
// Shape: the verify kernel's stream (cycle_verify_kernel.hip has the reasoning) -- persistent 1024-thread workgroups, 64 KiB chunks on
// absolute chunk-aligned EXPECT addresses, the source at any byte phase (plain or funnel form), nt loads in a ping-pong pipeline behind
// one workgroup barrier, chunks assigned STATICALLY (workgroup b: chunks b, b + G, ...: nothing that can run out), each entry's ragged
// edges (< 16 bytes), its cut first chunk and the store of its n done by workgroup p before the stream, per-lane counts and positions
// in registers for as long as the workgroup is inside one entry, folded through 16 bytes of LDS into at most ONE 64-bit atomic add and
// ONE 64-bit atomic min per workgroup and entry.  The results are initialised by the verify TU's init launch in front
// (modgpu_launch_verify_init), so every run and every graph replay starts clean.
// What differs: every lane-word carries TWO states, one per keystream, as in the rekey kernel (cycle_rekey_kernel.hip): a chunk's jump
// and a lane's are shared, each state costs one more multiply, and offsets that differ in any way only change the two base states the
// host computes.  The two-keystream block owns v[112:127], so the pipeline's two sets of two-sided loads live in 112 VGPRs; ONE pair of
// states is kept live and stepped from word to word (DESIGN.md 4.12 has the register story).  There is no identity form: entries
// whose keystreams cancel or of which one is the identity run on the verify kernels.
// The small helpers (source reader, Found, note_word) are this TU's own copies of the verify kernel's.
// Vector atomics and vector stores only.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_impl.h"
#include "cycle_rekey_verify_kernel.h"

#include <cstdio>

namespace {

// The source side of one chunk (cycle_to_kernel.hip): a descriptor and, for the funnel form, the byte shift inside a dword.
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

// what a lane has found in the entry its workgroup is in: mismatching bytes and the lowest of their indices
struct Found {
    uint32_t cnt;
    unsigned long long first;
};

// number of nonzero bytes of a dword
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return (uint32_t)__builtin_popcount(w & 0x01010101u);
}
// the slow path: x != 0 is one word's difference, j0 the index of its first byte in the entry
__device__ __forceinline__ void note_word(Found &f, u32x4 x, unsigned long long j0)
{
    f.cnt += nonzero_bytes(x.x) + nonzero_bytes(x.y) + nonzero_bytes(x.z) + nonzero_bytes(x.w);
    uint32_t low = 12u + ((uint32_t)__builtin_ctz(x.w | 0x80000000u) >> 3);
    if (x.z) low = 8u + ((uint32_t)__builtin_ctz(x.z) >> 3);
    if (x.y) low = 4u + ((uint32_t)__builtin_ctz(x.y) >> 3);
    if (x.x) low = (uint32_t)__builtin_ctz(x.x) >> 3;
    const unsigned long long j = j0 + low;
    f.first = j < f.first ? j : f.first;
}
__device__ __forceinline__ uint32_t any_bits(u32x4 x) { return x.x | x.y | x.z | x.w; }

// < 16 bytes before / after an entry's aligned expect body, bytewise, by 32 lanes of one workgroup
__device__ __forceinline__ void verify_edges(const CycleRekeyVerifyPart &P, uint64_t body_bytes, uint32_t tid, Found &f)
{
    if (tid < P.head_n) {
        uint32_t sa = P.base_head[0], sb = P.base_head[1];
        for (uint32_t j = 0; j < tid; ++j) {
            sa = mulmod_canon(sa, lcg::A);
            sb = mulmod_canon(sb, lcg::A);
        }
        if ((P.expect_body - P.head_n)[tid] != rekey_byte((P.src_body - P.head_n)[tid], sa, sb)) {
            f.cnt += 1;
            f.first = tid < f.first ? tid : f.first;
        }
    } else if (tid >= 16 && tid < 32 && tid - 16 < P.tail_n) {
        const uint32_t t = tid - 16;
        uint32_t sa = P.base_tail[0], sb = P.base_tail[1];
        for (uint32_t j = 0; j < t; ++j) {
            sa = mulmod_canon(sa, lcg::A);
            sb = mulmod_canon(sb, lcg::A);
        }
        if (P.expect_body[body_bytes + t] != rekey_byte(P.src_body[body_bytes + t], sa, sb)) {
            const unsigned long long j = P.head_n + body_bytes + t;
            f.cnt += 1;
            f.first = j < f.first ? j : f.first;
        }
    }
}

} // namespace

template <int U, int BLOCK, bool FUNNEL>
__global__ __launch_bounds__(BLOCK) MODGPU_REKEY_KEEP_OFF_THE_FIXED_TEMPORARIES void modgpu_cycle_rekey_verify_kernel(CycleRekeyVerifyArgs a)
{
    static_assert(BLOCK % 256 == 0 && BLOCK <= 1024, "BLOCK is a whole number of 4096-byte tiles");
    constexpr uint32_t CHUNK = (uint32_t)U * BLOCK * lcg::WORD;
    constexpr uint32_t SUB = BLOCK * lcg::WORD;
    const uint32_t tid = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    const uint32_t G = gridDim.x;
    const uint32_t n_parts = a.n_parts;
    const uint32_t total = a.start[kCycleBatchMax];
    __shared__ unsigned long long red[2]; // the workgroup's {count, lowest index} of the entry it is leaving
    const uint32_t voff = tid * lcg::WORD;
    const uint32_t lane_mul = mulmod_canon(c_tile_lo.v[tid >> 8], c_lane_pow.v[tid & 255]);
    Found f{0u, kVerifyNone};

    if (tid == 0) {
        red[0] = 0ull;
        red[1] = kVerifyNone;
    }
    __syncthreads();

    // The workgroup leaves an entry (uniform: every wave comes here at the same chunk): lanes that found something fold it into LDS,
    // thread 0 sends the sums on -- one add and one min, and only if there is something to send.
    auto flush = [&](CycleVerifyResult *res) {
        if (f.cnt != 0) {
            atomicAdd(&red[0], (unsigned long long)f.cnt);
            atomicMin(&red[1], f.first);
        }
        f.cnt = 0u;
        f.first = kVerifyNone;
        __syncthreads();
        if (tid == 0) {
            const unsigned long long c = red[0];
            if (c != 0) {
                __hip_atomic_fetch_add(&res->mismatches, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_min(&res->first_mismatch, red[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                red[0] = 0ull;
                red[1] = kVerifyNone;
            }
        }
        __syncthreads();
    };

    // edges and cut first chunk of entry p, and the entry's n: workgroup p, before the stream starts (cold code)
    for (uint32_t p = blk; p < n_parts; p += G) {
        const CycleRekeyVerifyPart &P = a.part[p];
        const uint64_t body_bytes = P.end - P.lead;
        if (tid == 0) P.result->n = P.n;
        if (tid < 32) verify_edges(P, body_bytes, tid, f);
        if (P.lead != 0 && body_bytes != 0) {
            const uint32_t inside = (uint32_t)(P.end < CHUNK ? body_bytes : CHUNK - P.lead);
            auto re = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(P.expect_body), 0, (int)inside, 0x00020000);
            const SrcRsrc rs = src_rsrc<FUNNEL>(P.src_body, inside);
            uint32_t sa = mulmod_canon(P.base_body[0], lane_mul), sb = mulmod_canon(P.base_body[1], lane_mul);
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)U; ++u) {
                const uint32_t o = voff + u * SUB - P.lead; // lanes in front of the body wrap past num_records: dropped, and masked below
                Raw w;
                load_src<FUNNEL>(w, rs, o);
                const u32x4 e = __builtin_amdgcn_raw_buffer_load_b128(re, o, 0, AUX_NT);
                const u32x4 x = rekey_word(src_word<FUNNEL>(w, rs.sh), sa, sb) ^ e;
                sa = mulmod_canon(sa, lcg::kTileLo.v[BLOCK / 256]);
                sb = mulmod_canon(sb, lcg::kTileLo.v[BLOCK / 256]);
                if (o < inside && any_bits(x) != 0) note_word(f, x, (unsigned long long)P.head_n + o);
            }
        }
        flush(P.result);
    }

    struct View {
        const uint8_t *origin;     // expect_body - lead
        const uint8_t *src_origin; // src_body - lead
        CycleVerifyResult *res;
        uint32_t full, rem; // whole chunks from the chunk origin to the body's end, and the bytes of the ragged one behind them
        uint64_t idx0;      // index in the entry of the byte at the chunk origin (head_n - lead, modulo 2^64)
        uint32_t lo, hi;
        uint32_t first;
        uint32_t lane_base[2];
    };
    auto locate = [&](uint32_t g, View &v) {
        uint32_t p = 0;
#pragma unroll 1
        for (uint32_t i = 1; i < n_parts; ++i) p += g >= a.start[i] ? 1u : 0u;
        const CycleRekeyVerifyPart &P = a.part[p];
        v.origin = P.expect_body - P.lead;
        v.src_origin = P.src_body - P.lead;
        v.res = P.result;
        v.full = (uint32_t)(P.end / CHUNK);
        v.rem = (uint32_t)(P.end % CHUNK);
        v.idx0 = (uint64_t)P.head_n - P.lead;
        v.first = P.lead != 0 ? 1u : 0u;
        v.lo = a.start[p];
        v.hi = a.start[p + 1];
        v.lane_base[0] = mulmod_canon(P.base_body[0], lane_mul);
        v.lane_base[1] = mulmod_canon(P.base_body[1], lane_mul);
    };
    auto chunk_off = [&](uint32_t g, const View &v) { return (uint64_t)(v.first + (g - v.lo)) * CHUNK; };
    // (32-bit scalar compares only: a 64-bit one is done by the VALU, in a register the loads in flight may own)
    auto chunk_left = [&](uint32_t g, const View &v) {
        const uint32_t c = v.first + (g - v.lo);
        const uint32_t left = c < v.full ? CHUNK : c == v.full ? v.rem : 0u;
        return g < v.hi ? left : 0u; // past the last entry: zero-size descriptors
    };
    // both keystreams' states of the lane's first word of chunk g: one chunk jump, shared
    auto states = [&](uint32_t g, const View &v, uint32_t &sa, uint32_t &sb) {
        const uint32_t c = v.first + (g - v.lo);
        uint32_t p = mulmod_canon(c_chunk_pow0<CHUNK>.v[c & 255], c_chunk_pow1<CHUNK>.v[(c >> 8) & 255]);
        p = mulmod_canon(p, c_chunk_pow2<CHUNK>.v[(c >> 16) & 255]);
        sa = mulmod_canon(v.lane_base[0], p);
        sb = mulmod_canon(v.lane_base[1], p);
    };
    View vl{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, {1, 1}}, vp{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, {1, 1}}; // load side, compare side
    // The load side of a trip: chunk g's SOURCE words go out at once, a whole trip ahead, into the set the compare side is not reading;
    // what comes back is the descriptor of the chunk's comparand, whose words follow one by one as the compare side frees their registers
    // (two sets of both sides do not fit under v112 next to the two-keystream block: DESIGN.md 4.12).
    auto load = [&](Raw(&w)[U], uint32_t g) {
        if (g - vl.lo >= vl.hi - vl.lo) locate(g, vl);
        const uint64_t o = chunk_off(g, vl);
        const uint32_t left = chunk_left(g, vl);
        const SrcRsrc rs = src_rsrc<FUNNEL>(vl.src_origin + o, left);
#pragma unroll
        for (int u = 0; u < U; ++u) load_src<FUNNEL>(w[u], rs, voff + u * SUB);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(vl.origin + o), 0, (int)left, 0x00020000);
    };
    // Compares chunk g; `next` is the comparand of the chunk after it: word u of it is asked for as soon as word u of this one has been
    // used, so it has the rest of this trip and the start of the next to arrive -- the distance the source's loads have.
    auto compare = [&](Raw(&w)[U], u32x4(&e)[U], uint32_t g, __amdgpu_buffer_rsrc_t next) {
        if (g - vp.lo >= vp.hi - vp.lo) {
            if (vp.res) flush(vp.res); // the workgroup moves on to another entry
            locate(g, vp);
        }
        const uint64_t o = chunk_off(g, vp);
        const uint32_t left = chunk_left(g, vp);
        const uint32_t sh = FUNNEL ? (uint32_t)(uintptr_t)(vp.src_origin + o) & 3u : 0u;
        uint32_t sa, sb;
        states(g, vp, sa, sb);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 x = rekey_word(src_word<FUNNEL>(w[u], sh), sa, sb) ^ e[u];
            e[u] = __builtin_amdgcn_raw_buffer_load_b128(next, voff + u * SUB, 0, AUX_NT);
            if (u + 1 < U) { // (one pair of states live, not U: the loads need the registers)
                sa = mulmod_canon(sa, lcg::kTileLo.v[BLOCK / 256]);
                sb = mulmod_canon(sb, lcg::kTileLo.v[BLOCK / 256]);
            }
            // a lane past the ragged end of the entry's last chunk read nothing on either side: its x is the keystreams, not a finding
            const uint32_t in = voff + (uint32_t)u * SUB < left ? ~0u : 0u;
            x &= in;
            // clean data costs three ORs and this test per word; the rest is for the waves that have something to report
            if (__builtin_amdgcn_ballot_w64(any_bits(x) != 0u) != 0ull) {
                if (any_bits(x) != 0u) note_word(f, x, vp.idx0 + o + voff + (uint32_t)u * SUB);
            }
        }
    };

    uint32_t g = blk;
    if (g < total) {
        Raw w[2][U];
        u32x4 e[U];
        {
            const auto re = load(w[0], g);
#pragma unroll
            for (int u = 0; u < U; ++u) e[u] = __builtin_amdgcn_raw_buffer_load_b128(re, voff + u * SUB, 0, AUX_NT);
        }
        bool finished = false;
        while (!finished) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                __builtin_amdgcn_s_barrier();
                const auto next = load(w[p ^ 1], g + G); // (past the last chunk: zero-size descriptors, nothing is read)
                __builtin_amdgcn_sched_barrier(0);
                compare(w[p], e, g, next);
                g += G;
                if (g >= total) {
                    finished = true;
                    break;
                }
            }
        }
        flush(vp.res);
    }
}

namespace {
template <int U, int BLOCK, bool FUNNEL> struct RekeyVerifyShape {
    static constexpr uint32_t chunk = (uint32_t)U * BLOCK * lcg::WORD;
    static constexpr uint32_t block = BLOCK;
    static void launch(const CycleRekeyVerifyArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_rekey_verify_kernel<U, BLOCK, FUNNEL>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    static const char *name() // as a profiler prints it
    {
        static char buf[112];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_rekey_verify_kernel<%d, %d, %s>", U, BLOCK, FUNNEL ? "true" : "false");
        (void)n;
        return buf;
    }
};
// the verify kernel's shape (1024 threads x 4 words = 64 KiB chunks)
using RekeyVerifyPlain = RekeyVerifyShape<4, 1024, false>;
using RekeyVerifyFunnel = RekeyVerifyShape<4, 1024, true>;
static_assert(RekeyVerifyPlain::chunk == RekeyVerifyFunnel::chunk, "one chunk size for both forms");
} // namespace

uint32_t modgpu_rekey_verify_chunk_bytes() { return RekeyVerifyPlain::chunk; }
uint32_t modgpu_rekey_verify_block() { return RekeyVerifyPlain::block; }
const char *modgpu_rekey_verify_kernel_name(int form) { return form == CYCLE_REKEY_VERIFY_FUNNEL ? RekeyVerifyFunnel::name() : RekeyVerifyPlain::name(); }
hipError_t modgpu_launch_cycle_rekey_verify(const CycleRekeyVerifyArgs &a, int form, uint32_t grid, hipStream_t stream)
{
    if (form == CYCLE_REKEY_VERIFY_FUNNEL) RekeyVerifyFunnel::launch(a, grid, stream);
    else RekeyVerifyPlain::launch(a, grid, stream);
    return hipGetLastError();
}
