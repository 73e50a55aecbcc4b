// cycle_rekey_table_kernel.hip -- a TABLE of rekey entries that lives in device memory, any number of them, in three launches:
// dst_i[j] = src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j], the plaintext only in registers.  The two-keystream
// block: cycle_rekey_impl.h; the jump tables and the single-state arithmetic: cycle_kernel_impl.h; both included and not changed (their
// hashes are the rekey kernel's and the roofline kernel's; this TU has its own).
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
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_impl.h"
#include "cycle_rekey_table_kernel.h"

#include <cstdio>

namespace {

// a^(b * 256^k) for the four bytes of an exponent < 2^32: a^e by three multiplies
__constant__ lcg::Table<256> c_pow_b0 = lcg::make_pow_table<256>(1);
__constant__ lcg::Table<256> c_pow_b1 = lcg::make_pow_table<256>(256);
__constant__ lcg::Table<256> c_pow_b2 = lcg::make_pow_table<256>(65536);
__constant__ lcg::Table<256> c_pow_b3 = lcg::make_pow_table<256>(1u << 24);

__device__ __forceinline__ uint32_t pow_a(uint32_t e)
{
    uint32_t p = mulmod_canon(c_pow_b0.v[e & 255], c_pow_b1.v[(e >> 8) & 255]);
    p = mulmod_canon(p, c_pow_b2.v[(e >> 16) & 255]);
    return mulmod_canon(p, c_pow_b3.v[e >> 24]);
}

// x * y mod m for a state x (canonical, or 2^31-1 for the identity keystream) and a power y of a.  The fold gives x*y mod m or that
// + m; for x = 2^31-1 it gives 2^31-1 exactly.  Bit 31 set is the excess (r + m >= 2^31 for r >= 1), so 2^31-1 is kept.
__device__ __forceinline__ uint32_t mulmod_keep(uint32_t x, uint32_t y)
{
    const uint32_t X = mul_fold(x, 2u * y);
    return X >= 0x80000000u ? X - lcg::M : X;
}

// the state of stream byte o1 - 1 (o1 = off mod period + 1 + position, reduced) under key residue k; the identity keeps 2^31-1
__device__ __forceinline__ uint32_t state_at(uint32_t k, uint64_t e) { return k ? mulmod_canon(k, pow_a((uint32_t)(e % lcg::PERIOD))) : lcg::M; }

__device__ __forceinline__ uint32_t key_res(int32_t key)
{
    const int64_t kr = (int64_t)key % (int64_t)lcg::M;
    return (uint32_t)(kr < 0 ? kr + lcg::M : kr);
}

// reads of memory no launch of this TU writes while it runs: scalar loads when the address is uniform (address space 4; the host pass
// of the compiler only needs the types)
#if defined(__HIP_DEVICE_COMPILE__)
#define REKEY_TABLE_CONST_AS __attribute__((address_space(4)))
#else
#define REKEY_TABLE_CONST_AS
#endif
template <class T> __device__ __forceinline__ const REKEY_TABLE_CONST_AS T *as_const(const T *p) { return (const REKEY_TABLE_CONST_AS T *)p; }
struct Keys16 {
    uint32_t v[16];
};

constexpr uint32_t kChunk = 65536; // the stream kernel's chunk: 4 words x 1024 threads x 16 bytes

} // namespace

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_table_plan(RekeyTableArgs a)
{
    __shared__ uint64_t sc[kTableBlock];
    __shared__ uint32_t sbad;
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kTableBlock + tid;
    if (blockIdx.x == 0 && tid == 0) {
        a.hdr->ticket = 0;
        a.hdr->first_bad = kTableNoBad;
        a.hdr->total = 0;
    }
    if (tid == 0) sbad = 0;
    uint64_t cnt = 0;
    uint32_t bad = 0;
    if (i < a.n) {
        const RekeyTableEntry E = a.entries[i];
        const uintptr_t d = reinterpret_cast<uintptr_t>(E.dst);
        const uint64_t head = E.n < ((16 - (d & 15)) & 15) ? E.n : ((16 - (d & 15)) & 15);
        const uint64_t words = (E.n - head) / 16;
        const uint64_t tail = E.n - head - words * 16;
        const uint32_t lead = (uint32_t)((d + head) & (kChunk - 1));
        const uint64_t end = lead + words * 16;
        cnt = words ? (end + kChunk - 1) / kChunk : 0;
        bad = (E.n && (!E.dst || !E.src)) || E.flags != 0 || E.reserved != 0 || cnt > kTableMaxEntryChunks ? 1u : 0u;
        if (bad) cnt = 0;
        // states: key * a^(o + 1 + position), positions mod the period; the body's counted from the chunk origin
        const uint32_t kf = key_res(E.key_from), kt = key_res(E.key_to);
        const uint64_t of = E.off_from % lcg::PERIOD + 1, ot = E.off_to % lcg::PERIOD + 1;
        const uint64_t body = head + lcg::PERIOD - lead, after = head + (words * 16) % lcg::PERIOD;
        RekeyTablePlan P;
        P.dst_origin = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(E.dst) + head - lead); // (as integers: a refused entry's pointer may be NULL)
        P.src_origin = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(E.src) + head - lead);
        P.end = end;
        P.start = 0;
        P.lead = lead;
        P.chunks = (uint32_t)cnt;
        P.base_from = state_at(kf, of + body);
        P.base_to = state_at(kt, ot + body);
        P.bad = bad;
        P.head_n = (uint32_t)head;
        P.tail_n = (uint32_t)tail;
        P.pad = 0;
        a.plan[i] = P;
        RekeyTableEdge X;
        X.head[0] = state_at(kf, of);
        X.head[1] = state_at(kt, ot);
        X.tail[0] = state_at(kf, of + after);
        X.tail[1] = state_at(kt, ot + after);
        a.edge[i] = X;
    }
    sc[tid] = cnt;
    __syncthreads();
    if (bad) atomicOr(&sbad, 1u);
    // inclusive scan of the 1024 counts (Hillis-Steele; every thread reaches every barrier)
    for (uint32_t s = 1; s < kTableBlock; s <<= 1) {
        const uint64_t v = tid >= s ? sc[tid - s] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    if (i < a.n) a.plan[i].start = sc[tid] - cnt;
    if (tid == kTableBlock - 1) {
        a.blk[blockIdx.x].chunks = sc[tid];
        a.blk[blockIdx.x].bad = sbad;
    }
}

// ---- finish: global starts, the status, the search levels, the ragged edges --------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_table_finish(RekeyTableArgs a)
{
    __shared__ uint64_t r_before[kTableBlock], r_total[kTableBlock];
    __shared__ uint32_t sbad;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t i = (uint64_t)b * kTableBlock + tid;
    if (tid == 0) sbad = 0;
    uint64_t before = 0, total = 0;
    uint32_t bad = 0;
    for (uint32_t k = tid; k < a.n_blk; k += kTableBlock) {
        const uint64_t c = a.blk[k].chunks;
        total += c;
        before += k < b ? c : 0;
        bad |= a.blk[k].bad;
    }
    r_before[tid] = before;
    r_total[tid] = total;
    __syncthreads();
    if (bad) atomicOr(&sbad, 1u);
    for (uint32_t s = kTableBlock / 2; s > 0; s >>= 1) {
        if (tid < s) {
            r_before[tid] += r_before[tid + s];
            r_total[tid] += r_total[tid + s];
        }
        __syncthreads();
    }
    before = r_before[0];
    total = r_total[0];
    const bool ok = sbad == 0 && total <= kTableMaxChunks;
    if (b == 0 && tid == 0) a.hdr->total = ok ? total : 0;
    if (i < a.n) {
        const RekeyTablePlan P = a.plan[i];
        const uint64_t start = before + P.start;
        if (!ok) {
            // refused: write nothing; the lowest bad entry -- a refused one, or the first whose chunks pass the ticket range
            if (P.bad || start + P.chunks > kTableMaxChunks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        } else {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k)
                if (k <= a.top && (i & ((1ull << (4 * k)) - 1)) == 0) a.level[k][i >> (4 * k)] = (uint32_t)start;
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
#pragma unroll
            for (uint32_t j = 0; j < 15; ++j) {
                const uint32_t y = c_pow_b0.v[j];
                if (j < P.head_n) db[(int64_t)j - P.head_n] = rekey_byte(hb[j], mulmod_keep(X.head[0], y), mulmod_keep(X.head[1], y));
                if (j < P.tail_n) db[body + j] = rekey_byte(tb[j], mulmod_keep(X.tail[0], y), mulmod_keep(X.tail[1], y));
            }
        }
    }
    // each level padded with ~0 to a whole line of 16 keys: the descent reads 16 at a time
    if (ok && b == 0 && tid < 16)
        for (uint32_t k = 0; k < kTableLevels; ++k)
            if (k <= a.top && a.level_n[k] + tid < ((a.level_n[k] + 15) & ~15ull)) a.level[k][a.level_n[k] + tid] = ~0u;
}

// ---- stream ------------------------------------------------------------------------------------------------------------------------
namespace {
struct Raw {
    u32x4 d;
    uint32_t e; // the dword after d, read when the chunk's source is not dword-aligned
};
__device__ __forceinline__ u32x4 funnel(const Raw &w, uint32_t sh) // sh == 0: alignbyte by 0 is the low dword itself
{
    u32x4 d;
    d.x = __builtin_amdgcn_alignbyte(w.d.y, w.d.x, sh);
    d.y = __builtin_amdgcn_alignbyte(w.d.z, w.d.y, sh);
    d.z = __builtin_amdgcn_alignbyte(w.d.w, w.d.z, sh);
    d.w = __builtin_amdgcn_alignbyte(w.e, w.d.w, sh);
    return d;
}
} // namespace

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
        for (int k = (int)a.top; k >= 0; --k) {
            const Keys16 keys = *as_const(reinterpret_cast<const Keys16 *>(a.level[k] + 16u * j));
            uint32_t c = 0;
#pragma unroll
            for (int t = 0; t < 16; ++t) c += keys.v[t] <= g ? 1u : 0u;
            j = 16u * j + c - 1u;
        }
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
    struct Span {
        uint64_t off;
        uint32_t cut, bytes;
    };
    auto span = [&](uint32_t g, const View &v) {
        Span s{0, 0, 0};
        if (g >= total) return s; // past the last entry: zero-size descriptors, loads give 0, stores drop
        const uint32_t c = g - v.lo;
        s.off = (uint64_t)c * CHUNK;
        s.cut = c ? 0u : v.lead;
        const uint64_t lim = v.end < s.off + CHUNK ? v.end : s.off + CHUNK;
        s.bytes = (uint32_t)(lim - s.off - s.cut);
        return s;
    };
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
    static const char *name() // as a profiler prints it
    {
        static char buf[96];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_rekey_table_kernel<%d, %d>", U, BLOCK);
        (void)n;
        return buf;
    }
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
