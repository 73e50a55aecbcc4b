// cycle_rekey_verify_table_kernel.hip -- a TABLE of rekey entries that lives in device memory, any number of them, VERIFIED in three
// launches: result_i = { #{ j : dst_i[j] != (src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j]) }, the lowest such
// j, n_i, 0 }, dst being the comparand.  Both sides are read once; nothing is written but the results and the workspace.  The
// two-keystream block: cycle_rekey_impl.h; the jump tables and the single-state arithmetic: cycle_kernel_impl.h; both included and not
// changed (this TU has a hash of its own).
//
// Three parents, joined (their code is copied here, not shared: every TU keeps a source list and a hash of its own):
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
#include "cycle_rekey_verify_table_kernel.h"

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
#define REKEY_VERIFY_TABLE_CONST_AS __attribute__((address_space(4)))
#else
#define REKEY_VERIFY_TABLE_CONST_AS
#endif
template <class T> __device__ __forceinline__ const REKEY_VERIFY_TABLE_CONST_AS T *as_const(const T *p) { return (const REKEY_VERIFY_TABLE_CONST_AS T *)p; }
struct Keys16 {
    uint32_t v[16];
};

constexpr uint32_t kChunk = 65536; // the stream kernel's chunk: 4 words x 1024 threads x 16 bytes

} // namespace

// ---- plan: one thread per entry ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_verify_table_plan(RekeyVerifyTableArgs a)
{
    __shared__ uint64_t sc[kTableBlock];
    __shared__ uint32_t sbad;
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
    if (tid == 0) sbad = 0;
    uint64_t cnt = 0;
    uint32_t bad = 0;
    if (i < a.n) {
        const RekeyTableEntry E = a.entries[i];
        const uintptr_t d = reinterpret_cast<uintptr_t>(E.dst); // the comparand: the chunk grid is laid on it
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

// ---- finish: global starts, the status, the search levels, the ragged edges compared, every result initialised ---------------------
__global__ __launch_bounds__(kTableBlock) void modgpu_cycle_rekey_verify_table_finish(RekeyVerifyTableArgs a)
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
            // refused: no result is written; the lowest bad entry -- a refused one, or the first whose chunks pass the ticket range
            if (P.bad || start + P.chunks > kTableMaxChunks) atomicMin((unsigned long long *)&a.hdr->first_bad, (unsigned long long)i);
        } else {
            a.plan[i].start = start;
            for (uint32_t k = 0; k < kTableLevels; ++k)
                if (k <= a.top && (i & ((1ull << (4 * k)) - 1)) == 0) a.level[k][i >> (4 * k)] = (uint32_t)start;
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
__device__ __forceinline__ u32x4 funnel(const Raw &w, uint32_t sh) // sh == 0: alignbyte by 0 is the low dword itself (w.e, not loaded then, has no part in d.w)
{
    u32x4 d;
    d.x = __builtin_amdgcn_alignbyte(w.d.y, w.d.x, sh);
    d.y = __builtin_amdgcn_alignbyte(w.d.z, w.d.y, sh);
    d.z = __builtin_amdgcn_alignbyte(w.d.w, w.d.z, sh);
    d.w = __builtin_amdgcn_alignbyte(w.e, w.d.w, sh);
    return d;
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
// the slow path: x != 0 is one word's difference, at `pos` bytes from the chunk's origin; `low` = the lowest such position so far
__device__ __forceinline__ void note_word(uint32_t &cnt, uint32_t &low, u32x4 x, uint32_t pos)
{
    cnt += nonzero_bytes(x.x) + nonzero_bytes(x.y) + nonzero_bytes(x.z) + nonzero_bytes(x.w);
    uint32_t b = 12u + ((uint32_t)__builtin_ctz(x.w | 0x80000000u) >> 3);
    if (x.z) b = 8u + ((uint32_t)__builtin_ctz(x.z) >> 3);
    if (x.y) b = 4u + ((uint32_t)__builtin_ctz(x.y) >> 3);
    if (x.x) b = (uint32_t)__builtin_ctz(x.x) >> 3;
    low = pos + b < low ? pos + b : low;
}
__device__ __forceinline__ uint32_t any_bits(u32x4 x) { return x.x | x.y | x.z | x.w; }

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
        do { // (level 0 always exists)
            const Keys16 keys = *as_const(reinterpret_cast<const Keys16 *>(a.level[k] + 16u * j));
            uint32_t c = 0;
#pragma unroll
            for (int t = 0; t < 16; ++t) c += keys.v[t] <= g ? 1u : 0u;
            j = 16u * j + c - 1u;
        } while (--k >= 0);
        const RekeyTablePlan P = *as_const(a.plan + j);
        v.exp0 = P.dst_origin;
        v.src0 = P.src_origin;
        v.lead_rem = P.lead | ((uint32_t)(P.end - (uint64_t)(P.chunks - 1u) * CHUNK) - 1u) << 16;
        v.lo = (uint32_t)P.start;
        v.hi = (uint32_t)P.start + P.chunks;
        v.entry = j | (P.head_n << 24);
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
        if (g >= total) return s; // past the last entry: zero-size descriptors, loads give 0
        const uint32_t c = g - v.lo;
        s.off = (uint64_t)c * CHUNK;
        s.cut = c ? 0u : v.lead_rem & 0xFFFFu;
        s.bytes = (c + 1u == v.hi - v.lo ? (v.lead_rem >> 16) + 1u : CHUNK) - s.cut;
        return s;
    };
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
    static const char *name() // as a profiler prints it
    {
        static char buf[96];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_rekey_verify_table_kernel<%d, %d>", U, BLOCK);
        (void)n;
        return buf;
    }
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
