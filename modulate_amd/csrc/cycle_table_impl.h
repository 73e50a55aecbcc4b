// cycle_table_impl.h -- device code the five TABLE TUs share (cycle_table_kernel.hip, cycle_rekey_table_kernel.hip,
// cycle_verify_table_kernel.hip, cycle_rekey_verify_table_kernel.hip, cycle_rekey_move_table_kernel.hip): the state of any stream
// position by four byte tables, an entry laid on the chunk grid and the refusal rule, the plan launch's scan, the finish launch's totals
// and search levels, one level of the 16-ary descent, a chunk's span, the funnel; what the two-keystream tables add (the identity kept
// as 2^31-1, the six states of an entry); what the verifying tables add (a lane's findings); what the two digesting loops add (a word's sums, the reduction mod 65521, the wave
// fold).  Each of those TUs includes it and names
// it in its source list, so each keeps a hash of its own.  A TU keeps its __global__ kernels, its View, its load / store / compare /
// move code, its edge treatment and its launch wrappers; the two verifying stream kernels also keep their per-wave flush, and the
// descent's loop stays with its caller (two of them enter it without the test for level 0): as functions here they changed those
// kernels' register allocation, and the stream kernels' assembly is held to what it was.
//
// Everything is in an unnamed namespace: each TU gets its own __constant__ tables, as before.  The two-keystream pieces are templates
// over the record types of cycle_rekey_table_kernel.h, so this header does not need it.  The helpers take the fields they use, never a
// kernel's whole argument: a reference to it makes the compiler load every argument up front.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#include "cycle_kernel_impl.h"
#include "cycle_table_kernel.h"

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

// reads of memory no launch of the TU writes while it runs: scalar loads when the address is uniform (address space 4; the host pass
// of the compiler only needs the types)
#if defined(__HIP_DEVICE_COMPILE__)
#define TABLE_CONST_AS __attribute__((address_space(4)))
#else
#define TABLE_CONST_AS
#endif
template <class T> __device__ __forceinline__ const TABLE_CONST_AS T *as_const(const T *p) { return (const TABLE_CONST_AS T *)p; }
struct Keys16 {
    uint32_t v[16];
};

constexpr uint32_t kChunk = 65536; // the stream kernels' chunk: 4 words x 1024 threads x 16 bytes

// ---- plan ----------------------------------------------------------------------------------------------------------------------------
// An entry on the chunk grid of its destination (the comparand, for a verifying table): < 16 bytes in front of the 16-byte aligned body,
// the body's words, < 16 bytes behind it; lead = the body's first byte modulo the chunk, end = lead + body bytes, cnt = its chunks.
struct TableGrid {
    uint64_t head, words, tail, end, cnt;
    uint32_t lead, bad;
};
// `flags` = every field of the entry that must be 0.  Refused: a NULL pointer with bytes to move, a nonzero flag, a body beyond the chunk
// jump tables; a refused entry has no chunks.
template <class Entry> __device__ __forceinline__ TableGrid table_grid(const Entry &E, uint32_t flags)
{
    TableGrid g;
    const uintptr_t d = reinterpret_cast<uintptr_t>(E.dst);
    g.head = E.n < ((16 - (d & 15)) & 15) ? E.n : ((16 - (d & 15)) & 15);
    g.words = (E.n - g.head) / 16;
    g.tail = E.n - g.head - g.words * 16;
    g.lead = (uint32_t)((d + g.head) & (kChunk - 1));
    g.end = g.lead + g.words * 16;
    g.cnt = g.words ? (g.end + kChunk - 1) / kChunk : 0;
    g.bad = (E.n && (!E.dst || !E.src)) || flags != 0 || g.cnt > kTableMaxEntryChunks ? 1u : 0u;
    if (g.bad) g.cnt = 0;
    return g;
}
// the fields every kind of plan record has
template <class Plan, class Entry> __device__ __forceinline__ void table_lay(Plan &P, const Entry &E, const TableGrid &g)
{
    P.dst_origin = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(E.dst) + g.head - g.lead); // (as integers: a refused entry's pointer may be NULL)
    P.src_origin = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(E.src) + g.head - g.lead);
    P.end = g.end;
    P.start = 0;
    P.lead = g.lead;
    P.chunks = (uint32_t)g.cnt;
    P.bad = g.bad;
    P.head_n = (uint32_t)g.head;
    P.tail_n = (uint32_t)g.tail;
}

__device__ __forceinline__ uint32_t key_res(int32_t key)
{
    const int64_t kr = (int64_t)key % (int64_t)lcg::M;
    return (uint32_t)(kr < 0 ? kr + lcg::M : kr);
}

// a single-keystream entry: its three base states, key * a^(o + 1 + position), positions mod the period; 0 = the identity keystream
__device__ __forceinline__ void table_plan_entry(CycleTablePlan &P, const CycleTableEntry &E, const TableGrid &g)
{
    const uint32_t k = key_res(E.key);
    const uint64_t o1 = E.stream_off % lcg::PERIOD + 1;
    P.base_head = mulmod_canon(k, pow_a((uint32_t)(o1 % lcg::PERIOD)));
    P.base = mulmod_canon(k, pow_a((uint32_t)((o1 + g.head + lcg::PERIOD - g.lead) % lcg::PERIOD)));
    P.base_tail = mulmod_canon(k, pow_a((uint32_t)((o1 + g.head + (g.words * 16) % lcg::PERIOD) % lcg::PERIOD)));
    table_lay(P, E, g);
}

// The workgroup's 1024 chunk counts scanned in LDS (Hillis-Steele; every thread reaches every barrier): this thread's inclusive sum,
// and whether any thread of the workgroup has a bad entry.  Owns 8200 bytes of LDS: call once per kernel.
struct PlanScan {
    uint64_t upto;
    uint32_t bad;
};
__device__ __forceinline__ PlanScan table_plan_scan(uint64_t cnt, uint32_t bad, uint32_t tid)
{
    __shared__ uint64_t sc[kTableBlock];
    __shared__ uint32_t sbad;
    if (tid == 0) sbad = 0;
    sc[tid] = cnt;
    __syncthreads();
    if (bad) atomicOr(&sbad, 1u);
    for (uint32_t s = 1; s < kTableBlock; s <<= 1) {
        const uint64_t v = tid >= s ? sc[tid - s] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    return PlanScan{sc[tid], sbad};
}
// ... and what the plan launch leaves of it: the entry's start among the 1024 of its record, the record's count and refusal
template <class Plan, class Blk> __device__ __forceinline__ void table_plan_store(Plan *plan, Blk *blk, uint64_t n, uint64_t i, uint64_t cnt, uint32_t bad, uint32_t tid)
{
    const PlanScan S = table_plan_scan(cnt, bad, tid);
    if (i < n) plan[i].start = S.upto - cnt;
    if (tid == kTableBlock - 1) {
        blk[blockIdx.x].chunks = S.upto;
        blk[blockIdx.x].bad = S.bad;
    }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------------
// Every workgroup adds up the chunk counts of the records before its own (b) and of all of them, and ORs their refusals: the entries'
// starts are global without a third scan pass.  each(k, B) sees every record this thread reads, in rising order; merge() runs in every
// thread behind the first barrier, where a TU folds what its each() gathered into LDS of its own (initialised before the call; readable
// after it).  Owns 16392 bytes of LDS: call once per kernel.
struct TableTotals {
    uint64_t before, total;
    uint32_t bad;
};
template <class Blk, class Each, class Merge>
__device__ __forceinline__ TableTotals table_totals(const Blk *blk, uint32_t n_blk, uint32_t b, uint32_t tid, Each each, Merge merge)
{
    __shared__ uint64_t r_before[kTableBlock], r_total[kTableBlock];
    __shared__ uint32_t sbad;
    if (tid == 0) sbad = 0;
    uint64_t before = 0, total = 0;
    uint32_t bad = 0;
    for (uint32_t k = tid; k < n_blk; k += kTableBlock) {
        const Blk B = blk[k];
        total += B.chunks;
        before += k < b ? B.chunks : 0;
        bad |= B.bad;
        each(k, B);
    }
    r_before[tid] = before;
    r_total[tid] = total;
    __syncthreads();
    if (bad) atomicOr(&sbad, 1u);
    merge();
    for (uint32_t s = kTableBlock / 2; s > 0; s >>= 1) {
        if (tid < s) {
            r_before[tid] += r_before[tid + s];
            r_total[tid] += r_total[tid + s];
        }
        __syncthreads();
    }
    return TableTotals{r_before[0], r_total[0], sbad};
}
template <class Blk> __device__ __forceinline__ TableTotals table_totals(const Blk *blk, uint32_t n_blk, uint32_t b, uint32_t tid)
{
    return table_totals(blk, n_blk, b, tid, [](uint32_t, const Blk &) {}, [] {});
}
// The search levels: level k holds the start of every 16^k-th entry, up to level `top`.  A TU calls these for k = 0 .. kTableLevels - 1,
// on its own kernel argument: entry i's global start into level k if that level holds it ...
__device__ __forceinline__ void table_set_level(uint32_t *level, uint32_t k, uint32_t top, uint64_t i, uint64_t start)
{
    if (k <= top && (i & ((1ull << (4 * k)) - 1)) == 0) level[i >> (4 * k)] = (uint32_t)start;
}
// ... and, by 16 threads, the level of n keys padded with ~0 to a whole line of 16 keys: the descent reads 16 at a time
__device__ __forceinline__ void table_pad_level(uint32_t *level, uint64_t n, uint32_t k, uint32_t top, uint32_t tid)
{
    if (k <= top && n + tid < ((n + 15) & ~15ull)) level[n + tid] = ~0u;
}

// ---- stream --------------------------------------------------------------------------------------------------------------------------
// One level of the 16-ary descent: of line j's 16 children, the last whose start is <= g.  One s_load_dwordx16 when j is uniform.
__device__ __forceinline__ uint32_t table_descend(const uint32_t *level, uint32_t j, uint32_t g)
{
    const Keys16 keys = *as_const(reinterpret_cast<const Keys16 *>(level + 16u * j));
    uint32_t c = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) c += keys.v[t] <= g ? 1u : 0u;
    return 16u * j + c - 1u;
}

// where chunk g lies: offset of its chunk from the entry's origin, the cut in front of the body (chunk 0 only), its bytes
struct Span {
    uint64_t off;
    uint32_t cut, bytes;
};
// ... from a View with lo (the global chunk that is the entry's chunk 0), lead and end
template <uint32_t CHUNK, class View> __device__ __forceinline__ Span table_span(uint32_t g, uint32_t total, const View &v)
{
    if (g >= total) return Span{0, 0, 0}; // past the last entry: zero-size descriptors, loads give 0, stores drop
    const uint32_t c = g - v.lo;
    const uint64_t off = (uint64_t)c * CHUNK;
    const uint32_t cut = c ? 0u : v.lead;
    const uint64_t lim = v.end < off + CHUNK ? v.end : off + CHUNK;
    return Span{off, cut, (uint32_t)(lim - off - cut)};
}
// ... from a verifying View of global chunks [lo, hi) with lead_rem: bits 0..15 lead, bits 16..31 bytes of the last chunk, counted from its chunk
// origin (1 .. CHUNK), less 1
template <uint32_t CHUNK, class View> __device__ __forceinline__ Span table_span_packed(uint32_t g, uint32_t total, const View &v)
{
    static_assert(CHUNK == 65536, "two offsets in a chunk packed into 32 bits");
    if (g >= total) return Span{0, 0, 0}; // past the last entry: zero-size descriptors, loads give 0
    Span s;
    const uint32_t c = g - v.lo;
    s.off = (uint64_t)c * CHUNK;
    s.cut = c ? 0u : v.lead_rem & 0xFFFFu;
    s.bytes = (c + 1u == v.hi - v.lo ? (v.lead_rem >> 16) + 1u : CHUNK) - s.cut;
    return s;
}
template <class Plan> __device__ __forceinline__ uint32_t table_lead_rem(const Plan &P)
{
    return P.lead | ((uint32_t)(P.end - (uint64_t)(P.chunks - 1u) * kChunk) - 1u) << 16;
}

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

// a stream kernel's name as a profiler prints it.  One buffer per <U, BLOCK>, written once from the first stem it is called with: a TU
// has one stream kernel and calls this with that kernel's stem only.
template <int U, int BLOCK> const char *table_kernel_name(const char *stem)
{
    static char buf[96];
    static const int n = std::snprintf(buf, sizeof buf, "%s<%d, %d>", stem, U, BLOCK);
    (void)n;
    return buf;
}

// ---- two keystreams ------------------------------------------------------------------------------------------------------------------
// The identity keystream (a key == 0 mod 2^31-1) is kept as the state 2^31-1 rather than 0 (cycle_rekey_table_kernel.hip says why).
// x * y mod m for a state x (canonical, or 2^31-1 for the identity keystream) and a power y of a.  The fold gives x*y mod m or that
// + m; for x = 2^31-1 it gives 2^31-1 exactly.  Bit 31 set is the excess (r + m >= 2^31 for r >= 1), so 2^31-1 is kept.
__device__ __forceinline__ uint32_t mulmod_keep(uint32_t x, uint32_t y)
{
    const uint32_t X = mul_fold(x, 2u * y);
    return X >= 0x80000000u ? X - lcg::M : X;
}

// the state of stream byte o1 - 1 (o1 = off mod period + 1 + position, reduced) under key residue k; the identity keeps 2^31-1
__device__ __forceinline__ uint32_t state_at(uint32_t k, uint64_t e) { return k ? mulmod_canon(k, pow_a((uint32_t)(e % lcg::PERIOD))) : lcg::M; }

// a rekey entry: the laid fields and the SIX states -- head, body and tail for each keystream, the body's counted from the chunk origin
template <class Plan, class Edge, class Entry> __device__ __forceinline__ void rekey_table_plan_entry(Plan &P, Edge &X, const Entry &E, const TableGrid &g)
{
    const uint32_t kf = key_res(E.key_from), kt = key_res(E.key_to);
    const uint64_t of = E.off_from % lcg::PERIOD + 1, ot = E.off_to % lcg::PERIOD + 1;
    const uint64_t body = g.head + lcg::PERIOD - g.lead, after = g.head + (g.words * 16) % lcg::PERIOD;
    table_lay(P, E, g);
    P.base_from = state_at(kf, of + body);
    P.base_to = state_at(kt, ot + body);
    X.head[0] = state_at(kf, of);
    X.head[1] = state_at(kt, ot);
    X.tail[0] = state_at(kf, of + after);
    X.tail[1] = state_at(kt, ot + after);
}

// ---- verifying -----------------------------------------------------------------------------------------------------------------------
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

// ---- digesting ----------------------------------------------------------------------------------------------------------------------
// (the verify table TU's digest loop and the out-of-place table TU's cycle digest loop; cycle_table_kernel.h: DigestTableRecord)
// byte sum and position sum (byte i of the word weighs i) of one 16-byte word: one v_dot4_u32_u8 per dword and weight.  The five
// weights live in VGPRs: v_dot4 takes no literal, and as hoisted scalar constants they cost the stream kernel an SGPR spill.
struct DotWeights {
    uint32_t ones, p0, p1, p2, p3;
};
__device__ __forceinline__ DotWeights dot_weights()
{
    DotWeights k;
    asm("v_mov_b32 %0, 0x01010101" : "=v"(k.ones));
    asm("v_mov_b32 %0, 0x03020100" : "=v"(k.p0));
    asm("v_mov_b32 %0, 0x07060504" : "=v"(k.p1));
    asm("v_mov_b32 %0, 0x0B0A0908" : "=v"(k.p2));
    asm("v_mov_b32 %0, 0x0F0E0D0C" : "=v"(k.p3));
    return k;
}
__device__ __forceinline__ void word_sums(const u32x4 &d, const DotWeights &k, uint32_t &b, uint32_t &w)
{
    b = __builtin_amdgcn_udot4(d.x, k.ones, 0u, false);
    b = __builtin_amdgcn_udot4(d.y, k.ones, b, false);
    b = __builtin_amdgcn_udot4(d.z, k.ones, b, false);
    b = __builtin_amdgcn_udot4(d.w, k.ones, b, false);
    w = __builtin_amdgcn_udot4(d.x, k.p0, 0u, false);
    w = __builtin_amdgcn_udot4(d.y, k.p1, w, false);
    w = __builtin_amdgcn_udot4(d.z, k.p2, w, false);
    w = __builtin_amdgcn_udot4(d.w, k.p3, w, false);
}
// x mod 65521 for any 64-bit x, without a 64-bit division: 2^16 = 15 (mod 65521), so the four 16-bit pieces of x weigh 1, 15, 225 and
// 3375 -- their weighted sum is below 65536 * 3616 < 2^28 and one 32-bit remainder finishes it
__device__ __forceinline__ uint32_t digest_red(unsigned long long x)
{
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    return ((lo & 0xFFFFu) + 15u * (lo >> 16) + 225u * (hi & 0xFFFFu) + 3375u * (hi >> 16)) % kDigestTableMod;
}
// The sum of x over the wave's 64 lanes, in lane 63 (other lanes hold partial sums): the row_shr / row_bcast DPP ladder, so that no
// lane index is needed (v_mbcnt is what this TU's guard reads as a rewritten ticket atomic).  A lane the control leaves without a
// source adds 0 (old = 0, bound_ctrl off).  x < 2^26 in every lane: no carry is lost.
__device__ __forceinline__ uint32_t wave_sum_lane63(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false); // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false); // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false); // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false); // row_shr:8: lane 15 of a row has the row's sum
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false); // row_bcast:15 into rows 1 and 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false); // row_bcast:31 into rows 2 and 3
    return x;
}

} // namespace
