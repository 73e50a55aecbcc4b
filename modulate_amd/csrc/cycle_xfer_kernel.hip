// cycle_xfer_kernel.hip -- the transfer kernels (see cycle_xfer_kernel.h): upload (host -> device buffer) and download (device buffer ->
// host) with the cipher in flight, one pass over one direction of the link.  Its own TU: the arithmetic is cycle_kernel_impl.h's
// (cycle_word<1>, the Mersenne-fold multiply, the jump tables), the loop is the host-fed kernel's (cycle_feed_kernel.hip has the
// reasoning behind its shape: thread 0's one region in front of the first barrier, the ticket and the ok word read into scalar
// registers, the give-up rules), neither file changed.
//
// What differs from the host-fed kernel: a piece has a source and a destination, one in HBM and one across PCIe.  The grid of
// 16-byte words sits on the DESTINATION's addresses: the < 16 bytes in front of its first aligned word and behind its last are done
// bytewise, the words are stored whole and aligned.  A staged chunk sits in its slot at `slot_phase` = dev mod 16, so slot and device
// buffer are co-aligned and the source words are aligned too; only the caller's own page-locked pages (the direct form) can have a phase
// of their own, and then the source is read with cycle_to_kernel.hip's v_alignbyte_b32 funnel.  Loads nt; stores into HBM nt sc1,
// stores across PCIe sc1 without nt (cycle_feed_kernel.hip: nt stores across PCIe measured 15-20 % slower).
//
// LIST MODE (cycle_xfer_kernel.h: XferListRec) is a second loop of the two FUNNEL instantiations, behind one uniform branch: the piece
// is a piece of the packed stream of a list of ranges, and is done segment by segment, one xfer_span per entry that reaches into it.
// Its DIGEST MODE (cycle_xfer_kernel.h) sums each segment's bytes while they are in registers and adds the sums onto the entry's record.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#include "cycle_kernel_impl.h"
#include "cycle_xfer_kernel.h"

namespace {
constexpr uint32_t kNone = 0xFFFFFFFFu;

// The source side of a piece's words (cycle_to_kernel.hip's SrcRsrc): a descriptor and, for the funnel, the byte shift inside a dword.
// The funnel's extra dword of the last word is the aligned dword that holds the last source byte, so num_records grows by 4 whenever
// sh != 0 and never reaches past the source's own dwords.
struct SrcRsrc {
    __amdgpu_buffer_rsrc_t r;
    uint32_t sh;
};
template <bool FUNNEL> __device__ __forceinline__ SrcRsrc src_rsrc(const uint8_t *p, uint32_t bytes)
{
    if constexpr (FUNNEL) {
        const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
        return {__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p - sh), 0, (int)(bytes + (sh && bytes ? 4u : 0u)), 0x00020000), sh};
    } else {
        return {__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p), 0, (int)bytes, 0x00020000), 0u};
    }
}
template <bool FUNNEL> __device__ __forceinline__ u32x4 load_word(const SrcRsrc &s, uint32_t o)
{
    const u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(s.r, o, 0, AUX_NT);
    if constexpr (!FUNNEL) {
        return d;
    } else {
        const uint32_t e = __builtin_amdgcn_raw_buffer_load_b32(s.r, o + lcg::WORD, 0, AUX_NT);
        u32x4 w;
        w.x = __builtin_amdgcn_alignbyte(d.y, d.x, s.sh);
        w.y = __builtin_amdgcn_alignbyte(d.z, d.y, s.sh);
        w.z = __builtin_amdgcn_alignbyte(d.w, d.z, s.sh);
        w.w = __builtin_amdgcn_alignbyte(e, d.w, s.sh);
        return w;
    }
}
// state of the byte q bytes into a piece whose first byte has state sp (q < kFeedPieceBytes)
__device__ __forceinline__ uint32_t state_in_piece(uint32_t sp, uint32_t q)
{
    uint32_t st = mulmod_canon(sp, c_lane_pow.v[(q >> 4) & 255]);
    st = mulmod_canon(st, c_tile_lo.v[q >> 12]);
    for (uint32_t k = 0; k < (q & 15u); ++k) st = mulmod_canon(st, lcg::A);
    return st;
}
// ---- the digest mode's sums (cycle_xfer_kernel.h: DIGEST MODE; restated from the table kernels' helpers, this TU keeps its five files) ----
// byte sum and position sum (byte i of the word weighs i) of one 16-byte word: one v_dot4_u32_u8 per dword and weight.  The five weights
// live in VGPRs: v_dot4 takes no literal, and as hoisted scalar constants they cost these kernels an SGPR spill.
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
__device__ __forceinline__ uint32_t to_vgpr(uint32_t x)
{
    asm("" : "+v"(x));
    return x;
}
// a pointer into global memory (the kernel's arguments point nowhere else) whose two halves are held in vector registers
typedef __attribute__((address_space(1))) unsigned long long GlobalU64;
struct VgprPointer {
    uint32_t lo, hi;
    __device__ __forceinline__ GlobalU64 *at(uint32_t byte_offset) const { return (GlobalU64 *)(((uint64_t)hi << 32 | lo) + byte_offset); }
};
__device__ __forceinline__ VgprPointer vgpr_pointer(const void *p) { return {to_vgpr((uint32_t)(uintptr_t)p), to_vgpr((uint32_t)((uintptr_t)p >> 32))}; }
// x mod 65521 for any 32-bit x, in vector registers: floor(x / 65521) = (x * 0x80078071) >> 47 for every x < 2^32.  Multiplier and
// modulus are put into VGPRs by hand: v_mul_hi_u32 / v_mul_lo_u32 take no literal, and as hoisted scalar constants the two cost these
// kernels an SGPR spill (the list loop has next to no scalar register left, and vector registers to spare).
__device__ __forceinline__ uint32_t mod_adler(uint32_t x)
{
    uint32_t m, p;
    asm("v_mov_b32 %0, 0x80078071" : "=v"(m));
    asm("v_mov_b32 %0, 0xfff1" : "=v"(p));
    return x - (__umulhi(x, m) >> 15) * p;
}
// a 64-bit x folded to a 32-bit value of the same residue mod 65521, without a 64-bit division: 2^16 = 15 (mod 65521), so the four
// 16-bit pieces of x weigh 1, 15, 225 and 3375 -- their weighted sum is below 65536 * 3616 < 2^28
__device__ __forceinline__ uint32_t digest_fold(uint64_t x)
{
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    return (lo & 0xFFFFu) + 15u * (lo >> 16) + 225u * (hi & 0xFFFFu) + 3375u * (hi >> 16);
}
// The sum of x over the wave's 64 lanes, in lane 63 (other lanes hold partial sums): the row_shr / row_bcast DPP ladder.  A lane the
// control leaves without a source adds 0 (old = 0, bound_ctrl off).  Called at full EXEC; x < 2^26 in every lane: no carry is lost.
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
// What a span's sums are of and where they go (list mode's digest mode only; on == 0: no sums).  `in_mask`: all ones when the record is
// of the source as read, zero when of what is stored; `pos_mod`: the position of the span's first byte in its entry, mod 65521.  `on`
// is uniform and scalar; the others are uniform too but kept in VECTOR registers (to_vgpr, vgpr_pointer): the list loop has next to no
// scalar register left, and a vector register to spare for each.
struct SpanDigest {
    uint32_t on;
    GlobalU64 *rec; // the record's s1; its s2 follows
    uint32_t in_mask, pos_mod;
};

// One span of a piece: `len` bytes src -> dst, the first with state sp.  The grid of 16-byte words sits on dst: the < 16 bytes in front
// of its first aligned word and behind its last go bytewise, so a whole-word store never reaches outside [dst, dst + len).
template <bool UP, bool FUNNEL>
__device__ __forceinline__ void xfer_span(uint8_t *const dst, const uint8_t *const src, const uint32_t len, const uint32_t sp, const uint32_t copy, const uint32_t tid,
                                          const SpanDigest dg)
{
    constexpr int SAUX = UP ? (AUX_NT | AUX_SC1) : AUX_SC1; // HBM: streaming write-through; across PCIe: write-through only
    const uint32_t lead = (16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u;
    const uint32_t head = lead < len ? lead : len;
    const uint32_t words = (len - head) / lcg::WORD;
    const uint32_t tail = len - head - words * lcg::WORD;
    // digest mode: this lane's byte sum and position sum, positions counted from the span's first byte
    uint32_t c1 = 0u, c2 = 0u;
    // < 16 bytes in front of the destination's first aligned word (lanes 0..15) and behind its last (lanes 16..31), bytewise
    if (tid < head || (tid >= 16u && tid - 16u < tail)) {
        const uint32_t q = tid < 16u ? tid : head + words * lcg::WORD + (tid - 16u);
        const uint8_t x = src[q];
        const uint8_t y = copy ? x : cycle_byte(x, state_in_piece(sp, q));
        dst[q] = y;
        if constexpr (FUNNEL) {
            c1 = dg.on ? (dg.in_mask & x) | (~dg.in_mask & y) : 0u;
            c2 = q * c1;
        }
    }
    uint32_t sw = sp; // state of the first aligned word: sp * a^head
    for (uint32_t k = 0; k < head; ++k) sw = mulmod_canon(sw, lcg::A);
    uint32_t s = mulmod_canon(sw, c_lane_pow.v[tid]); // this lane's first word
    // the hardware range check (num_records = the piece's whole words) drops the lanes past the last word
    auto rd = __builtin_amdgcn_make_buffer_rsrc(dst + head, 0, (int)(words * lcg::WORD), 0x00020000);
    const SrcRsrc rs = src_rsrc<FUNNEL>(src + head, words * lcg::WORD);
    const uint32_t trips = (words + 255u) / 256u;
    for (uint32_t j = 0; j < trips; ++j) {
        const uint32_t o = (j * 256u + tid) * lcg::WORD;
        u32x4 w = load_word<FUNNEL>(rs, o);
        [[maybe_unused]] const u32x4 x = w;
        if (!copy) w = cycle_word<1>(w, s);
        __builtin_amdgcn_raw_buffer_store_b128(w, rd, o, 0, SAUX);
        s = mulmod_canon(s, lcg::kTileLo.v[1]); // a^4096: the same lane, one trip on
        if constexpr (FUNNEL) {
            uint32_t on = dg.on;
            asm volatile("" : "+v"(on)); // opaque on every trip: the word loop is not split into a summing and a plain copy (ONE keystream block per kernel)
            if (__builtin_amdgcn_readfirstlane(on)) {
                u32x4 y;
                y.x = (dg.in_mask & x.x) | (~dg.in_mask & w.x);
                y.y = (dg.in_mask & x.y) | (~dg.in_mask & w.y);
                y.z = (dg.in_mask & x.z) | (~dg.in_mask & w.z);
                y.w = (dg.in_mask & x.w) | (~dg.in_mask & w.w);
                uint32_t b, ws;
                word_sums(y, dot_weights(), b, ws);
                const bool inside = o < words * lcg::WORD; // (a lane past the last word loaded zeros, and stored nothing)
                b = inside ? b : 0u;
                ws = inside ? ws : 0u;
                c1 += b;
                c2 += (head + o) * b + ws;
            }
        }
    }
    if constexpr (FUNNEL) {
        if (dg.on) { // (uniform: every wave of the workgroup is here at full EXEC)
            // A lane's sums before the wave sum.  A span is at most a piece: at most 8 words of 16 bytes and one edge byte per lane, each byte
            // <= 255, at positions < 32768 -- c1 <= 8 * 16 * 255 + 255 < 2^16, c2 < 32768 * c1 < 2^31; with the span's own position
            // (< 65521) folded in, pos * c1 + c2 < 65521 * 32895 + 2^31 < 2^32.  Reduced mod 65521 both are below 2^16, 64 of them below 2^22.
            const uint32_t r1 = wave_sum_lane63(mod_adler(c1)), r2 = wave_sum_lane63(mod_adler(dg.pos_mod * c1 + c2));
            if ((tid & 63u) == 63u && (r1 | r2) != 0u) { // (a wave without bytes, or of zero bytes only, adds nothing)
                __hip_atomic_fetch_add(dg.rec, (unsigned long long)r1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(dg.rec + 1, (unsigned long long)r2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
} // namespace

template <bool UP, bool FUNNEL> __global__ __launch_bounds__(256) void modgpu_cycle_xfer_kernel(CycleXferArgs a)
{
    __shared__ uint32_t s_t, s_ok;
    const uint32_t tid = threadIdx.x;
    const bool staged = a.ready != nullptr;
    const uint32_t tpc = a.chunk_bytes / kFeedPieceBytes;
    const uint32_t n_tickets = (uint32_t)((a.n + kFeedPieceBytes - 1) / kFeedPieceBytes);
    const uint32_t n_chunks = (n_tickets + tpc - 1) / tpc;
    // digest mode of the list mode (FUNNEL only): the records, the plan's digest records and the side, uniform values in vector registers
    [[maybe_unused]] VgprPointer records{0u, 0u}, digest{0u, 0u};
    [[maybe_unused]] uint32_t in_mask = 0u;
    if constexpr (FUNNEL) {
        records = vgpr_pointer(a.records);
        digest = vgpr_pointer(a.digest);
        in_mask = to_vgpr(a.side != 0u ? ~0u : 0u);
    }
    uint32_t counted = kNone; // thread 0: the chunk of the piece this workgroup has finished and not yet counted (staged only)
    for (;;) {
        if (tid == 0) {
            if (counted != kNone) {
                const uint32_t pieces = counted + 1 < n_chunks ? tpc : n_tickets - counted * tpc;
                if (__hip_atomic_fetch_add(&a.work[2 + counted], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == pieces - 1)
                    __hip_atomic_store(&a.done[counted], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                counted = kNone;
            }
            const uint32_t t = atomicAdd(&a.work[0], 1u);
            uint32_t ok = 1;
            if (t < n_tickets && staged) {
                const uint32_t c = t / tpc;
                counted = c;
                const uint64_t since = wall_clock64();
                while (__hip_atomic_load(&a.ready[c], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
                    if (__hip_atomic_load(a.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u || wall_clock64() - since > a.patience_ticks ||
                        __hip_atomic_load(&a.work[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                        ok = 0;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(16);
                }
            }
            s_t = t;
            s_ok = ok;
        }
        __syncthreads();
        const uint32_t t = __builtin_amdgcn_readfirstlane(s_t), ok = __builtin_amdgcn_readfirstlane(s_ok);
        if (t >= n_tickets || !ok) {
            if (!ok && tid == 0) atomicAdd(&a.work[1], 1u);
            break;
        }
        const uint32_t c = t / tpc, piece = t - c * tpc;
        const uint64_t pos = (uint64_t)t * kFeedPieceBytes; // stream position of the piece's first byte
        uint8_t *const h = staged ? a.slot[(c % a.pipes) * 2u + (c / a.pipes) % 2u] + a.slot_phase + (uint64_t)piece * kFeedPieceBytes : a.host + pos;
        uint8_t *const d = a.dev + pos;
        const uint32_t len = (uint32_t)(a.n - pos < kFeedPieceBytes ? a.n - pos : kFeedPieceBytes);
        // state of the piece's first byte: base * a^(32768 * t), by the three bytes of t
        uint32_t sp = mulmod_canon(a.base, c_chunk_pow0<kFeedPieceBytes>.v[t & 255]);
        sp = mulmod_canon(sp, c_chunk_pow1<kFeedPieceBytes>.v[(t >> 8) & 255]);
        sp = mulmod_canon(sp, c_chunk_pow2<kFeedPieceBytes>.v[t >> 16]);
        // The spans of the piece: ONE, the piece itself -- or, in list mode (FUNNEL only, a uniform branch), one SEGMENT per entry that reaches
        // into this piece of the packed stream, from the last record whose start is not behind the piece's first byte.
        uint32_t e = 0, e_end = 1;
        if constexpr (FUNNEL) {
            if (a.list != nullptr) {
                uint32_t lo = 0, hi = a.list_n; // (record 0 starts at 0; the search never leaves [0, list_n) whatever the records hold)
                while (hi - lo > 1u) {
                    const uint32_t mid = lo + (hi - lo) / 2u;
                    if (a.list[mid].start <= pos) lo = mid;
                    else hi = mid;
                }
                e = lo;
                e_end = a.list_n;
            }
        }
        for (; e < e_end; ++e) {
            uint8_t *sd = d, *sh = h;
            uint32_t sl = len, ss = sp, sc = a.copy;
            SpanDigest dg{0u, nullptr, 0u, 0u};
            if constexpr (FUNNEL) {
                uint32_t listed = a.list != nullptr ? 1u : 0u;
                asm volatile("" : "+v"(listed)); // opaque on every trip: the loop is not split into a listed and a plain copy (ONE keystream block per kernel)
                if (__builtin_amdgcn_readfirstlane(listed)) {
                    const uint64_t end = pos + len;
                    const uint64_t es = a.list[e].start, en = a.list[e + 1].start; // (record list_n is the terminator: start = the total)
                    if (es >= end) break;
                    const uint64_t b = es > pos ? es : pos, f = en < end ? en : end;
                    if (f <= b) continue;
                    // state of the segment's first byte: the entry's base, the whole 32 KiB steps of the distance by the jump tables, the rest
                    // as inside a piece (a segment that begins inside the piece: distance 0, the base itself)
                    const uint64_t into = b - es;
                    const uint32_t steps = (uint32_t)(into / kFeedPieceBytes);
                    ss = mulmod_canon(a.list[e].base, c_chunk_pow0<kFeedPieceBytes>.v[steps & 255]);
                    ss = mulmod_canon(ss, c_chunk_pow1<kFeedPieceBytes>.v[(steps >> 8) & 255]);
                    ss = mulmod_canon(ss, c_chunk_pow2<kFeedPieceBytes>.v[(steps >> 16) & 255]);
                    ss = state_in_piece(ss, (uint32_t)(into % kFeedPieceBytes));
                    sd = a.list[e].dev + into;
                    sh = h + (b - pos);
                    sl = (uint32_t)(f - b);
                    sc = a.list[e].copy;
                    // digest mode: the segment's record, and the position of its first byte in its entry mod 65521 (a record clipped by a
                    // window begins skip_mod bytes into its entry)
                    uint32_t summing = records.lo | records.hi;
                    asm volatile("" : "+v"(summing)); // opaque on every trip, like `listed`
                    if (__builtin_amdgcn_readfirstlane(summing)) {
                        const unsigned long long g = *digest.at(e * (uint32_t)sizeof(XferListDigestRec)); // {entry, skip_mod}
                        dg.on = 1u;
                        dg.rec = records.at((uint32_t)g * (uint32_t)sizeof(XferDigestRecord)); // (MODGPU_TABLE_MAX_ENTRIES * 32 < 2^32)
                        dg.in_mask = in_mask;
                        dg.pos_mod = mod_adler((uint32_t)(g >> 32) + to_vgpr(digest_fold(into))); // (skip_mod < 65521)
                    }
                }
            }
            xfer_span<UP, FUNNEL>(UP ? sd : sh, UP ? sh : sd, sl, ss, sc, tid, dg);
        }
        __threadfence_system(); // this wave's stores have reached their memory ...
        __syncthreads();        // ... and every wave's have, before thread 0 counts the piece at the top of the next trip
    }
}

namespace {
template <bool UP, bool FUNNEL> struct XferShape {
    static void launch(const CycleXferArgs &a, uint32_t grid, hipStream_t stream)
    {
        hipLaunchKernelGGL((modgpu_cycle_xfer_kernel<UP, FUNNEL>), dim3(grid), dim3(256), 0, stream, a);
    }
    static const char *name() // as a profiler prints it
    {
        static char buf[96];
        static const int n = std::snprintf(buf, sizeof buf, "modgpu_cycle_xfer_kernel<%s, %s>", UP ? "true" : "false", FUNNEL ? "true" : "false");
        (void)n;
        return buf;
    }
};
} // namespace

uint32_t modgpu_xfer_block() { return 256u; }
const char *modgpu_xfer_kernel_name(bool upload, int form)
{
    if (upload) return form == XFER_FUNNEL ? XferShape<true, true>::name() : XferShape<true, false>::name();
    return form == XFER_FUNNEL ? XferShape<false, true>::name() : XferShape<false, false>::name();
}
hipError_t modgpu_launch_cycle_xfer(const CycleXferArgs &a, bool upload, int form, uint32_t grid, hipStream_t stream)
{
    if (upload) {
        if (form == XFER_FUNNEL) XferShape<true, true>::launch(a, grid, stream);
        else XferShape<true, false>::launch(a, grid, stream);
    } else {
        if (form == XFER_FUNNEL) XferShape<false, true>::launch(a, grid, stream);
        else XferShape<false, false>::launch(a, grid, stream);
    }
    return hipGetLastError();
}
hipError_t modgpu_launch_cycle_xfer_list(const CycleXferArgs &a, bool upload, uint32_t grid, hipStream_t stream)
{
    if (a.list == nullptr || a.list_n == 0 || a.ready == nullptr) return hipErrorInvalidValue; // (list mode is staged, and has records)
    if (upload) XferShape<true, true>::launch(a, grid, stream);
    else XferShape<false, true>::launch(a, grid, stream);
    return hipGetLastError();
}
hipError_t modgpu_launch_cycle_xfer_list_digest(const CycleXferArgs &a, bool upload, uint32_t grid, hipStream_t stream)
{
    if (a.records == nullptr || a.digest == nullptr || a.side > 1u) return hipErrorInvalidValue; // (digest mode has records and a side)
    return modgpu_launch_cycle_xfer_list(a, upload, grid, stream);
}

int modgpu_xfer_device_of(const void *p, uint64_t n)
{
    auto one = [](const void *q) -> int {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        return at.type == hipMemoryTypeDevice ? at.device : -1;
    };
    const int first = one(p);
    if (first < 0 || n <= 1) return first;
    return one(static_cast<const uint8_t *>(p) + (n - 1)) == first ? first : -1;
}
