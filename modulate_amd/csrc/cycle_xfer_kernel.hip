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
// One span of a piece: `len` bytes src -> dst, the first with state sp.  The grid of 16-byte words sits on dst: the < 16 bytes in front
// of its first aligned word and behind its last go bytewise, so a whole-word store never reaches outside [dst, dst + len).
template <bool UP, bool FUNNEL>
__device__ __forceinline__ void xfer_span(uint8_t *const dst, const uint8_t *const src, const uint32_t len, const uint32_t sp, const uint32_t copy, const uint32_t tid)
{
    constexpr int SAUX = UP ? (AUX_NT | AUX_SC1) : AUX_SC1; // HBM: streaming write-through; across PCIe: write-through only
    const uint32_t lead = (16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u;
    const uint32_t head = lead < len ? lead : len;
    const uint32_t words = (len - head) / lcg::WORD;
    const uint32_t tail = len - head - words * lcg::WORD;
    // < 16 bytes in front of the destination's first aligned word (lanes 0..15) and behind its last (lanes 16..31), bytewise
    if (tid < head || (tid >= 16u && tid - 16u < tail)) {
        const uint32_t q = tid < 16u ? tid : head + words * lcg::WORD + (tid - 16u);
        dst[q] = copy ? src[q] : cycle_byte(src[q], state_in_piece(sp, q));
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
        if (!copy) w = cycle_word<1>(w, s);
        __builtin_amdgcn_raw_buffer_store_b128(w, rd, o, 0, SAUX);
        s = mulmod_canon(s, lcg::kTileLo.v[1]); // a^4096: the same lane, one trip on
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
                }
            }
            xfer_span<UP, FUNNEL>(UP ? sd : sh, UP ? sh : sd, sl, ss, sc, tid);
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
