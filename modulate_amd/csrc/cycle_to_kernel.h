// cycle_to_kernel.h -- launch interface of the OUT-OF-PLACE kernel (cycle_to_kernel.hip): dst = src ^ keystream, src left intact.
// Its own TU with a source hash of its own (modgpu_to_kernel_source_hash); the arithmetic is cycle_kernel_impl.h's (ALG 2).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel.h" // kCycleBatchMax

// reporting only (modgpu_last_launch): an out-of-place launch, one or several entries
constexpr int CYCLE_TO = 5;
// ... and a launch of the same kernels' digest loop (modgpu_digest_device / modgpu_digest_batch_device)
constexpr int CYCLE_TO_DIGEST = 16;

// One entry of an out-of-place launch.  The work-queue shape's part (CycleQueuePart) with two pointers: chunks sit on absolute
// chunk-aligned DESTINATION addresses, so the destination body is 16-byte aligned and the source body is wherever the same
// byte of the source lies -- any alignment.
struct CycleToPart {
    uint8_t *dst_body;       // 16-byte aligned start of the destination's body
    const uint8_t *src_body; // the source byte that goes to dst_body[0] (any alignment)
    uint64_t end;            // lead + body bytes: one past the body's last byte, counted from the chunk origin (dst_body - lead)
    uint32_t lead;           // dst_body modulo the chunk size (the cut first chunk is workgroup p's, outside the index space)
    uint32_t base_body;      // state of the byte at the chunk origin
    uint32_t base_head, base_tail;
    uint32_t head_n, tail_n; // < 16 bytes before / after the body, done bytewise
};
// The digest loop: the out-of-place pass whose destination is a sum.  For an entry of n output bytes out[j] = src[j] ^ ks[stream_off + j]
// the kernel adds, with 64-bit atomic adds and nothing else, onto a record the host has zeroed on the launch's stream:
//   s1 += sum of out[j], s2 += sum of j * out[j]   -- in pieces, each reduced mod 65521 by the workgroup that sends it, so only the
//   residues mod 65521 of the two words mean anything --, and n += the entry's n (once, by the workgroup that owns its edges).
// Adler-32 of out follows on the host: A = (1 + S1) mod 65521, B = (n + n * S1 - S2) mod 65521 (modgpu_digest_adler32).
// Chunks are assigned statically (workgroup b: chunks b, b + G, ...): no ticket, `queue` is not touched and may be null.
// An entry without a destination (digest only) is planned with its SOURCE in the destination's role: dst_body == src_body, nothing stored.
struct CycleToDigest {
    unsigned long long s1, s2, n, reserved;
};
constexpr uint32_t kDigestMod = 65521u; // the largest prime below 2^16 (Adler-32)
enum CycleToDigestMode : uint32_t { CYCLE_TO_DIGEST_ON = 1u, CYCLE_TO_DIGEST_IDENTITY = 2u }; // IDENTITY: out = src (key == 0 mod 2^31 - 1)
struct CycleToArgs {
    uint32_t *queue;      // {ticket counter, workgroups done}: a pair of the work-queue ring (modgpu_capi.cpp: queue_pair)
    uint32_t *queue_done; // host-visible word that receives queue_seq once the pair is clean again; nullptr: nobody waits
    uint32_t queue_seq;
    uint32_t n_parts;                   // 1 .. kCycleBatchMax
    uint32_t start[kCycleBatchMax + 1]; // first global chunk index of each entry; start[n_parts] = total; unused entries = total
    CycleToPart part[kCycleBatchMax];
    // the digest loop (below); all zero in a launch of the stream loop
    uint32_t digest;                       // 0: the stream loop; else CYCLE_TO_DIGEST_ON, | CYCLE_TO_DIGEST_IDENTITY
    uint32_t store_mask;                   // bit p: entry p has a destination of its own, out is stored as well as summed (fused)
    CycleToDigest *result[kCycleBatchMax]; // each entry's record, zeroed in stream order in front of the launch
};

// How the source is read when (src - dst) mod 4 != 0 (DESIGN.md 4.6 has the A/B):
//   CYCLE_TO_PLAIN   one buffer_load_dwordx4 per word at the source's own byte address (unaligned buffer access)
//   CYCLE_TO_FUNNEL  one dwordx4 at the dword-aligned address below it plus the dword after it, joined by v_alignbyte_b32
enum CycleToForm : int { CYCLE_TO_PLAIN = 0, CYCLE_TO_FUNNEL = 1 };
uint32_t modgpu_to_chunk_bytes();
uint32_t modgpu_to_block();
const char *modgpu_to_kernel_name(int form);
hipError_t modgpu_launch_cycle_to(const CycleToArgs &a, int form, uint32_t grid, hipStream_t stream);
// the same two kernels with a.digest set: the digest loop over a.part / a.result on `grid` workgroups (any grid >= 1 gives the same sums)
hipError_t modgpu_launch_cycle_to_digest(const CycleToArgs &a, int form, uint32_t grid, hipStream_t stream);
