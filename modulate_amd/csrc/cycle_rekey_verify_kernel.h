// cycle_rekey_verify_kernel.h -- launch interface of the REKEY VERIFY kernel (cycle_rekey_verify_kernel.hip): count the j with
// expect[j] != (src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j]) and find the lowest one, in ONE read-only pass over both
// buffers -- "is `expect` what the rekey kernel would have made of `src`?".  Nothing is written but the 32-byte result of each entry.
// Its own TU with a source hash of its own (modgpu_rekey_verify_kernel_source_hash); the two-keystream block is cycle_rekey_impl.h's,
// the result record and the launch that initialises it are the verify kernels' (cycle_verify_kernel.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_verify_kernel.h" // CycleVerifyResult, kVerifyNone, modgpu_launch_verify_init; kCycleBatchMax

// reporting only (modgpu_last_launch): a two-keystream compare launch, one or several entries
constexpr int CYCLE_REKEY_VERIFY = 12;

// One entry of a rekey verify launch: the verify kernel's entry (chunks on absolute chunk-aligned EXPECT addresses, the source at any
// phase) with two base states per piece, as the rekey kernel's: [0] for the keystream the source is under, [1] for the one `expect`
// should be under.  Both count positions from the same chunk origin, so the kernel's jumps are shared and only the bases differ.
struct CycleRekeyVerifyPart {
    const uint8_t *expect_body; // 16-byte aligned start of the comparand's body
    const uint8_t *src_body;    // the source byte that is compared with expect_body[0] (any alignment)
    CycleVerifyResult *result;  // device memory, initialised by modgpu_cycle_verify_init earlier on the same stream
    uint64_t n;                 // the entry's bytes: what result->n receives (from the workgroup that owns the entry's edges)
    uint64_t end;               // lead + body bytes, counted from the chunk origin (expect_body - lead)
    uint32_t lead;              // expect_body modulo the chunk size (the cut first chunk is workgroup p's, outside the index space)
    uint32_t base_body[2];      // states of the byte at the chunk origin
    uint32_t base_head[2], base_tail[2];
    uint32_t head_n, tail_n; // < 16 bytes before / after the body, compared bytewise
};
struct CycleRekeyVerifyArgs {
    uint32_t n_parts;                   // 1 .. kCycleBatchMax
    uint32_t start[kCycleBatchMax + 1]; // first global chunk index of each entry; start[n_parts] = total; unused entries = total
    CycleRekeyVerifyPart part[kCycleBatchMax];
};

// How the source is read: plain when (src - expect) mod 4 == 0 (dword-aligned dwordx4 loads), else the funnel (a dwordx4 at the dword
// below and the dword after it, joined by v_alignbyte_b32).  There is no identity form: entries whose two keystreams cancel, or of
// which only one is left, are the verify kernels' (modgpu_capi.cpp routes them).
enum CycleRekeyVerifyForm : int { CYCLE_REKEY_VERIFY_PLAIN = 0, CYCLE_REKEY_VERIFY_FUNNEL = 1 };
uint32_t modgpu_rekey_verify_chunk_bytes();
uint32_t modgpu_rekey_verify_block();
const char *modgpu_rekey_verify_kernel_name(int form);
// Static chunk assignment (workgroup b takes chunks b, b + grid, ...): no ticket, no scratch, nothing that can run out.
hipError_t modgpu_launch_cycle_rekey_verify(const CycleRekeyVerifyArgs &a, int form, uint32_t grid, hipStream_t stream);
