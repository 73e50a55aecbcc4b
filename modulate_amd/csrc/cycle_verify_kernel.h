// cycle_verify_kernel.h -- launch interface of the VERIFY kernels (cycle_verify_kernel.hip): count the j with
// expect[j] != (src[j] ^ ks[stream_off + j]) and find the lowest one, in ONE read-only pass over both buffers.  The library's only
// reduction: nothing is written but the 32-byte result of each entry.  Its own TU with a source hash of its own
// (modgpu_verify_kernel_source_hash); the arithmetic is cycle_kernel_impl.h's (ALG 2).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel.h" // kCycleBatchMax

// reporting only (modgpu_last_launch): a verify launch, one or several entries
constexpr int CYCLE_VERIFY = 10;

// modgpu_verify_result_t (include/modgpu.h), as the kernels see it
struct CycleVerifyResult {
    unsigned long long mismatches;
    unsigned long long first_mismatch;
    unsigned long long n;
    unsigned long long reserved;
};
constexpr unsigned long long kVerifyNone = ~0ull; // first_mismatch of a clean entry

// One entry of a verify launch: the out-of-place kernel's entry with `expect` in the destination's role -- chunks sit on absolute
// chunk-aligned EXPECT addresses, so the expect body is 16-byte aligned and the source body is wherever the same byte of the source
// lies -- and the entry's result.
struct CycleVerifyPart {
    const uint8_t *expect_body; // 16-byte aligned start of the comparand's body
    const uint8_t *src_body;    // the source byte that is compared with expect_body[0] (any alignment)
    CycleVerifyResult *result;  // device memory, initialised by modgpu_cycle_verify_init earlier on the same stream
    uint64_t n;                 // the entry's bytes: what result->n receives (from the workgroup that owns the entry's edges)
    uint64_t end;               // lead + body bytes, counted from the chunk origin (expect_body - lead)
    uint32_t lead;              // expect_body modulo the chunk size (the cut first chunk is workgroup p's, outside the index space)
    uint32_t base_body;         // state of the byte at the chunk origin (unused by the identity forms)
    uint32_t base_head, base_tail;
    uint32_t head_n, tail_n; // < 16 bytes before / after the body, compared bytewise
};
struct CycleVerifyArgs {
    uint32_t n_parts;                   // 1 .. kCycleBatchMax
    uint32_t start[kCycleBatchMax + 1]; // first global chunk index of each entry; start[n_parts] = total; unused entries = total
    CycleVerifyPart part[kCycleBatchMax];
};

// Forms of the stream kernel.  Bit 0: how the source is read -- plain when (src - expect) mod 4 == 0 (dword-aligned dwordx4 loads),
// else the funnel (a dwordx4 at the dword below and the dword after it, joined by v_alignbyte_b32: the out-of-place kernel's shipped
// form).  Bit 1: the identity keystream (key == 0 mod 2^31-1) -- a plain compare, no keystream block.
enum CycleVerifyForm : int { CYCLE_VERIFY_PLAIN = 0, CYCLE_VERIFY_FUNNEL = 1, CYCLE_VERIFY_IDENTITY = 2 };
uint32_t modgpu_verify_chunk_bytes();
uint32_t modgpu_verify_block();
const char *modgpu_verify_kernel_name(int form);
// every result of results[0 .. count) := {0, kVerifyNone, 0, 0}
hipError_t modgpu_launch_verify_init(CycleVerifyResult *results, uint64_t count, hipStream_t stream);
// Static chunk assignment (workgroup b takes chunks b, b + grid, ...): no ticket, no scratch, nothing that can run out.
hipError_t modgpu_launch_cycle_verify(const CycleVerifyArgs &a, int form, uint32_t grid, hipStream_t stream);
