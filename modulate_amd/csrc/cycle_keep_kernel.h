// cycle_keep_kernel.h -- launch interface of the work-queue kernel with a resident slice (cycle_keep_kernel.hip).  Its own TU with a
// source hash of its own (modgpu_keep_kernel_source_hash); the arithmetic is cycle_kernel_impl.h's (ALG 2).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel.h" // CycleQueueArgs

// The work-queue launch's arguments and the cache policy: a 64 KiB chunk at absolute address `addr` is stored so that it stays in
// the Infinity Cache when ((addr >> 16) & keep_mask) < keep_run, and streamed past it otherwise.  keep_run = 0: no chunk is kept.
struct CycleKeepArgs : CycleQueueArgs {
    uint32_t keep_mask; // a power of two minus one: the period of the pattern, in chunks
    uint32_t keep_run;  // chunks kept at the start of every period
};
uint32_t modgpu_keep_chunk_bytes();
uint32_t modgpu_keep_block();
const char *modgpu_keep_kernel_name();
hipError_t modgpu_launch_cycle_keep(const CycleKeepArgs &a, uint32_t grid, hipStream_t stream);
