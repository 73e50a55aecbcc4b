// cycle_rekey_verify_table_kernel.h -- launch interface of the REKEY VERIFY TABLE kernels (cycle_rekey_verify_table_kernel.hip): a table
// of rekey entries that lives in device memory, any number of them, VERIFIED in three launches whatever the count -- for entry i the
// count of the j with dst_i[j] != (src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j]) and the lowest such j, dst
// being the comparand.  Nothing is written but the entries' results and the workspace.  Its own TU with a source hash of its own
// (modgpu_rekey_verify_table_kernel_source_hash); the two-keystream block is cycle_rekey_impl.h's, the jump tables
// cycle_kernel_impl.h's.
//
// The entry is the rekey table call's (RekeyTableEntry), the per-entry records the rekey table call's (RekeyTablePlan, dst_origin read
// as the comparand's chunk origin; RekeyTableEdge), the result the verify call's (CycleVerifyResult), the summary line the verify
// table call's (VerifyTableSummary).  The workspace is the rekey table call's with that one line more; its layout is planned on the
// host (modgpu_capi.cpp: rekey_verify_table_layout) and handed to every launch in RekeyVerifyTableArgs:
//   hdr     CycleTableHdr, the table call's own header: modgpu_table_status reads this kind of call's workspace too
//   sum     VerifyTableSummary, the line behind the header, where modgpu_verify_table_summary reads it (plan resets it)
//   blk     per 1024 entries: their chunk count and whether one of them is bad (plan -> finish)
//   plan    per entry: RekeyTablePlan (plan -> finish, stream)
//   level   the 16-ary search levels of the chunk starts, as the table call's (finish -> stream)
//   edge    per entry: RekeyTableEdge, the head and tail states only the finish launch reads (plan -> finish)
// in this order in memory: rekey_table_layout's order (the edge states behind the levels) with the summary line put in behind the header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_table_kernel.h"  // RekeyTableEntry, RekeyTablePlan, RekeyTableEdge; through it the table call's header and limits
#include "cycle_verify_table_kernel.h" // VerifyTableSummary; through it CycleVerifyResult, kVerifyNone

// reporting only (modgpu_last_launch): the stream launch of a rekey verify table call
constexpr int CYCLE_REKEY_VERIFY_TABLE = 13;

struct RekeyVerifyTableArgs {
    const RekeyTableEntry *entries;
    uint64_t n;
    CycleTableHdr *hdr;
    VerifyTableSummary *sum;
    CycleTableBlk *blk;
    RekeyTablePlan *plan;
    RekeyTableEdge *edge;
    CycleVerifyResult *results;    // n results in the caller's device memory: stored whole by finish, added to and lowered by stream
    uint32_t *level[kTableLevels]; // level[k][j] = start of entry j * 16^k; unused levels nullptr
    uint64_t level_n[kTableLevels];
    uint32_t top;                  // highest level (<= 16 keys)
    uint32_t n_blk;                // ceil(n / 1024)
};

uint32_t modgpu_rekey_verify_table_chunk_bytes();
uint32_t modgpu_rekey_verify_table_block();
const char *modgpu_rekey_verify_table_kernel_name();
// The three launches of one call, in this order on one stream.  Each returns hipGetLastError().
hipError_t modgpu_launch_rekey_verify_table_plan(const RekeyVerifyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_verify_table_finish(const RekeyVerifyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_verify_table_stream(const RekeyVerifyTableArgs &a, uint32_t grid, hipStream_t stream);
