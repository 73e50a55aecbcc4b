// cycle_verify_table_kernel.h -- launch interface of the VERIFY TABLE kernels (cycle_verify_table_kernel.hip): a table of verify entries
// that lives in device memory, any number of them, in three launches whatever the count -- for entry i the count of the j with
// dst_i[j] != (src_i[j] ^ ks(key_i)[off_i + j]) and the lowest such j, dst being the comparand.  Nothing is written but the entries'
// results and the workspace.  Its own TU with a source hash of its own (modgpu_verify_table_kernel_source_hash); the keystream
// arithmetic is cycle_kernel_impl.h's (ALG 2).
//
// The entry is the table call's (CycleTableEntry), the per-entry record the table call's (CycleTablePlan, dst_origin read as the
// comparand's chunk origin), the result the verify call's (CycleVerifyResult).  The workspace is the table call's with one more line;
// its layout is planned on the host (modgpu_capi.cpp: verify_table_layout) and handed to every launch in VerifyTableArgs:
//   hdr     CycleTableHdr, the table call's own header: modgpu_table_status reads this kind of call's workspace too
//   sum     VerifyTableSummary, the line behind the header: the whole call's count and its lowest dirty entry (plan resets it)
//   blk     per 1024 entries: their chunk count and whether one of them is bad (plan -> finish)
//   plan    per entry: CycleTablePlan (plan -> finish, stream)
//   level   the 16-ary search levels of the chunk starts, as the table call's (finish -> stream)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_table_kernel.h"  // CycleTableEntry, CycleTableHdr, CycleTableBlk, CycleTablePlan and the table call's limits
#include "cycle_verify_kernel.h" // CycleVerifyResult, kVerifyNone

// reporting only (modgpu_last_launch): the stream launch of a verify table call
constexpr int CYCLE_VERIFY_TABLE = 11;
// ... and of a digest table call: the same three kernels with VerifyTableArgs::mode set (below)
constexpr int CYCLE_DIGEST_TABLE = 17;

// modgpu_verify_table_summary_t (include/modgpu.h) in its first 32 bytes; one line of the workspace
struct VerifyTableSummary {
    unsigned long long mismatches;      // sum of every entry's mismatches (finish: the edges; stream: the bodies)
    unsigned long long first_bad_entry; // lowest entry index with a mismatch, kVerifyNone if none
    unsigned long long entries;         // n_entries of the call
    unsigned long long reserved;
    unsigned long long pad[4];
};
static_assert(sizeof(VerifyTableSummary) == 64, "one line");

// The DIGEST TABLE mode of the same three kernels (modgpu_digest_table_device): for entry i the record of
//   out[j] = src_i[j] ^ ks(key_i)[off_i + j]:  s1 = sum of out[j], s2 = sum of j * out[j] (both in pieces, each reduced mod 65521 by
// whoever sends it: only the residues mean anything), n, 0 -- modgpu_digest_result_t, closed on the host (modgpu_digest_adler32).
// `dst` of an entry is never looked at: the plan launch lays the entry on the chunk grid of its SOURCE (the body's source is then
// 16-byte aligned: no funnel), the finish launch sums the < 16 bytes at either end and stores the record whole, the stream kernel's
// second loop (one uniform branch on `mode`) sums the bodies and adds to the records with non-returning 64-bit atomic adds.
// The workspace is the table call's own (no summary line: `sum` is null).
// (DigestTableRecord and kDigestTableMod: cycle_table_kernel.h)
//
// The CHECK mode of the finish kernel alone (modgpu_digest_check_device): no table, no workspace of its own.  One thread per RECORD of a
// digest producer (this TU's digest mode, the out-of-place table TU's, or the digest call's): the record is closed as
// modgpu_digest_adler32 closes it and compared with expect[i].  One ballot per wave is the wave's word of the bitmap (stored whole where
// a bitmap is given); only a wave whose ballot is nonzero sends one 64-bit add (its popcount) and one 64-bit unsigned min (its lowest
// bad index) to the 32-byte summary `check`, which modgpu_launch_verify_init has made {0, kVerifyNone, 0, 0} earlier on the stream.
// `producer`, when given, is the header of the table call that wrote the records: if that call was refused (first_bad set) nothing is
// compared, the summary becomes {0, kVerifyNone, n, 1} and the bitmap is not touched.  One uniform branch at the top of the kernel.
enum VerifyTableMode : uint32_t { VERIFY_TABLE_COMPARE = 0u, VERIFY_TABLE_DIGEST = 1u, VERIFY_TABLE_CHECK = 2u };
// reporting only (modgpu_last_launch): the check launch of modgpu_digest_check_device
constexpr int CYCLE_DIGEST_CHECK = 19;

struct VerifyTableArgs {
    const CycleTableEntry *entries;
    uint64_t n;
    CycleTableHdr *hdr;
    VerifyTableSummary *sum;
    CycleTableBlk *blk;
    CycleTablePlan *plan;
    CycleVerifyResult *results;    // n results in the caller's device memory: stored whole by finish, added to and lowered by stream
    uint32_t *level[kTableLevels]; // level[k][j] = start of entry j * 16^k; unused levels nullptr
    uint64_t level_n[kTableLevels];
    uint32_t top;                  // highest level (<= 16 keys)
    uint32_t n_blk;                // ceil(n / 1024)
    uint32_t mode;                 // VERIFY_TABLE_COMPARE, or VERIFY_TABLE_DIGEST: `records` in place of `results`, `sum` null
    DigestTableRecord *records;    // n records in the caller's device memory: stored whole by finish, added to by stream
    // VERIFY_TABLE_CHECK only (everything above but n, mode and records -- which are only read -- is unused then):
    const uint32_t *expect;         // n expected Adler-32 values
    unsigned long long *bad_bits;   // ceil(n / 64) words, bit b of word w = entry 64 w + b is bad; nullptr: no bitmap wanted
    const CycleTableHdr *producer;  // the header of the table call that wrote the records; nullptr: the records are taken as they are
    CycleVerifyResult *check;       // the summary: {bad entries, lowest bad entry, n, 1 if the producer was refused}
};

uint32_t modgpu_verify_table_chunk_bytes();
uint32_t modgpu_verify_table_block();
const char *modgpu_verify_table_kernel_name();
// The three launches of one call, in this order on one stream.  Each returns hipGetLastError().
hipError_t modgpu_launch_verify_table_plan(const VerifyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_verify_table_finish(const VerifyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_verify_table_stream(const VerifyTableArgs &a, uint32_t grid, hipStream_t stream);
// The same three kernels with a.mode = VERIFY_TABLE_DIGEST: the three launches of a digest table call (any grid >= 1 gives the same sums)
hipError_t modgpu_launch_digest_table_plan(const VerifyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_digest_table_finish(const VerifyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_digest_table_stream(const VerifyTableArgs &a, uint32_t grid, hipStream_t stream);
// The finish kernel with mode = VERIFY_TABLE_CHECK on ceil(n / 1024) workgroups, n > 0: `summary` initialised by
// modgpu_launch_verify_init(summary, 1, stream) earlier on the same stream.  bad_bits and producer may be nullptr.
hipError_t modgpu_launch_digest_check(const DigestTableRecord *records, const uint32_t *expect, uint64_t n, const CycleTableHdr *producer,
                                      CycleVerifyResult *summary, unsigned long long *bad_bits, hipStream_t stream);
