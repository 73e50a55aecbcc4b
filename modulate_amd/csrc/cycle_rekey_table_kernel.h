// cycle_rekey_table_kernel.h -- launch interface of the REKEY TABLE kernels (cycle_rekey_table_kernel.hip): a table of rekey entries
// that lives in device memory, any number of them, in three launches whatever the count -- dst_i[j] = src_i[j] ^
// ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j].  Its own TU with a source hash of its own
// (modgpu_rekey_table_kernel_source_hash); the two-keystream block is cycle_rekey_impl.h's, the jump tables cycle_kernel_impl.h's.
//
// The workspace is the table call's (cycle_table_kernel.h) with one more section; its layout is planned on the host (modgpu_capi.cpp:
// rekey_table_layout) and handed to every launch in RekeyTableArgs:
//   hdr     CycleTableHdr, the table call's own header: modgpu_table_status reads either kind of call's workspace
//   blk     per 1024 entries: their chunk count and whether one of them is bad (plan -> finish)
//   plan    per entry: RekeyTablePlan, what the stream launch reads of it (plan -> finish, stream)
//   edge    per entry: RekeyTableEdge, the head and tail states only the finish launch reads (plan -> finish)
//   level   the 16-ary search levels of the chunk starts, as the table call's (finish -> stream)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_table_kernel.h" // CycleTableHdr, CycleTableBlk and the table call's limits: one workspace header for both calls

// reporting only (modgpu_last_launch): the stream launch of a rekey table call
constexpr int CYCLE_REKEY_TABLE = 9;

// One entry as the caller writes it (include/modgpu.h: modgpu_rekey_table_entry_t, 56 bytes)
struct RekeyTableEntry {
    uint8_t *dst;
    const uint8_t *src;
    uint64_t n;
    uint64_t off_from;
    uint64_t off_to;
    int32_t key_from;
    int32_t key_to;
    uint32_t flags;
    uint32_t reserved;
};
static_assert(sizeof(RekeyTableEntry) == 56, "the public entry layout");

// What the stream launch needs of an entry: one s_load_dwordx16.  A keystream whose key is 0 mod 2^31-1 is the identity; its state
// is kept as 2^31-1 itself (not 0), whose packed byte is 0xFF and whose keystream byte ~0xFF is 0, and every state derived from it
// stays 2^31-1 (mulmod_keep): the two-keystream block then needs no case of its own -- one identity stream applies the other, two are
// a copy, and two equal states cancel.
struct RekeyTablePlan {
    uint8_t *dst_origin;       // dst body - lead: the absolute chunk-aligned address the entry's chunk 0 starts at
    const uint8_t *src_origin; // the source byte that pairs with dst_origin (never dereferenced below the body)
    uint64_t end;              // lead + body bytes
    uint64_t start;            // plan: first chunk among the 1024 entries of its blk record; finish: first global chunk
    uint32_t lead;             // dst body modulo the chunk size
    uint32_t chunks;           // chunks of the body, the cut first one included (0: no body)
    uint32_t base_from;        // states at the chunk origin of the keystream removed and of the one applied
    uint32_t base_to;
    uint32_t bad;              // 1 if the device tier refused the entry
    uint32_t head_n, tail_n;   // < 16 bytes before / after the body (the finish launch does them)
    uint32_t pad;
};
static_assert(sizeof(RekeyTablePlan) == 64, "one s_load_dwordx16");

// The states of the bytes before and after the body, [0] removed and [1] applied: only the finish launch reads them
struct RekeyTableEdge {
    uint32_t head[2];
    uint32_t tail[2];
};
static_assert(sizeof(RekeyTableEdge) == 16, "four states");

// The REKEY DIGEST mode of the same three kernels (modgpu_rekey_digest_table_device): every entry is rekeyed as in the plain mode -- plan
// is the plain mode's, the grid on the DESTINATION -- and record i receives the digest of the entry's stored bytes
// (REKEY_TABLE_SIDE_OUTPUT), of its source bytes as read (REKEY_TABLE_SIDE_INPUT), or of src ^ ks(key_from), the plaintext between the
// two keystreams that exists in registers only (REKEY_TABLE_SIDE_PLAIN).  The finish launch sums the < 16 bytes at either end while it
// rekeys them and stores the record whole; the stream kernel's second loop (one uniform branch on `mode`) sums one word per word it
// stores and adds to the records with non-returning 64-bit atomic adds.  The record and its protocol are the cycle digest table
// call's (cycle_table_kernel.h: DigestTableRecord).
enum RekeyTableMode : uint32_t { REKEY_TABLE_PLAIN = 0u, REKEY_TABLE_DIGEST = 1u };
enum RekeyTableSide : uint32_t { REKEY_TABLE_SIDE_OUTPUT = 0u, REKEY_TABLE_SIDE_INPUT = 1u, REKEY_TABLE_SIDE_PLAIN = 2u };
// reporting only (modgpu_last_launch): the stream launch of a rekey digest table call
constexpr int CYCLE_REKEY_DIGEST_TABLE = 20;

struct RekeyTableArgs {
    const RekeyTableEntry *entries;
    uint64_t n;
    CycleTableHdr *hdr;
    CycleTableBlk *blk;
    RekeyTablePlan *plan;
    RekeyTableEdge *edge;
    uint32_t *level[kTableLevels]; // level[k][j] = start of entry j * 16^k; unused levels nullptr
    uint64_t level_n[kTableLevels];
    uint32_t top;                  // highest level (<= 16 keys)
    uint32_t n_blk;                // ceil(n / 1024)
    uint32_t mode;                 // REKEY_TABLE_PLAIN (side 0, records null), or REKEY_TABLE_DIGEST
    uint32_t side;                 // REKEY_TABLE_SIDE_OUTPUT / _INPUT / _PLAIN: which bytes the records are of
    DigestTableRecord *records;    // n records in the caller's device memory: stored whole by finish, added to by stream
};

uint32_t modgpu_rekey_table_chunk_bytes();
uint32_t modgpu_rekey_table_block();
const char *modgpu_rekey_table_kernel_name();
// The three launches of one call, in this order on one stream.  Each returns hipGetLastError().
hipError_t modgpu_launch_rekey_table_plan(const RekeyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_table_finish(const RekeyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_table_stream(const RekeyTableArgs &a, uint32_t grid, hipStream_t stream);
// The same three kernels with a.mode = REKEY_TABLE_DIGEST (a.side and a.records are the caller's): the three launches of a rekey digest
// table call (any grid >= 1 gives the same bytes and the same residues)
hipError_t modgpu_launch_rekey_digest_table_plan(const RekeyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_digest_table_finish(const RekeyTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_digest_table_stream(const RekeyTableArgs &a, uint32_t grid, hipStream_t stream);
