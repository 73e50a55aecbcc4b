// cycle_table_kernel.h -- launch interface of the TABLE kernels (cycle_table_kernel.hip): a table of out-of-place entries that lives in
// device memory, any number of them, cycled in three launches whatever the count -- dst_i[j] = src_i[j] ^ ks(key_i)[off_i + j].
// Its own TU with a source hash of its own (modgpu_table_kernel_source_hash); the keystream arithmetic is cycle_kernel_impl.h's (ALG 2).
//
// Everything the launches schedule with lives in a WORKSPACE the caller owns (modgpu_table_workspace_bytes); its layout is planned on
// the host (modgpu_capi.cpp: table_layout) and handed to every launch in CycleTableArgs:
//   hdr     CycleTableHdr: the ticket counter, the lowest bad entry, the total of chunks
//   blk     per 1024 entries: their chunk count and whether one of them is bad (plan -> finish)
//   plan    per entry: CycleTablePlan (plan -> finish, stream)
//   level   the sorted chunk starts of the entries, level k holding every 16^k-th, each padded with ~0 to a multiple of 16 (finish ->
//           stream): a chunk's entry is found by a 16-ary descent of scalar loads, one s_load_dwordx16 per level
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// reporting only (modgpu_last_launch): the stream launch of a table call
constexpr int CYCLE_TABLE = 8;

constexpr uint32_t kTableBlock = 1024;          // threads of a plan / finish workgroup = entries per blk record
constexpr int kTableLevels = 6;                 // 16^5 * 16 >= kTableMaxEntries: levels 0..5 at most
constexpr uint64_t kTableMaxEntries = 1u << 22; // the finish launch reads every blk record in every workgroup: O((n / 1024)^2)
constexpr uint64_t kTableMaxEntryChunks = 1u << 24; // an entry's chunks from its chunk origin: the three-byte chunk jump tables (1 TiB)
constexpr uint64_t kTableMaxChunks = 1ull << 31;    // all entries' chunks: 32-bit tickets with room for a grid's overshoot
constexpr uint64_t kTableNoBad = ~0ull;

// One entry as the caller writes it (include/modgpu.h: modgpu_table_entry_t, 40 bytes)
struct CycleTableEntry {
    uint8_t *dst;
    const uint8_t *src;
    uint64_t n;
    uint64_t stream_off;
    int32_t key;
    uint32_t flags;
};
static_assert(sizeof(CycleTableEntry) == 40, "the public entry layout");

struct CycleTableHdr {
    uint32_t ticket; // the stream launch's ticket counter (0 at its start: the plan launch resets it)
    uint32_t pad0;
    uint64_t first_bad; // lowest entry the device refused, kTableNoBad if none (reset by plan, written by finish)
    uint64_t total;     // chunks of all entries; 0 if the call was refused (written by finish)
    uint64_t pad1[5];
};
static_assert(sizeof(CycleTableHdr) == 64, "one line");

struct CycleTableBlk {
    uint64_t chunks; // the chunk count of the 1024 entries of this record
    uint32_t bad;    // 1 if one of them is bad
    uint32_t pad;
};

// What the stream launch needs of an entry: its destination body on the chunk grid, the source byte paired with the body's first
// byte, and the state at the chunk origin.  One s_load_dwordx16.
struct CycleTablePlan {
    uint8_t *dst_origin;       // dst body - lead: the absolute chunk-aligned address the entry's chunk 0 starts at
    const uint8_t *src_origin; // the source byte that pairs with dst_origin (src body - lead; never dereferenced below the body)
    uint64_t end;              // lead + body bytes
    uint64_t start;            // plan: first chunk among the 1024 entries of its blk record; finish: first global chunk
    uint32_t lead;             // dst body modulo the chunk size
    uint32_t chunks;           // chunks of the body, the cut first one included (0: no body)
    uint32_t base;             // state at the chunk origin; 0 = the identity keystream (key == 0 mod 2^31-1): a copy
    uint32_t bad;              // 1 if the device tier refused the entry
    uint32_t head_n, tail_n;   // < 16 bytes before / after the body (the finish launch does them)
    uint32_t base_head, base_tail;
};
static_assert(sizeof(CycleTablePlan) == 64, "one s_load_dwordx16");

// The record of a digesting table call (modgpu_digest_result_t): s1 = sum of byte[j], s2 = sum of j * byte[j], both in pieces, each
// reduced mod 65521 by whoever sends it (only the residues mean anything), n, 0.  Closed on the host (modgpu_digest_adler32).
struct DigestTableRecord {
    unsigned long long s1, s2, n, reserved;
};
constexpr uint32_t kDigestTableMod = 65521u; // the largest prime below 2^16 (Adler-32)

// The CYCLE DIGEST mode of the same three kernels (modgpu_cycle_digest_table_device): every entry is cycled as in the plain mode --
// plan is the plain mode's, the grid on the DESTINATION -- and record i receives the digest of the entry's stored bytes
// (CYCLE_TABLE_SIDE_OUTPUT) or of its source bytes as read (CYCLE_TABLE_SIDE_INPUT).  The finish launch sums the < 16 bytes at either
// end while it cycles them and stores the record whole; the stream kernel's second loop (one uniform branch on `mode`) sums each word
// it stores, or the funnelled word it read, and adds to the records with non-returning 64-bit atomic adds.
enum CycleTableMode : uint32_t { CYCLE_TABLE_PLAIN = 0u, CYCLE_TABLE_DIGEST = 1u };
enum CycleTableSide : uint32_t { CYCLE_TABLE_SIDE_OUTPUT = 0u, CYCLE_TABLE_SIDE_INPUT = 1u };
// reporting only (modgpu_last_launch): the stream launch of a cycle digest table call
constexpr int CYCLE_DIGEST_CYCLE_TABLE = 18;

struct CycleTableArgs {
    const CycleTableEntry *entries;
    uint64_t n;
    CycleTableHdr *hdr;
    CycleTableBlk *blk;
    CycleTablePlan *plan;
    uint32_t *level[kTableLevels]; // level[k][j] = start of entry j * 16^k; unused levels nullptr
    uint64_t level_n[kTableLevels];
    uint32_t top;                  // highest level (<= 16 keys)
    uint32_t n_blk;                // ceil(n / 1024)
    uint32_t mode;                 // CYCLE_TABLE_PLAIN (side 0, records null), or CYCLE_TABLE_DIGEST
    uint32_t side;                 // CYCLE_TABLE_SIDE_OUTPUT / _INPUT: which side of the XOR the records are of
    DigestTableRecord *records;    // n records in the caller's device memory: stored whole by finish, added to by stream
};

uint32_t modgpu_table_chunk_bytes();
uint32_t modgpu_table_block();
const char *modgpu_table_kernel_name();
// The three launches of one call, in this order on one stream.  Each returns hipGetLastError().
hipError_t modgpu_launch_table_plan(const CycleTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_table_finish(const CycleTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_table_stream(const CycleTableArgs &a, uint32_t grid, hipStream_t stream);
// The same three kernels with a.mode = CYCLE_TABLE_DIGEST (a.side and a.records are the caller's): the three launches of a cycle digest
// table call (any grid >= 1 gives the same bytes and the same residues)
hipError_t modgpu_launch_cycle_digest_table_plan(const CycleTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_cycle_digest_table_finish(const CycleTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_cycle_digest_table_stream(const CycleTableArgs &a, uint32_t grid, hipStream_t stream);
