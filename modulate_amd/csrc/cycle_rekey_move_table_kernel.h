// cycle_rekey_move_table_kernel.h -- launch interface of the REKEY MOVE TABLE kernels (cycle_rekey_move_table_kernel.hip): a table of
// rekey entries that lives in device memory, whose destinations may lie on top of ANY entry's source, moved with memmove rules in one
// pass over HBM -- dst_i[j] = SRC0_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j], SRC0 the memory as the call
// found it.  Its own TU with a source hash of its own (modgpu_rekey_move_table_kernel_source_hash); the two-keystream block is
// cycle_rekey_impl.h's, the jump tables cycle_kernel_impl.h's, the entry and edge records the rekey table call's.
//
// Which tables: DOWNWARD (every dst_i <= src_i) or UPWARD (every dst_i >= src_i), the non-empty entries listed by rising address with
// sources pairwise disjoint and destinations pairwise disjoint.  Positions: the global chunks in table order for a
// downward table, in reverse for an upward one; a chunk's destination then meets the source reads of LOWER positions only.
//
// Five launches, in this order on one stream:
//   plan    one thread per entry: the rekey table call's plan (checks, chunk grid, six base states), the previous non-empty entry of
//           each entry among its 1024, the first strictly downward / upward entry of the 1024; resets the header and every flag
//   finish  global starts; the direction (that of the first entry with dst != src); the rule above, each non-empty entry against the
//           non-empty one before it; the status; the search levels; the < 16 ragged bytes of each end rekeyed INTO SCRATCH -- read
//           before any launch of the call has written anything outside the workspace
//   window  one thread per chunk: the global chunks [lo, lo + n), all at lower positions, whose source reads (rounded out to whole
//           source dwords) meet the chunk's destination, by two binary searches over the chunks -- their sources rise with the index
//   move    persistent workgroups; positions are tickets from the header, drawn one at a time; a chunk's flag goes up once its source
//           is in registers, its stores wait for the flags of its window (cycle_rekey_kernel.hip's move loop, per chunk of a table)
//   place   one thread per entry: the ragged ends from scratch into place
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_rekey_table_kernel.h" // RekeyTableEntry, RekeyTableEdge, and through it the table call's limits

// reporting only (modgpu_last_launch): the move launch of a rekey move table call
constexpr int CYCLE_REKEY_MOVE_TABLE = 15;

// the longest a move workgroup polls one flag, in ticks of the constant 100 MHz clock (wall_clock64): 2 s, as the single move call's
constexpr uint64_t kMoveTableStallTicks = 200000000ull;

// The table call's header (CycleTableHdr: ticket, first_bad and total where modgpu_table_status and the stream kernels expect them)
// with this call's words in its padding.
struct MoveTableHdr {
    uint32_t ticket;    // the move launch's position counter (0 at its start: the plan launch resets it)
    uint32_t stalled;   // 0, or 1 + the global chunk whose wait ran out: that workgroup stored nothing from there on
    uint64_t first_bad; // lowest entry the device refused, kTableNoBad if none (reset by plan, written by finish)
    uint64_t total;     // chunks of all entries (written by finish); the later launches do nothing when first_bad is set
    uint32_t up;        // 1: an upward table, position p is chunk total - 1 - p
    uint32_t pad0;
    uint64_t pad1[4];
};
static_assert(sizeof(MoveTableHdr) == sizeof(CycleTableHdr) && offsetof(MoveTableHdr, first_bad) == offsetof(CycleTableHdr, first_bad) &&
                  offsetof(MoveTableHdr, total) == offsetof(CycleTableHdr, total),
              "modgpu_table_status reads this workspace too");

struct MoveTableBlk {
    uint64_t chunks;     // the chunk count of the 1024 entries of this record
    uint32_t bad;        // 1 if one of them is bad
    uint32_t last;       // 1 + the last non-empty entry among them (global index), 0 if all are empty
    uint32_t first_down; // the first entry among them with dst < src, ~0 if none
    uint32_t first_up;   // ... with dst > src
    uint32_t pad[2];     // a sweep of a relayout call: the chunk count of the 1024 entries with no entry filtered, low word first; else 0
};
static_assert(sizeof(MoveTableBlk) == 32, "two per line");

// RekeyTablePlan with the word the order check needs
struct MoveTablePlan {
    uint8_t *dst_origin;
    const uint8_t *src_origin;
    uint64_t end;
    uint64_t start;
    uint32_t lead;
    uint32_t chunks;
    uint32_t base_from;
    uint32_t base_to;
    uint32_t bad;
    uint32_t head_n, tail_n;
    uint32_t prev; // 1 + the previous non-empty entry among the 1024 of its blk record (local index), 0 if there is none
};
static_assert(sizeof(MoveTablePlan) == 64, "one s_load_dwordx16");

// the chunks a chunk waits for: flags[lo .. lo + n - 1]
struct MoveTableWin {
    uint32_t lo, n;
};

constexpr uint32_t kMoveTableScratch = 32; // bytes of scratch per entry: 16 for the head, 16 for the tail

struct MoveTableArgs {
    const RekeyTableEntry *entries;
    uint64_t n;
    uint64_t cap; // chunks the workspace has flags and windows for
    MoveTableHdr *hdr;
    MoveTableBlk *blk;
    MoveTablePlan *plan;
    RekeyTableEdge *edge;
    uint8_t *scratch;
    uint32_t *flags;
    MoveTableWin *win;
    uint32_t *level[kTableLevels];
    uint64_t level_n[kTableLevels];
    uint32_t top;
    uint32_t n_blk;
    uint32_t sweep; // 0: the move table call; 1, 2: sweep 0 (dst <= src) and sweep 1 (dst > src) of a relayout call, see below
};

// The RELAYOUT call (modgpu_rekey_relayout_table_device): a table whose entries slide BOTH ways, as two sweeps of the
// five launches above on one stream and one workspace.  An entry that slides down or stays never meets one that slides up (the lemma
// of 4.20), so the table is two same-direction tables interleaved; `sweep` is a mode of the plan and finish kernels that picks one:
//   plan    an entry of the other direction is FILTERED: planned as an empty entry -- no chunks, no ragged ends, nothing placed --
//           but it still counts as non-empty for the prev / last links the order check follows, it is still refused for what an
//           entry is refused for, and its chunks still count toward MoveTableBlk.pad, the UNFILTERED chunk sum of the record.
//           Sweep 1 keeps the header's `stalled` word as sweep 0 left it, and if it is set filters every entry: nothing more is stored.
//   finish  no direction clause: each non-empty entry against the non-empty one before it, whatever the direction of either; the
//           capacity check is made on the unfiltered sum, so both sweeps reach the same verdict; hdr->up = sweep - 1.
// Window, move and place run as they are: to them a filtered entry is an empty one.
constexpr uint32_t kRelayoutSweepDown = 1, kRelayoutSweepUp = 2;

uint32_t modgpu_rekey_move_table_chunk_bytes();
uint32_t modgpu_rekey_move_table_block();
const char *modgpu_rekey_move_table_kernel_name();
// The launches of one call, in this order on one stream.  Each returns hipGetLastError().
hipError_t modgpu_launch_rekey_move_table_plan(const MoveTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_move_table_finish(const MoveTableArgs &a, hipStream_t stream);
hipError_t modgpu_launch_rekey_move_table_window(const MoveTableArgs &a, hipStream_t stream);
// *grid comes in as the grid asked for and goes out as the grid launched: never more workgroups than the device holds at once
hipError_t modgpu_launch_rekey_move_table_move(const MoveTableArgs &a, uint32_t *grid, hipStream_t stream);
hipError_t modgpu_launch_rekey_move_table_place(const MoveTableArgs &a, hipStream_t stream);
// The plan and finish launches of one sweep of a relayout call (sweep = kRelayoutSweepDown or kRelayoutSweepUp; a.sweep is not looked
// at); the window, move and place launches above follow each pair.
hipError_t modgpu_launch_rekey_relayout_plan(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream);
hipError_t modgpu_launch_rekey_relayout_finish(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream);
