// cycle_rekey_kernel.h -- launch interface of the REKEY kernel (cycle_rekey_kernel.hip): dst = src ^ ks(key_from)[off_from + j] ^
// ks(key_to)[off_to + j], ciphertext under one keystream to ciphertext under another in ONE pass, the plaintext only in registers.
// Its own TU with a source hash of its own (modgpu_rekey_kernel_source_hash); the two-keystream block is cycle_rekey_impl.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel.h" // kCycleBatchMax

// reporting only (modgpu_last_launch): a rekey launch, one or several entries; the body launch of an overlapping move
constexpr int CYCLE_REKEY = 7;
constexpr int CYCLE_REKEY_MOVE = 14;

// One entry of a rekey launch: the out-of-place kernel's entry (chunks on absolute chunk-aligned DESTINATION addresses, the source
// at any phase) with two base states per piece, [0] for the keystream being removed and [1] for the one being applied.  Both count
// positions from the same chunk origin, so the kernel's jumps (lane, tile, chunk) are shared: only the bases differ.
struct CycleRekeyPart {
    uint8_t *dst_body;       // 16-byte aligned start of the destination's body
    const uint8_t *src_body; // the source byte that goes to dst_body[0] (any alignment)
    uint64_t end;            // lead + body bytes, counted from the chunk origin (dst_body - lead)
    uint32_t lead;           // dst_body modulo the chunk size (the cut first chunk is workgroup p's, outside the index space)
    uint32_t base_body[2];   // states of the byte at the chunk origin
    uint32_t base_head[2], base_tail[2];
    uint32_t head_n, tail_n; // < 16 bytes before / after the body, done bytewise
};
struct CycleRekeyArgs {
    uint32_t *queue;      // {ticket counter, workgroups done}: a pair of the work-queue ring (modgpu_capi.cpp: queue_pair)
    uint32_t *queue_done; // host-visible word that receives queue_seq once the pair is clean again; nullptr: nobody waits
    uint32_t queue_seq;
    uint32_t n_parts;                   // 1 .. kCycleBatchMax
    uint32_t start[kCycleBatchMax + 1]; // first global chunk index of each entry; start[n_parts] = total; unused entries = total
    CycleRekeyPart part[kCycleBatchMax];
    // ---- the MOVE loop (modgpu_rekey_move_device: [dst, dst+n) partly overlaps [src, src+n)); move_flags == nullptr: the ordinary pass.
    // One entry with lead 0 and no edges.  Chunks are handed out in POSITION order by tickets alone (no static prefix: every position
    // belongs to a workgroup that is running); position p is chunk p (move_down == 0: dst < src, walking up) or chunk total-1-p
    // (dst > src, walking down).  move_flags[c] becomes 1 once chunk c's source is in registers; chunk c is stored once the flags of
    // chunks c + move_win_lo .. c + move_win_lo + move_win_n - 1 (those inside the entry) are up: the chunks, other than c, whose
    // source reads meet c's destination.  All of them are at lower positions.
    uint32_t *move_flags;
    uint32_t *move_status; // 0, or 1 + the chunk whose wait ran out (kRekeyMoveStallTicks): that workgroup stored nothing from there on
    uint32_t move_down;
    int32_t move_win_lo;
    uint32_t move_win_n; // 0 .. 3
};
// the longest a move workgroup polls one flag, in ticks of the constant 100 MHz clock (wall_clock64): 2 s, more than ten times the
// longest admissible pass.  A bug is an error (modgpu_move_status), not a hang.
constexpr uint64_t kRekeyMoveStallTicks = 200000000ull;

// How the source is read: CYCLE_REKEY_PLAIN when (src - dst) mod 4 == 0 (dword-aligned dwordx4 loads), else CYCLE_REKEY_FUNNEL
// (a dwordx4 at the dword below and the dword after it, joined by v_alignbyte_b32 -- the out-of-place kernel's shipped form).
enum CycleRekeyForm : int { CYCLE_REKEY_PLAIN = 0, CYCLE_REKEY_FUNNEL = 1 };
// Launch shapes (DESIGN.md 4.7 has the A/B): the same kernel, the grid differs.
//   CYCLE_REKEY_SHAPE_QUEUE  the out-of-place kernel's grid: 25 main workgroups per 32 CUs (200 on MI355X)
//   CYCLE_REKEY_SHAPE_ALL    one workgroup per CU on every CU (256): a VALU-bound pass wants every SIMD
enum CycleRekeyShape : int { CYCLE_REKEY_SHAPE_QUEUE = 0, CYCLE_REKEY_SHAPE_ALL = 1 };
uint32_t modgpu_rekey_chunk_bytes();
uint32_t modgpu_rekey_block();
const char *modgpu_rekey_kernel_name(int form);
hipError_t modgpu_launch_cycle_rekey(const CycleRekeyArgs &a, int form, uint32_t grid, hipStream_t stream);
// The same kernel on its move loop (a.move_flags != nullptr).  *grid comes in as the grid asked for and goes out as the grid launched:
// never more workgroups than the device holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs).
hipError_t modgpu_launch_cycle_rekey_move(const CycleRekeyArgs &a, int form, uint32_t *grid, hipStream_t stream);
