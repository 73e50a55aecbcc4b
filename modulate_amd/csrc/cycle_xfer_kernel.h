// cycle_xfer_kernel.h -- launch interface of the TRANSFER kernels (cycle_xfer_kernel.hip): the cipher in flight between host memory
// (or a part file, through the library's page-locked slots) and a buffer the caller keeps in device memory.
//   upload    reads each byte across PCIe once (a slot, or the caller's page-locked pages), XORs it, writes it into the device buffer;
//   download  reads the device buffer in HBM, XORs, writes each byte across PCIe once (into a slot, or the caller's page-locked pages).
// ONE launch per call, on the host-fed protocol of cycle_feed_kernel.h: a workgroup draws a 32 KiB ticket in stream order, waits for its
// chunk's `ready` word, does the piece, and the workgroup that completes a chunk marks it `done`.  Upload: ready = "the host has filled the
// slot", done = "the host may refill it".  Download: ready = "the slot is free", done = "the host may drain it".  The give-up rules are the
// host-fed kernel's: `abort`, `patience_ticks`, work[1].  With the caller's page-locked pages as the host side (`ready` == nullptr) every
// chunk is ready at launch and nothing is counted: the kernel never waits for the host.
// Its own TU with a source hash of its own (modgpu_xfer_kernel_source_hash); the arithmetic is cycle_kernel_impl.h's (ALG 1, what runs
// across PCIe), the protocol constants cycle_feed_kernel.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_feed_kernel.h" // kFeedSlotsMax, kFeedPieceBytes, kFeedPiecesMax

// reporting only (modgpu_last_launch): a transfer launch, either direction (`bytes` = the call's)
constexpr int CYCLE_XFER = 6;

struct CycleXferArgs {
    uint8_t *slot[kFeedSlotsMax]; // staged: chunk k is at slot[(k % pipes) * 2 + (k / pipes) % 2] + slot_phase, as the device addresses it
    uint8_t *host;                // direct (ready == nullptr): the caller's page-locked bytes as the device addresses them, byte j at host + j
    uint8_t *dev;                 // the caller's device buffer, byte j at dev + j
    const uint32_t *ready;        // [chunks] host memory, written by the host; nullptr: direct, every chunk ready, nothing counted
    const uint32_t *abort;        // host memory: the call is lost, leave
    uint32_t *done;               // [chunks] host memory, written by the kernel (staged only)
    uint32_t *work;               // device memory, zero at launch: [0] ticket counter, [1] workgroups that gave up, [2 + k] pieces of chunk k finished
    uint64_t n;                   // bytes of the call
    uint64_t patience_ticks;      // longest wait for one chunk, in ticks of the 100 MHz wall clock
    uint32_t chunk_bytes;         // a multiple of kFeedPieceBytes; chunk_bytes + slot_phase fit in a slot
    uint32_t pipes;               // pipelines of the call (each owns two slots)
    uint32_t slot_phase;          // dev mod 16: a slot holds its chunk this far in, so that slot and device buffer are co-aligned mod 16
    uint32_t base;                // canonical state of the call's first byte
    uint32_t copy;                // 1: the identity keystream (key == 0 mod 2^31-1): the bytes are copied unchanged
    // list mode (modgpu_launch_cycle_xfer_list; nullptr otherwise): the call's stream is the PACKED stream of a list of ranges
    const struct XferListRec *list; // device memory: list_n records in packed order, then a terminator
    uint32_t list_n;
    // digest mode of a list launch (modgpu_launch_cycle_xfer_list_digest; nullptr / 0 otherwise): one record of sums per entry of the caller's list
    struct XferDigestRecord *records;       // device memory: the caller's records, {0, 0, n, 0} at the first launch of the call
    uint32_t side;                          // MODGPU_DIGEST_OUTPUT (0): the sums are of what is stored; MODGPU_DIGEST_INPUT (1): of the source as read
    const struct XferListDigestRec *digest; // device memory: parallel to `list`, list_n of them
};

// LIST MODE (modgpu_cycle_host_to_device_list / modgpu_cycle_device_to_host_list): the stream of the call is the entries' bytes laid end to
// end, entry e from packed position start[e]; a slot holds its chunk of the packed stream from its first byte (slot_phase 0), `n` is the
// list's total, `dev`, `base` and `copy` are not used.  A workgroup that has drawn a piece finds the last record whose start is not
// behind the piece by a uniform binary search (bounded by list_n: a bad plan cannot send it out of the array) and walks the piece's
// SEGMENTS, one per entry that reaches into it: each is done like a piece of the plain call -- the 16-byte grid on the segment's
// destination, < 16 bytes bytewise at either edge, whole words through the v_alignbyte_b32 funnel, since slot position and device address
// of a segment share no phase -- with the state of its first byte taken from the entry's base.  Neighbouring segments share 16-byte words
// of a slot and neighbouring pieces belong to different workgroups: a whole-word store never reaches outside its own segment.  No barrier,
// no LDS and no wait are added; a piece is counted once, after every segment's stores have been fenced.  A piece full of tiny entries runs
// its segments one after another with few lanes busy: correct, and slow (a lane-parallel mapping for such runs is not built).
// A runtime mode of the two FUNNEL instantiations; the plain ones do not have the loop.
struct XferListRec {
    uint8_t *dev;   // the entry's device side, byte j of the entry at dev + j (terminator: nullptr)
    uint64_t start; // packed position of the entry's first byte; strictly increasing, record 0 at 0 (terminator: the list's total)
    uint32_t base;  // canonical state of the entry's first byte (modgpu_state_at's arithmetic)
    uint32_t copy;  // 1: this entry's key is 0 mod 2^31-1, its bytes are copied unchanged
};
constexpr int CYCLE_XFER_LIST = 21; // reporting only (modgpu_last_launch): a list transfer launch, either direction (`bytes` = the list's total)
constexpr uint64_t kXferListEntryMax = 1ull << 39; // an entry's bytes stay below this: its 32 KiB steps fit the three-byte jump tables

// DIGEST MODE of the list mode (modgpu_cycle_host_to_device_list_digest / modgpu_cycle_device_to_host_list_digest): every segment also sums
// the bytes of one side -- what it stores, or what it read -- while they are in registers: S1 = sum of x[j], S2 = sum of j * x[j], j counted
// from the ENTRY's first byte, both taken mod 65521 (include/modgpu.h: modgpu_digest_result_t; the sums are order-free, so any number of
// workgroups, launches and windows add onto one record).  A lane sums its words with v_dot4_u32_u8 and its edge byte by itself, relative to
// the segment's first byte; the segment's own position in its entry, (skip_mod + into) mod 65521, is folded in once per lane; each wave
// reduces across its lanes and ONE lane sends a pair of non-returning 64-bit atomic adds at agent scope onto records[entry].  No LDS, no
// barrier and no wait are added, and the atomics lie in front of the trip's closing fence.  A runtime mode behind one uniform branch whose
// flag is opaque on every trip: the loop body, and its one keystream block, are shared with the plain list mode.
struct XferDigestRecord { // modgpu_digest_result_t as the kernel sees it
    unsigned long long s1, s2, n, reserved;
};
struct XferListDigestRec {
    uint32_t entry;    // index of the plan record's entry in the caller's list: its record is records[entry]
    uint32_t skip_mod; // bytes of the entry in front of the plan record's first byte, mod 65521 (non-zero only for a record clipped by a window)
};
constexpr uint32_t kXferDigestMod = 65521u;
constexpr int CYCLE_XFER_LIST_DIGEST = 22; // reporting only (modgpu_last_launch): a digesting list transfer launch (`bytes` = the window's total)

// How a source whose phase differs from the destination's by a non-whole number of dwords is read (only the direct form can meet one:
// a staged chunk sits in its slot co-aligned with the device buffer):
//   XFER_PLAIN   one dwordx4 per word at the source's own address (dword-aligned)
//   XFER_FUNNEL  a dwordx4 at the dword below it and the dword after it, joined by v_alignbyte_b32 (cycle_to_kernel.hip's funnel)
enum XferForm : int { XFER_PLAIN = 0, XFER_FUNNEL = 1 };
uint32_t modgpu_xfer_block();
const char *modgpu_xfer_kernel_name(bool upload, int form);
hipError_t modgpu_launch_cycle_xfer(const CycleXferArgs &a, bool upload, int form, uint32_t grid, hipStream_t stream);
// a list launch (a.list set): always the funnel kernel of its direction.  A launch function of its own so that the CPU stand-in of the
// runtime can supply it from a file of its own.
hipError_t modgpu_launch_cycle_xfer_list(const CycleXferArgs &a, bool upload, uint32_t grid, hipStream_t stream);
// the same launch in digest mode (a.records, a.side and a.digest set as well).  Again a function of its own for the stand-in's sake.
hipError_t modgpu_launch_cycle_xfer_list_digest(const CycleXferArgs &a, bool upload, uint32_t grid, hipStream_t stream);
// The HIP device whose memory [p, p + n) is (both ends looked up with hipPointerGetAttributes), or -1: host memory, unknown, or
// the two ends on different devices.  Lives here so that the CPU stand-in of the runtime can supply its own.
int modgpu_xfer_device_of(const void *p, uint64_t n);
