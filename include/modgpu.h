/*
 * modgpu.h -- C ABI of the MI355X (gfx950) implementation of Modulate's cipher hot path.
 *
 * The reference (AdamClixby/Modulate) has no FFI or plugin interface; the seam it offers is
 * one C++ class,
 *
 *     class CEncryptionCycler { public: void Cycle(unsigned char*, unsigned int, int); ... };
 *                                                  (Modulate/CEncryptionCycler.h:3-10)
 *
 * called from exactly three places, always as  Cycle(buf + 4, size - 4, key):
 *     Modulate/CArk.cpp:338-339     CArk::Load            (header decrypt)
 *     Modulate/CArk.cpp:1135-1136   CArk::SaveArk         (header encrypt)
 *     Modulate/Modulate.cpp:485-486 Decode                (-decode command)
 *
 * This header is what that class's body binds to (modulate_amd/csrc/host/CEncryptionCycler.cpp is
 * the binding; INTEGRATION.md shows the same stub for the upstream tree).  Plain pointers and
 * sizes only; no C++ or torch types.  Every function returns MODGPU_OK (0) or a MODGPU_ERR_*
 * code, never throws, never prints; modgpu_last_error() gives the text for the calling thread.
 *
 * Semantics (bit-exact with Modulate/CEncryptionCycler.cpp:4-25):
 *     ks[i]  = low8( a^(i+1) * key mod (2^31-1) ) ^ 0xFF        a = 16807, residue 0 -> 2^31-1
 *     buf[j] ^= ks[stream_off + j]                               j = 0 .. n-1
 * stream_off = 0 reproduces one reference Cycle call.  n and stream_off are 64-bit, which lifts
 * the reference's `unsigned int` length cap (2^32-1) and lets one logical stream be split over
 * calls or devices.  Keys congruent to 0 mod 2^31-1 give the identity, as in the reference.
 *
 * Which engine computes.  Every modgpu_cycle_* / modgpu_hdr_* entry point below runs the gfx950
 * kernel and NOTHING ELSE: without a usable HIP device they fail with MODGPU_ERR_NO_DEVICE /
 * MODGPU_ERR_HIP.  The two exceptions are named for what they are:
 *     modgpu_cycle_scalar_host   the library's own host loop (never the GPU)
 *     modgpu_cycle_auto_host     the reference's "Cycle cannot fail" contract and its size dispatch: the
 *                                host loop for buffers below MODGPU_MIN_GPU_BYTES (header-sized: a kernel
 *                                launch costs more than the arithmetic) or when no GPU is usable, else the GPU
 * modgpu_path_stats() counts calls and bytes per engine, and MODGPU_REQUIRE_GPU=1 in the environment
 * forbids the host loop altogether (both entry points then fail with MODGPU_ERR_FORBIDDEN instead of
 * computing), so a test-suite or benchmark can prove which engine produced its bytes.
 *
 * Threading: callable concurrently from any number of host threads.  `device` selects the GPU
 * per call (-1 = the calling thread's current HIP device); no global "current device" is
 * relied on, and a call made with an explicit device leaves the calling thread's current HIP
 * device as it found it.  Host-buffer calls to the same device run side by side, each on staging slots of its own (a call
 * that finds too few free takes fewer pipelines; one that finds none waits for a release).  The library keeps parked worker
 * threads (for the staging pipelines per device and per NUMA node a caller's pages have been found on -- slots and workers sit
 * on the node of the pages they copy, only the GPU crosses the socket link; one pool for the host loop): started on first use,
 * never joined.
 *
 * Environment (each read once, when first needed) -- these ten and no others (tests/test_capi_cpu.py compares this list with the
 * strings of the built library):
 *     MODGPU_REQUIRE_GPU=1       no host loop anywhere (see above)
 *     MODGPU_MIN_GPU_BYTES=n     modgpu_cycle_auto_host's size threshold (default 16 MiB, the measured crossover
 *                                against one host thread; 0 = always the GPU)
 *     MODGPU_HOST_POLICY=name    what modgpu_cycle_auto_host does ABOVE that threshold when a GPU is usable:
 *                                offload (default) = the kernel -- the host's cores stay free and every GPU adds a link;
 *                                fastest = per call, the engine the committed crossover table prices as faster for this
 *                                size and memory kind, the host loop with the threads it would really get
 *     MODGPU_HOST_ISA=name       host-loop body: generic | avx2 | avx512 (default: the best the CPU runs)
 *     MODGPU_HOST_THREADS=n      most host threads one host-loop call may use (default min(cores, 32); never more than the
 *                                control group's CPU quota or the caller's affinity mask allow)
 *     MODGPU_HOST_PIPES=n        pipelines (host threads) one host-buffer call spreads its staging copies over (1..16, default 8)
 *     MODGPU_HOST_CHUNK_MB=n     largest page-locked staging slot in MiB (1..256, default 8): 2 x pipelines of them per caller at work
 *     MODGPU_DEVICE_ALIAS=n      see modgpu_device_count
 *     MODGPU_NUMA=0              do not place host memory and worker threads next to their GPU
 *     MODGPU_HELPER_BELOW_MHZ=n  shader clock below which the helper workgroups of a large launch join in (default: 77 % of the
 *                                device's peak shader clock, 1 848 MHz on MI355X; 0 = never)
 * (How a staged stream is cut and queued -- chunk count, ramp, lanes, copy flavour, ring depth -- and the host loop's binding and
 * control-group switches were environment variables until ABI 6.  They are constants now, the values the committed profiles
 * chose; the testing flavour of the library, libmodgpu_testing.so, still has them as knobs: include/modgpu_testing.h.)
 */
#ifndef MODGPU_H
#define MODGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MODGPU_OK 0
#define MODGPU_ERR_INVALID 1   /* bad argument (null pointer with n > 0, bad device index ...) */
#define MODGPU_ERR_NO_DEVICE 2 /* no HIP device visible                                        */
#define MODGPU_ERR_HIP 3       /* a HIP runtime call failed; see modgpu_last_error()           */
#define MODGPU_ERR_MAGIC 4     /* header magic is neither PS3 nor PS4 (eError_UnknownVersionNumber,
                                  Modulate/CArk.cpp:329-334, Modulate/Modulate.cpp:476-481)    */
#define MODGPU_ERR_IO 5        /* open / read / write of a part file failed (eError_FailedToOpenFile,
                                  eError_FailedToWriteData at Modulate/CArk.cpp:745-749, 883-889)     */
#define MODGPU_ERR_FORBIDDEN 6 /* the host loop was needed or asked for, and MODGPU_REQUIRE_GPU=1 forbids it */

/* Settings.h:16-20 */
#define MODGPU_MAGIC_PS3 0xc64eed30u
#define MODGPU_MAGIC_PS4 0x6f303f55u
#define MODGPU_KEY_PS3 0xc64eed30u
#define MODGPU_KEY_PS4 0x90cfc0abu

/* ABI version of this header (bumped on any signature change; ABI 8 also gained modgpu_cycle_device_to and
 * modgpu_cycle_batch_device_to, the four transfer calls modgpu_cycle_host_to_device & co., and modgpu_rekey_device_to and
 * modgpu_rekey_batch_device_to, and the table calls modgpu_cycle_table_device & co., and the rekey table calls
 * modgpu_rekey_table_device & co., and the verify calls modgpu_verify_device & co., and the verify table calls
 * modgpu_verify_table_device & co., and the rekey verify calls modgpu_verify_rekey_device and modgpu_verify_rekey_batch_device,
 * additions that change no existing signature). */
#define MODGPU_ABI_VERSION 8
int modgpu_abi_version(void);

/* Number of HIP devices this library addresses (0 if none / runtime unusable).  Normally the
 * devices visible to the process; with MODGPU_DEVICE_ALIAS=N in the environment (a rehearsal
 * switch for multi-GPU code on a box with fewer GPUs) it is N logical devices, logical device d
 * running on physical device d mod <visible>, each with its own staging context and worker. */
int modgpu_device_count(void);

/* Text of the last error raised on the calling thread ("" if none).  Never NULL. */
const char *modgpu_last_error(void);

/* ---- the hot path ------------------------------------------------------------------ */

/* Replaces the loop body of CEncryptionCycler::Cycle (CEncryptionCycler.cpp:9-13) for a buffer
 * that is already device-resident.  `dev_buf` may have any byte alignment (the reference's
 * callers pass buf+4).  Asynchronous on `hip_stream` (a hipStream_t; NULL = the device's
 * null stream); the caller synchronises.  This is the entry point the roofline is measured on.
 * Allocation-free and capturable into a hipGraph.  Any number of EAGER launches may be in flight at once, on any streams,
 * beside any number of graph replays: the scheduling scratch of a large launch (a ticket counter) is never shared between
 * two launches that could overlap -- an eager launch gets scratch whose previous user has finished, or a launch shape that
 * needs none; a captured launch owns its scratch for good.
 * What the CALLER of a captured launch must ensure: the same captured node must not run twice at the same time.  That means
 * (a) do not launch one executable graph again -- on any stream -- while an earlier launch of it may still be running (CUDA
 * orders such launches itself; HIP does not document that it does, so this library does not rely on it), and (b) do not
 * launch two executable graphs instantiated from the same capture concurrently.  Both replay the same node, scratch
 * included: the tickets of the two runs would interleave and bytes would come out wrong WITHOUT an error.  Capture again
 * for every concurrent user.
 * Captured large launches draw their scratch from a grow-only pool of 1 024 lines per device that is never handed out
 * again (a graph may be replayed at any time).  A process that keeps re-capturing exhausts it; captures beyond that -- and a
 * capture that is the device's very first large launch -- take the static streaming shape, which needs no scratch and is
 * correct but ~7 % slower at 4 GiB.  modgpu_queue_stats (modgpu_testing.h) counts both. */
int modgpu_cycle_device(void *dev_buf, uint64_t n, int32_t key, uint64_t stream_off,
                        int device, void *hip_stream);

/* n_parts device-resident buffers of ONE device, each its own Cycle call under one key -- its own keystream, from
 * stream_offs[i], or from 0 when stream_offs is NULL: what a caller does with the parts of an archive (the reference
 * treats them as independent files, CArk.cpp:741-755, 849-897).  Asynchronous on hip_stream like
 * modgpu_cycle_device; buffers may have any alignment and any size (empty ones are skipped); they must not overlap.
 * Runs of up to 16 parts share ONE kernel launch when together they are beyond 256 MiB, or no more than 24 MiB each on
 * average: the fixed cost of a launch (~7 us: pipeline fill, the finishing spread, the gap to the next launch) is 5 % of
 * a 411 MB part and most of the time of a small one (measured: +5 % at 8 x 411 MB, +30 % at 16 x 50 MB, 3x at 16 x 1 MiB). */
int modgpu_cycle_batch_device(void *const *dev_parts, const uint64_t *sizes, const uint64_t *stream_offs, int n_parts,
                              int32_t key, int device, void *hip_stream);

/* OUT OF PLACE: dev_dst[j] = dev_src[j] ^ ks[stream_off + j], j = 0 .. n-1, in one pass (src read once, dst written once);
 * dev_src is not modified.  Same keystream, 64-bit offsets and key reduction as modgpu_cycle_device, and the same contract:
 * asynchronous on `hip_stream`, `device` -1 = the current device (an explicit device leaves the thread's current device as it
 * was), allocation-free, capturable into a hipGraph; the concurrency and graph-scratch rules are the ones documented at
 * modgpu_cycle_device (a launch that finds no scratch -- every eager line busy, or a capture with the pool used up -- copies
 * with hipMemcpyAsync and cycles in place on the same stream: correct and capturable, two passes over HBM instead of one).  Edge cases:
 *   - src and dst may each have any byte alignment; their phases mod 16 are independent;
 *   - dst == src (exact alias) is allowed and gives what modgpu_cycle_device gives;
 *   - [dst, dst+n) partly overlapping [src, src+n) is MODGPU_ERR_INVALID, returned before anything is queued;
 *   - keys == 0 mod 2^31-1 (identity keystream) COPY: dst == src afterwards (hipMemcpyAsync on the stream);
 *   - n == 0 does nothing; a NULL pointer with n > 0 is MODGPU_ERR_INVALID;
 *   - either side may be page-locked host memory (modgpu_host_alloc): the kernel reaches it across PCIe -- supported, not tuned.
 * A kernel entry point like the rest: no host loop; MODGPU_ERR_NO_DEVICE / MODGPU_ERR_HIP as usual; path_stats().gpu_launches
 * counts its launches. */
int modgpu_cycle_device_to(void *dev_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off,
                           int device, void *hip_stream);

/* n_parts entries of ONE device, each its own out-of-place Cycle call under one key: dst_parts[i][j] = src_parts[i][j] ^
 * ks[stream_offs[i] + j] (stream_offs NULL = 0 for every entry).  What extracting the files of a resident archive part is:
 * src = part + o_i, dst = the file's own buffer, stream_off = o_i.  Everything modgpu_cycle_device_to says holds per entry;
 * in addition SOURCE ranges may overlap each other (they are only read), but a destination range that meets any other
 * entry's source or destination range makes the whole call MODGPU_ERR_INVALID (an entry's exact self-alias is allowed).
 * Any n_parts: up to 16 non-empty entries share one launch, more take more launches, in order, on the same stream; empty
 * entries are skipped.  For more than a handful of entries -- an archive's files -- modgpu_cycle_table_device takes a table of any
 * length in three launches, each entry with its own key. */
int modgpu_cycle_batch_device_to(void *const *dst_parts, const void *const *src_parts, const uint64_t *sizes,
                                 const uint64_t *stream_offs, int n_parts, int32_t key, int device, void *hip_stream);

/* REKEY: dev_dst[j] = dev_src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j], j = 0 .. n-1, in ONE pass: ciphertext under
 * one keystream becomes ciphertext under another without the plaintext ever reaching memory (it exists only in registers).  What
 * converting an encrypted part between platforms is (key_from = MODGPU_KEY_PS3, key_to = MODGPU_KEY_PS4, both offsets 0), and what
 * moving an encrypted file to another place in a part is (one key, off_from = the file's old stream offset, off_to = its new one).
 * The contract is modgpu_cycle_device_to's, word for word where it applies: asynchronous on `hip_stream`, `device` -1 = the current
 * device, allocation-free, capturable into a hipGraph under the same concurrency and graph-scratch rules; either side any byte
 * alignment, the two offsets any values (their phases mod 16 independent of each other and of the pointers'); dst == src (exact alias)
 * rekeys in place; a partial overlap is MODGPU_ERR_INVALID before anything is queued; n == 0 does nothing; a NULL pointer with n > 0
 * is MODGPU_ERR_INVALID; a page-locked host buffer on either side is supported, not tuned; no host loop.
 * Degenerate keystreams take the out-of-place call: key_from == 0 mod 2^31-1 is modgpu_cycle_device_to with key_to at off_to;
 * key_to == 0 is modgpu_cycle_device_to with key_from at off_from; both zero, or the same reduced key at the same stream position
 * (offsets equal mod 2^31-2), copy.  A launch that finds no scratch runs two passes on the same stream: out of place under
 * key_from, then in place under key_to (correct and capturable; modgpu_last_launch then reports the in-place launch).
 * A destination that partly overlaps its source is what modgpu_rekey_move_device takes. */
int modgpu_rekey_device_to(void *dev_dst, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to,
                           uint64_t off_to, int device, void *hip_stream);

/* ---- MOVE and rekey: the same bytes for ANY overlap of [dev_dst, dev_dst+n) with [dev_src, dev_src+n), in ONE pass ------------------
 * memmove rules: dev_dst[j] = SRC0[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j], where SRC0 is the source as it was when
 * the call started on the device -- every source byte is read before it is overwritten, in either direction.  Nothing outside
 * [dev_dst, dev_dst+n) is written; source bytes outside the destination range keep their values.  What closing the gap behind a
 * removed file of a resident part is (every later byte slides down by d: dev_dst = dev_src - d, one key, off_to = off_from - d), and
 * what opening one is; with equal keys and offsets, or two keys == 0 mod 2^31-1, it is the library's memmove.
 * The contract is otherwise modgpu_rekey_device_to's, word for word: asynchronous on `hip_stream`, `device` -1 = the current device,
 * allocation-free, capturable into a hipGraph; either side any byte alignment, the two offsets any 64-bit values (their phases mod 16
 * independent of each other and of the pointers'); n == 0 does nothing; a NULL pointer with n > 0 is MODGPU_ERR_INVALID; an entry
 * of 2^24 chunks of 64 KiB or more is MODGPU_ERR_INVALID; no host loop.  Page-locked host memory on either side is refused
 * (MODGPU_ERR_INVALID): the ordering below is for device memory.
 * The WORKSPACE is the caller's: device memory of `device`, 8-byte aligned, at least modgpu_move_workspace_bytes(n) bytes, checked on
 * the host before anything is queued, as the table calls check theirs.  It holds a header line (a status word and a ticket pair of the
 * call's own: the call never depends on the library's scratch and never degrades for lack of it), one 32-bit "loaded" flag per 64 KiB
 * chunk, and scratch for the ragged pieces.  The call resets it in stream order (hipMemsetAsync), so a replayed graph starts clean.
 * Two calls on one workspace must not overlap in time; a workspace that meets [dev_dst, dev_dst+n) or [dev_src, dev_src+n) is
 * MODGPU_ERR_INVALID.
 * Routes, chosen on the host:
 *   * disjoint ranges, or dev_dst == dev_src: modgpu_rekey_device_to, unchanged (the workspace is still checked, and its header
 *     reset);
 *   * a partial overlap: the bytes before the destination's first 64 KiB boundary and the last < 16 are rekeyed INTO the workspace by
 *     one ordinary rekey launch, the body in between is moved by the rekey kernel's move loop -- chunks in the direction of the move,
 *     each stored only once every chunk whose source it overwrites has been loaded --, and two copies put the pieces in place: 2
 *     kernel launches (path_stats().gpu_launches), 1 when the body is empty (n < 64 KiB or so) or there are no pieces;
 *     modgpu_last_launch reports the body launch as variant 14 with `bytes` = n;
 *   * keystreams that cancel (the same reduced key at the same stream position) or are both the identity: the same, bit-exact;
 *   * exactly ONE key == 0 mod 2^31-1 with a partial overlap: TWO passes on the same stream, the plain move, then the other key
 *     applied in place on dev_dst (path_stats().gpu_launches gains the in-place pass's launches too, and modgpu_last_launch
 *     then reports the in-place launch, not variant 14).
 * No wait inside the pass is unbounded: a workgroup that has waited 2 s for another one gives up, stores nothing more, and the call
 * ends; modgpu_move_status then returns MODGPU_ERR_HIP and the contents of [dev_dst, dev_dst+n) are unspecified.  That is a bug in
 * the library or a device in trouble, never a property of the arguments. */
uint64_t modgpu_move_workspace_bytes(uint64_t n); /* 0 for n == 0 or an entry of 2^24 chunks or more */
int modgpu_rekey_move_device(void *dev_dst, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from, int32_t key_to,
                             uint64_t off_to, void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);
/* Status of the last modgpu_rekey_move_device that ran on dev_workspace, read after the caller has synchronised: MODGPU_OK with
 * *stalled_chunk = UINT64_MAX, or MODGPU_ERR_HIP with *stalled_chunk = the 64 KiB chunk of the body whose wait ran out.
 * Synchronous, like modgpu_table_status (a small copy from the device). */
int modgpu_move_status(const void *dev_workspace, int device, uint64_t *stalled_chunk);

/* n_parts rekey entries of ONE device: dst_parts[i][j] = src_parts[i][j] ^ ks(key_from)[offs_from[i] + j] ^ ks(key_to)[offs_to[i] + j]
 * (a NULL offs_from or offs_to means 0 for every entry).  Relocating the files of an encrypted part is this call with
 * src = old part + o_old_i, dst = new part + o_new_i, offs_from = o_old, offs_to = o_new.  Everything modgpu_rekey_device_to says holds
 * per entry; as in modgpu_cycle_batch_device_to SOURCE ranges may overlap each other, a destination that meets any other entry's
 * source or destination makes the whole call MODGPU_ERR_INVALID, any n_parts is taken with up to 16 non-empty entries per launch, in
 * order, on the same stream, and empty entries are skipped.  For more than a handful of entries -- the files of a part --
 * modgpu_rekey_table_device takes a table of any length in three launches, each entry with its own pair of keys. */
int modgpu_rekey_batch_device_to(void *const *dst_parts, const void *const *src_parts, const uint64_t *sizes,
                                 const uint64_t *offs_from, const uint64_t *offs_to, int n_parts, int32_t key_from,
                                 int32_t key_to, int device, void *hip_stream);

/* ---- a TABLE of out-of-place entries in device memory: any length, three launches -----------------------------------------------
 * One entry: dst[j] = src[j] ^ ks(key)[stream_off + j], j = 0 .. n-1 -- exactly what modgpu_cycle_device_to computes for it (any byte
 * alignment on either side, dst == src cycles in place, n == 0 is skipped, a key == 0 mod 2^31-1 copies, 64-bit offsets).  What
 * extracting the files of a resident archive part is, each file with its own key if need be.  The layout is pinned (40 bytes). */
typedef struct modgpu_table_entry {
    void *dst;
    const void *src;
    uint64_t n;
    uint64_t stream_off;
    int32_t key;
    uint32_t flags; /* must be 0 (reserved) */
} modgpu_table_entry_t;

#define MODGPU_TABLE_MAX_ENTRIES 4194304u /* 2^22 entries per call */

/* Bytes of device workspace a call over n_entries needs: about 68 per entry plus a few lines (0 above MODGPU_TABLE_MAX_ENTRIES). */
uint64_t modgpu_table_workspace_bytes(uint64_t n_entries);

/* Cycles the n_entries entries at dev_entries, a table in device memory of `device`, in THREE kernel launches whatever n_entries is
 * (plan, finish, stream; path_stats().gpu_launches counts them, modgpu_last_launch reports the stream launch as variant 8).
 * Asynchronous on `hip_stream`; `device` -1 = the current device; allocation-free; capturable into a hipGraph.  THE TABLE IS READ
 * WHEN THE CALL RUNS ON THE DEVICE, not when it is queued: a captured call picks up whatever the caller wrote into the table (keys,
 * offsets, pointers, sizes) before each replay.
 * The WORKSPACE is the caller's: at least modgpu_table_workspace_bytes(n_entries) bytes of device memory of `device`, 8-byte aligned.
 * It holds all the call schedules with (its ticket counter, its plan, its status): the call shares nothing with other calls, so calls
 * with different workspaces may run at the same time on any streams, while two calls on ONE workspace must not overlap in time (a
 * captured call owns its workspace for as long as the graph may be replayed).  The call's first kernel resets the workspace in stream
 * order; nothing needs clearing beforehand.
 * Checks, in three tiers:
 *   1. on the host, before anything is queued -- MODGPU_ERR_INVALID: a NULL table or workspace with n_entries > 0, a table or
 *      workspace that is not 8-byte aligned, a workspace smaller than required, n_entries above MODGPU_TABLE_MAX_ENTRIES, a table or
 *      workspace that is not device memory of `device`.  n_entries == 0 queues nothing (and leaves the workspace's status as it was).
 *   2. on the device, by the plan: an entry with a NULL dst or src and n > 0, an entry with nonzero flags, an entry of 1 TiB or more,
 *      or entries of more than 2^31 chunks of 64 KiB together.  Any of these makes the WHOLE CALL WRITE NOTHING; modgpu_table_status
 *      names the lowest such entry once the caller has synchronised.
 *   3. not checked on the device: overlaps.  The rule is modgpu_cycle_batch_device_to's -- sources may overlap each other, an entry may
 *      alias itself exactly, a destination may meet no other entry's source or destination range.  Bytes in ranges that break it are
 *      unspecified, but nothing outside the entries' [dst, dst+n) is ever written.  modgpu_table_validate checks a host copy. */
int modgpu_cycle_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, void *dev_workspace,
                              uint64_t workspace_bytes, int device, void *hip_stream);

/* Status of the last call that ran on dev_workspace (read after the caller has synchronised; a modgpu_rekey_table_device workspace too,
 * and a modgpu_verify_table_device or modgpu_verify_rekey_table_device one, read unchanged: the header comes first in all of them): MODGPU_OK with *first_bad_entry =
 * UINT64_MAX if it ran clean, MODGPU_ERR_INVALID with *first_bad_entry = the lowest entry the device refused (the call wrote
 * nothing).  Synchronous (a small copy from the device). */
int modgpu_table_status(const void *dev_workspace, int device, uint64_t *first_bad_entry);

/* A host copy of a table against tiers 1-3 above, in O(n log n): MODGPU_OK, or MODGPU_ERR_INVALID with modgpu_last_error() naming
 * an entry at fault (a NULL pointer with n > 0, nonzero flags, a destination partly overlapping its own source, a destination
 * meeting another entry's source or destination).  No device is touched. */
int modgpu_table_validate(const modgpu_table_entry_t *host_entries, uint64_t n_entries);

/* ---- a TABLE of rekey entries in device memory: any length, three launches -------------------------------------------------------
 * One entry: dst[j] = src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j], j = 0 .. n-1 -- exactly what
 * modgpu_rekey_device_to computes for it (any byte alignment on either side, each offset with its own phase, dst == src rekeys in
 * place, n == 0 is skipped, 64-bit offsets; a key == 0 mod 2^31-1 is the identity keystream, so one such key applies or removes only
 * the other, two copy, and the same reduced key at offsets equal mod 2^31-2 copies).  What relocating the files of an encrypted part
 * is (src = old part + o_old, dst = new part + o_new, off_from = o_old, off_to = o_new), converting them between platforms in the
 * same step if the keys differ.  The plaintext never reaches memory.  The layout is pinned (56 bytes, 8-byte aligned). */
typedef struct modgpu_rekey_table_entry {
    void *dst;
    const void *src;
    uint64_t n;
    uint64_t off_from; /* stream offset of src[0] under key_from */
    uint64_t off_to;   /* stream offset of dst[0] under key_to */
    int32_t key_from;
    int32_t key_to;
    uint32_t flags;    /* must be 0 (reserved) */
    uint32_t reserved; /* must be 0 */
} modgpu_rekey_table_entry_t;

/* Bytes of device workspace a rekey table call over n_entries needs: about 84 per entry plus a few lines (0 above
 * MODGPU_TABLE_MAX_ENTRIES). */
uint64_t modgpu_rekey_table_workspace_bytes(uint64_t n_entries);

/* Rekeys the n_entries entries at dev_entries, a table in device memory of `device`, in THREE kernel launches whatever n_entries is
 * (plan, finish, stream; path_stats().gpu_launches counts them, modgpu_last_launch reports the stream launch as variant 9).  The
 * contract is modgpu_cycle_table_device's, word for word where it applies: asynchronous on `hip_stream`, `device` -1 = the current
 * device, allocation-free, capturable into a hipGraph; THE TABLE IS READ WHEN THE CALL RUNS ON THE DEVICE, so a replayed graph picks
 * up entries rewritten between replays; up to MODGPU_TABLE_MAX_ENTRIES entries; the WORKSPACE is the caller's (at least
 * modgpu_rekey_table_workspace_bytes(n_entries) bytes of device memory of `device`, 8-byte aligned, reset by the call's first kernel
 * in stream order), and two calls on one workspace must not overlap in time.
 * Checks, in three tiers:
 *   1. on the host, before anything is queued -- MODGPU_ERR_INVALID: the table call's tier 1, with this call's workspace size.
 *   2. on the device, by the plan: an entry with a NULL dst or src and n > 0, an entry with nonzero flags or reserved, an entry of
 *      1 TiB or more, or entries of more than 2^31 chunks of 64 KiB together.  Any of these makes the WHOLE CALL WRITE NOTHING.
 *   3. not checked on the device: overlaps, under modgpu_rekey_batch_device_to's rule (sources may overlap each other, an entry may
 *      alias itself exactly, a destination may meet no other entry's source or destination range).  Bytes in ranges that break it
 *      are unspecified, but nothing outside the entries' [dst, dst+n) is ever written.  modgpu_rekey_table_validate checks a host copy.
 * The workspace starts with the table call's header, so modgpu_table_status reports this call too: once the caller has
 * synchronised it names the lowest entry the device refused, whichever kind of table call ran last on the workspace. */
int modgpu_rekey_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, void *dev_workspace,
                              uint64_t workspace_bytes, int device, void *hip_stream);

/* A host copy of a rekey table against tiers 1-3 above, in O(n log n): MODGPU_OK, or MODGPU_ERR_INVALID with modgpu_last_error()
 * naming an entry at fault (a NULL pointer with n > 0, nonzero flags or reserved, a destination partly overlapping its own source,
 * a destination meeting another entry's source or destination).  No device is touched. */
int modgpu_rekey_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries);

/* ---- a TABLE of rekey entries MOVED with memmove rules: compacting a resident part in one pass, five launches --------------------
 * For every entry i of a modgpu_rekey_table_entry_t table in device memory, used as it stands (56 bytes, flags and reserved 0):
 *     dst_i[j] = SRC0_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j],   j = 0 .. n_i-1
 * where SRC0 is device memory as it was when the call started on the device: every source byte of every entry is read before any
 * entry overwrites it, and nothing outside the entries' [dst, dst+n) is written.  A destination may meet ANY entry's source, its own
 * or another's: removing or resizing k files of a resident part leaves k surviving segments, each sliding by its own distance onto
 * the previous one's source, and this call moves them all in one pass over HBM.  Per entry everything modgpu_rekey_table_device says
 * holds: any byte alignment on either side, each offset with its own phase, 64-bit offsets, n == 0 is skipped, a key == 0 mod 2^31-1
 * is the identity keystream, the same reduced key at offsets equal mod 2^31-2 copies -- every degenerate key pair in the same single
 * pass (modgpu_rekey_move_device takes two passes when exactly one key is the identity).
 * WHICH TABLES ARE TAKEN.  After dropping empty entries the table must be DOWNWARD -- for every i: dst_i <= src_i,
 * src_i + n_i <= src_{i+1}, dst_i + n_i <= dst_{i+1} -- or UPWARD: the same listing order and the same two disjointness conditions
 * with dst_i >= src_i.  So the entries are listed by rising address, sources are pairwise disjoint, destinations are pairwise
 * disjoint, all entries slide the same way (dst == src is allowed in either kind; the first entry with dst != src says which kind
 * the table is).  DESIGN.md 4.15 has the argument why one pass then suffices.
 * total_bytes is the caller's upper bound on the sum of the n_i: the table is read when the call runs on the device, so the host
 * cannot know the chunk count; the workspace is sized for total_bytes / 64 KiB + 2 * n_entries chunks (a 32-bit "loaded" flag and an
 * 8-byte window per chunk) and 32 bytes of scratch per entry for the ragged ends (the < 16 bytes before and after each body).
 * modgpu_rekey_move_table_workspace_bytes returns 0 for no entries, for more than MODGPU_TABLE_MAX_ENTRIES, and for a total_bytes
 * whose chunks pass 2^31.
 * The contract is modgpu_rekey_table_device's, word for word where it applies: asynchronous on `hip_stream`, `device` -1 = the current
 * device, allocation-free, capturable into a hipGraph; THE TABLE IS READ WHEN THE CALL RUNS ON THE DEVICE, so a replayed graph picks
 * up entries rewritten between replays and starts from a clean workspace, which the first launch resets in stream order; the
 * WORKSPACE is the caller's, device memory of `device`, 8-byte aligned; two calls on one workspace must not overlap in time.  The
 * call draws its tickets from the workspace: it never touches the library's ring and has no degraded route.  FIVE kernel launches
 * whatever n_entries is (plan, finish, window, move, place; path_stats().gpu_launches counts them), no memset and no copy;
 * modgpu_last_launch reports the move launch as variant 15 (`bytes` = 0, as for 8).  Page-locked host memory anywhere in a table
 * is not supported: the ordering inside the pass is for device memory.
 * Checks, in three tiers:
 *   1. on the host, before anything is queued -- MODGPU_ERR_INVALID: the table call's tier 1, with this call's workspace size.
 *   2. on the device, by the plan: an entry with a NULL dst or src and n > 0, nonzero flags or reserved, an entry of 1 TiB or more,
 *      more chunks than the workspace was sized for, or AN ENTRY THAT BREAKS THE DIRECTION AND ORDER RULE above (each non-empty
 *      entry is compared with the non-empty entry before it).  Any of these makes the WHOLE CALL WRITE NOTHING, and the status names
 *      the lowest such entry.
 *   3. modgpu_rekey_move_table_validate checks a host copy against tiers 1 and 2 in O(n) and names an entry at fault in
 *      modgpu_last_error().  No device is touched.
 * No wait inside the pass is unbounded: a workgroup that has waited 2 s for another one gives up, records the chunk, stores nothing
 * more, and the call ends.  That is a bug in the library or a device in trouble, never a property of the arguments.
 * The workspace starts with the table call's header, so modgpu_table_status reads it unchanged.  modgpu_rekey_move_table_status
 * (synchronous, read after the caller has synchronised) reports one thing more: MODGPU_OK with both outputs UINT64_MAX;
 * MODGPU_ERR_INVALID with *first_bad_entry = the lowest entry the device refused (the call wrote nothing); MODGPU_ERR_HIP with
 * *stalled_chunk = the global 64 KiB chunk whose wait ran out (the contents of the destinations are then unspecified). */
uint64_t modgpu_rekey_move_table_workspace_bytes(uint64_t n_entries, uint64_t total_bytes);
int modgpu_rekey_move_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, uint64_t total_bytes,
                                   void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);
int modgpu_rekey_move_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries);
int modgpu_rekey_move_table_status(const void *dev_workspace, int device, uint64_t *first_bad_entry, uint64_t *stalled_chunk);

/* ---- a table of rekey entries RELAID OUT: segments that slide BOTH ways, a splice of a resident part in one pass, ten launches ------
 * Putting changed files into a resident part is a splice: some files grow, some shrink, some go away, and every surviving segment
 * slides by the running sum of the size changes before it -- some up and some down in the same table, which the move table call above
 * refuses.  This call takes such a table.  Its semantics are the move table call's, word for word, with these differences:
 *   SAME WHERE IT APPLIES: dst_i[j] = SRC0_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j] with SRC0 device memory
 *   as the call found it; every degenerate key pair in the pass; asynchronous on `hip_stream`; allocation-free; capturable into a
 *   hipGraph; the table read when the call runs on the device, so a replayed graph picks up rewritten entries; tier 1 on the host
 *   before anything is queued; page-locked host memory anywhere in a table is not supported.
 *   THE RULE.  After dropping empty entries: src_i + n_i <= src_{i+1} and dst_i + n_i <= dst_{i+1} -- the entries are listed by rising
 *   address, sources pairwise disjoint, destinations pairwise disjoint.  Each non-empty entry is checked against the non-empty entry
 *   before it, whatever the direction of either: there is no direction clause.  (Under that rule an entry with dst <= src and one with
 *   dst > src never meet, destination on source, so the table is two one-way tables interleaved: DESIGN.md 4.20.)
 *   LAUNCHES.  Exactly TEN kernel launches whatever n_entries is and whatever the mix: two sweeps of plan, finish, window, move, place
 *   on the one stream, sweep 0 over the entries with dst <= src, sweep 1 over those with dst > src.  No memset and no copy; each byte
 *   of each entry is read once and written once.  modgpu_last_launch reports the second move launch, as variant 15.
 *   ALL OR NOTHING.  Anything the device refuses makes the WHOLE CALL write nothing, in either sweep: a NULL dst or src with n > 0,
 *   nonzero flags or reserved, an entry of 1 TiB or more, the rule above, or more chunks than the workspace was sized for -- counted
 *   over ALL entries, not per sweep.  Both sweeps decide on the same quantities and reach the same verdict; the table must not
 *   change between them, so, as above, it must not lie in memory the call writes.
 *   WORKSPACE AND STATUS are the move table call's: modgpu_rekey_move_table_workspace_bytes(n_entries, total_bytes) and
 *   modgpu_rekey_move_table_status; sweep 1 reuses the workspace in stream order.  A wait that runs out in sweep 0 stays in the status,
 *   and sweep 1 then stores nothing.  *stalled_chunk is a chunk number in the numbering of the sweep that stalled (each sweep numbers
 *   the chunks of its own entries from 0): diagnostic only.
 * modgpu_rekey_relayout_table_validate checks a host copy against tier 1 and the rule above in O(n) and names the entry at fault in
 * modgpu_last_error().  No device is touched.  (A table the move table call takes is taken here too, at the price of the idle sweep's
 * five small launches.) */
int modgpu_rekey_relayout_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, uint64_t total_bytes,
                                       void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);
int modgpu_rekey_relayout_table_validate(const modgpu_rekey_table_entry_t *host_entries, uint64_t n_entries);

/* ---- VERIFY: is this buffer what the cipher would have produced from that one?  One read-only pass, two numbers -------------------
 * The result of one entry, in device memory.  The layout is pinned (32 bytes, 8-byte aligned). */
typedef struct modgpu_verify_result {
    uint64_t mismatches;     /* number of j in [0, n) with expect[j] != (src[j] ^ ks(key)[stream_off + j]) -- BYTES, not words */
    uint64_t first_mismatch; /* the lowest such j, counted from the entry's own first byte; UINT64_MAX if there is none */
    uint64_t n;              /* bytes compared = the entry's n (lets a reader tell "ran clean" from "never ran") */
    uint64_t reserved;       /* 0 */
} modgpu_verify_result_t;

/* Compares dev_expect[j] with dev_src[j] ^ ks(key)[stream_off + j] for j = 0 .. n-1 -- the bytes modgpu_cycle_device_to would have
 * written -- where the data lies, in one pass that READS 2n bytes and writes the 32 bytes of *dev_result.  Same keystream, 64-bit
 * offsets and key reduction as modgpu_cycle_device.  The contract is modgpu_cycle_device_to's, word for word where it applies:
 * asynchronous on `hip_stream`; `device` -1 = the current device, an explicit device leaves the thread's current device as it was;
 * allocation-free; capturable into a hipGraph; any number of calls may be in flight on any streams as long as their RESULT ranges
 * differ.  Kernel entry point: no host loop, MODGPU_ERR_NO_DEVICE / MODGPU_ERR_HIP as usual.
 *   * NOTHING BUT THE RESULT IS WRITTEN.  `expect` and `src` are read-only, so there is no overlap rule at all: they may be the same
 *     pointer or overlap partly (and in the batch any entry may overlap any other).  Either may be page-locked host memory
 *     (supported, not tuned).  Each may have any byte alignment; their phases mod 16 are independent.
 *   * The result lives in device memory of `device`, 8-byte aligned, the caller's.  A result pointer that the runtime does not report
 *     as device memory of the call's device (both ends of the range are asked about, as the transfer calls do), or that is misaligned,
 *     is MODGPU_ERR_INVALID before anything is queued; so is a NULL expect or src with n > 0, a NULL result, and an entry that spans
 *     2^24 chunks of 64 KiB or more (1 TiB; the table calls' limit).
 *   * THE CALL INITIALISES ITS RESULT ITSELF, IN STREAM ORDER, with a small kernel in front of the compare.  Nothing needs clearing
 *     beforehand, and a replayed graph starts from a clean result on every replay.  Once the call has completed on its stream the
 *     fields are as documented above.
 *   * n == 0 still produces a result: {0, UINT64_MAX, 0, 0}.
 *   * key == 0 mod 2^31-1 (the identity keystream) is a plain device memcmp with a count: same result fields.
 *   * The call never fails or degrades for lack of scheduling scratch: its chunks are assigned to workgroups statically, it draws no
 *     ticket line (modgpu_cycle_device_to does, and copies + cycles in place when none is free; a read-only call has nothing to fall
 *     back to, and measured against that call it does not need the ticket queue: DESIGN.md 4.10).
 *   * Launches (path_stats().gpu_launches counts them): ONE to initialise the results of the call, then ONE per started group of 16
 *     non-empty entries -- 2 for this call with n > 0, 1 with n == 0.  modgpu_last_launch reports the compare launch as variant 10
 *     (the initialising launch alone, `bytes` = 0, if the call had no non-empty entry). */
int modgpu_verify_device(const void *dev_expect, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off,
                         modgpu_verify_result_t *dev_result, int device, void *hip_stream);

/* n_parts entries of ONE device, dev_results[i] the result of entry i: everything modgpu_verify_device says holds per entry.
 * stream_offs NULL = 0 for every entry.  Any n_parts is taken: one launch initialises all n_parts results (empty entries get
 * {0, UINT64_MAX, 0, 0}), then up to 16 non-empty entries share a compare launch and further launches follow in order on the same
 * stream -- 1 + ceil(non_empty / 16) launches.  A negative n_parts, or NULL arrays or a NULL dev_results with n_parts > 0, is
 * MODGPU_ERR_INVALID; n_parts == 0 queues nothing. */
int modgpu_verify_batch_device(const void *const *expect_parts, const void *const *src_parts, const uint64_t *sizes,
                               const uint64_t *stream_offs, int n_parts, int32_t key, modgpu_verify_result_t *dev_results,
                               int device, void *hip_stream);

/* `count` results from device memory of `device` into host_out.  Synchronous (a small copy from the device, like
 * modgpu_table_status): call it after the caller has synchronised the stream the verify calls ran on. */
int modgpu_verify_results(const modgpu_verify_result_t *dev_results, uint64_t count, int device, modgpu_verify_result_t *host_out);

/* ---- DIGEST: what does the cipher make of this buffer?  One pass that reads n bytes and writes 32 ------------------------------------
 * Adler-32 (as zlib computes it) of out[j] = src[j] ^ ks(key)[stream_off + j], j = 0 .. n-1 -- the bytes modgpu_cycle_device_to would
 * write -- with or without storing them.  The device keeps two order-free integer sums, so the value is exact and the same for every
 * launch shape:   S1 = sum of out[j]      S2 = sum of j * out[j]      (both mod 65521)
 * and the host finalises them (modgpu_digest_adler32):   A = (1 + S1) mod 65521,  B = (n + n * S1 - S2) mod 65521,  B << 16 | A.
 * The record of one entry, in device memory.  The layout is pinned (32 bytes, 8-byte aligned). */
typedef struct modgpu_digest_result {
    uint64_t s1, s2;   /* only their residues mod 65521 are specified */
    uint64_t n;        /* the entry's n (lets a reader tell "ran" from "never ran"; it enters B) */
    uint64_t reserved; /* 0 */
} modgpu_digest_result_t;

/* dev_dst NULL: DIGEST ONLY -- reads the n bytes of dev_src, writes nothing but *dev_result.  dev_dst given: FUSED -- dev_dst[j] = out[j]
 * is stored exactly as modgpu_cycle_device_to stores it (byte for byte the same destination) and the same registers are summed.  Same
 * keystream, 64-bit offsets and key reduction as modgpu_cycle_device.  The contract is modgpu_cycle_device_to's where it applies:
 * asynchronous on `hip_stream`; `device` -1 = the current device, an explicit device leaves the thread's current device as it was;
 * allocation-free; capturable into a hipGraph; any byte alignment of either buffer; the source may be page-locked host memory
 * (supported, not tuned).
 *   * With a destination the out-of-place overlap rules hold: dst == src exactly is allowed, a partial overlap of dst and src (and, in
 *     the batch, a destination that meets another entry's source or destination) is MODGPU_ERR_INVALID before anything is queued.  So
 *     is a NULL src with n > 0, a NULL or misaligned result, a result that the runtime does not report as device memory of the call's
 *     device, and an entry that spans 2^24 chunks of 64 KiB or more (1 TiB).  Entries without a destination are only read and may
 *     overlap anything that is not written.
 *   * THE CALL ZEROES ITS RECORD ITSELF, IN STREAM ORDER (hipMemsetAsync on `hip_stream`): nothing needs clearing beforehand, and the
 *     memset is a node of a capture, so a replayed graph starts from a clean record on every replay.
 *   * n == 0 yields {0, 0, 0, 0} -- Adler-32 = 1 -- and no kernel launch.
 *   * key == 0 mod 2^31-1 (the identity keystream): out = src, the plain Adler-32 of the buffer (fused: a copy with a checksum).
 *   * The call never fails or degrades for lack of scheduling scratch: chunks are assigned to workgroups statically, no ticket line is
 *     drawn.
 *   * Launches (path_stats().gpu_launches counts them): ONE per started group of 16 non-empty entries.  modgpu_last_launch reports
 *     variant 16 with `bytes` = all entries of the launch. */
int modgpu_digest_device(void *dev_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off,
                         modgpu_digest_result_t *dev_result, int device, void *hip_stream);

/* n_parts entries of ONE device, dev_results[i] the record of entry i: everything modgpu_digest_device says holds per entry.
 * dst_parts NULL, or a NULL dst_parts[i]: that entry is digest only.  stream_offs NULL = 0 for every entry.  Any n_parts is taken: one
 * memset zeroes all n_parts records, then up to 16 non-empty entries share a launch and further launches follow in order on the same
 * stream.  A negative n_parts, or NULL src_parts / sizes / dev_results with n_parts > 0, is MODGPU_ERR_INVALID; n_parts == 0 queues
 * nothing. */
int modgpu_digest_batch_device(void *const *dst_parts, const void *const *src_parts, const uint64_t *sizes, const uint64_t *stream_offs,
                               int n_parts, int32_t key, modgpu_digest_result_t *dev_results, int device, void *hip_stream);

/* `count` records from device memory of `device` into host_out and, if adler32_out is not NULL, their Adler-32 values into
 * adler32_out[0 .. count).  Synchronous (a small copy from the device): call it after the caller has synchronised the stream. */
int modgpu_digest_results(const modgpu_digest_result_t *dev_results, uint64_t count, int device, modgpu_digest_result_t *host_out,
                          uint32_t *adler32_out);

/* Adler-32 from one record in HOST memory.  Pure arithmetic: no device, no error state (NULL gives 1, the Adler-32 of nothing). */
uint32_t modgpu_digest_adler32(const modgpu_digest_result_t *host_result);

/* ---- VERIFY REKEY: is this buffer what the rekey would have produced from that one?  The verify call against two keystreams ---------
 * Compares dev_expect[j] with dev_src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j] for j = 0 .. n-1 -- the bytes
 * modgpu_rekey_device_to would have written -- where the data lies, in one pass that READS 2n bytes and writes the 32 bytes of
 * *dev_result: mismatching BYTES, the lowest mismatching index counted from the entry's first byte, n, 0.  Without it a caller that
 * no longer has the plaintext has to rekey again into scratch memory as large as the data and compare that with the identity key.
 * The contract is modgpu_verify_device's, word for word where it applies: asynchronous on `hip_stream`; `device` -1 = the current
 * device, an explicit device leaves the thread's current device as it was; allocation-free; capturable into a hipGraph, a replay
 * starts from a clean result (the call initialises its result itself, in stream order); it draws no ticket line and cannot degrade
 * for lack of scratch; any alignment on either side, the two offsets' phases independent of each other and of the pointers'; no
 * overlap rule at all (nothing but the result is written); page-locked host memory on either input is supported, not tuned;
 * n == 0 gives {0, UINT64_MAX, 0, 0}.  MODGPU_ERR_INVALID before anything is queued: a NULL input with n > 0, a NULL, misaligned or
 * non-device result, an entry that spans 2^24 chunks of 64 KiB or more.  modgpu_verify_results reads the result back.
 *   * Degenerate keystreams follow modgpu_rekey_device_to's rules: a key == 0 mod 2^31-1 leaves only the other keystream (both: a
 *     plain compare), and the same reduced key at offsets equal mod 2^31-2 is a plain compare (ks ^ ks = 0).  Those entries run on
 *     modgpu_verify_device's kernels and are reported as variant 10; only entries whose two streams really differ reach the
 *     two-keystream kernel (variant 12).
 *   * Launches (path_stats().gpu_launches counts them): ONE to initialise the results of the call, then one per started group of 16
 *     non-empty entries -- 2 for this call with n > 0, 1 with n == 0. */
int modgpu_verify_rekey_device(const void *dev_expect, const void *dev_src, uint64_t n, int32_t key_from, uint64_t off_from,
                               int32_t key_to, uint64_t off_to, modgpu_verify_result_t *dev_result, int device, void *hip_stream);

/* n_parts entries of ONE device under one pair of keys, dev_results[i] the result of entry i: everything
 * modgpu_verify_rekey_device says holds per entry.  offs_from / offs_to NULL = 0 for every entry.  Any n_parts is taken: one launch
 * initialises all n_parts results, then one launch per started group of 16 non-empty entries whose two streams differ and one per
 * started group of 16 non-empty entries whose streams coincide (or of which a key is the identity), in that order on the same stream.
 * A negative n_parts, or NULL arrays or a NULL dev_results with n_parts > 0, is MODGPU_ERR_INVALID; n_parts == 0 queues nothing. */
int modgpu_verify_rekey_batch_device(const void *const *expect_parts, const void *const *src_parts, const uint64_t *sizes,
                                     const uint64_t *offs_from, const uint64_t *offs_to, int n_parts, int32_t key_from, int32_t key_to,
                                     modgpu_verify_result_t *dev_results, int device, void *hip_stream);

/* ---- VERIFY TABLE: the verify call over a device-resident table of any length, in three launches -------------------------------------
 * One entry is a modgpu_table_entry_t as it stands (40 bytes, flags 0) with `dst` read as the COMPARAND (`expect`; never written):
 * dev_results[i] receives exactly what modgpu_verify_device(dst, src, n, key, stream_off, ...) would have produced for entry i --
 * the same four fields, first_mismatch counted from the entry's own first byte; n == 0 gives {0, UINT64_MAX, 0, 0}; a key == 0 mod
 * 2^31-1 is a plain compare.  The bytes of workspace a call over n_entries needs (0 for none, or above MODGPU_TABLE_MAX_ENTRIES): */
uint64_t modgpu_verify_table_workspace_bytes(uint64_t n_entries);

/* The contract is modgpu_cycle_table_device's, word for word where it applies: THREE launches (plan, finish, stream) whatever the
 * count -- path_stats().gpu_launches counts 3, modgpu_last_launch reports the stream launch as variant 11 with `bytes` = 0 --;
 * asynchronous on `hip_stream`, allocation-free, capturable into a hipGraph; the table is read when the call RUNS on the device; the
 * workspace (modgpu_verify_table_workspace_bytes(n_entries) bytes of device memory of `device`, 8-byte aligned) is the caller's, reset
 * by the plan launch in stream order, and two calls on one workspace must not overlap in time.  The workspace starts with the table
 * call's header, so modgpu_table_status reports this call too.
 *   * EVERYTHING BUT THE RESULTS AND THE WORKSPACE IS READ-ONLY.  There is no overlap rule at all -- any entry's dst or src may
 *     overlap anything, itself included -- and no _validate function.
 *   * dev_results: n_entries results in device memory of `device`, 8-byte aligned, the caller's.  THE CALL INITIALISES THEM ITSELF:
 *     the finish launch stores every entry's result whole (what the < 16 ragged bytes at either end of the entry gave, and n), the
 *     stream launch then only adds to and lowers valid results.  Nothing needs clearing beforehand; a replayed graph starts clean.
 *   * Tier 1 (host, MODGPU_ERR_INVALID before anything is queued): modgpu_cycle_table_device's tier 1 with this call's workspace
 *     size; dev_results NULL with n_entries > 0, not 8-byte aligned, or not reported as device memory of `device` (both ends of the
 *     range are asked about, as modgpu_verify_device does).  n_entries == 0 queues nothing.
 *   * Tier 2 (device, by the plan launch): a NULL dst or src with n > 0, nonzero flags, an entry of 1 TiB or more, more than 2^31
 *     chunks of 64 KiB together.  Any of these makes the whole call write NO RESULT AT ALL -- dev_results stays as the caller left
 *     it --, modgpu_table_status names the lowest such entry and modgpu_verify_table_summary returns MODGPU_ERR_INVALID. */
int modgpu_verify_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, modgpu_verify_result_t *dev_results,
                               void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);

/* The whole call in 32 bytes, for the caller that asks "is the part intact, and if not, which file first" and does not want to
 * download n_entries results.  The layout is pinned. */
typedef struct modgpu_verify_table_summary {
    uint64_t mismatches;      /* sum of every entry's mismatches */
    uint64_t first_bad_entry; /* lowest entry index with at least one mismatch; UINT64_MAX if none */
    uint64_t entries;         /* n_entries of the call that ran */
    uint64_t reserved;        /* 0 */
} modgpu_verify_table_summary_t;
/* Synchronous (a small copy from the device, like modgpu_table_status): call it after the caller has synchronised the stream the
 * call ran on.  MODGPU_ERR_INVALID if the device refused the call (modgpu_table_status names the entry).  Reads the workspace of a
 * modgpu_verify_rekey_table_device call unchanged: its summary line sits in the same place. */
int modgpu_verify_table_summary(const void *dev_workspace, int device, modgpu_verify_table_summary_t *out);

/* ---- VERIFY REKEY TABLE: the rekey verify call over a device-resident table of any length, in three launches -------------------------
 * One entry is a modgpu_rekey_table_entry_t as it stands (56 bytes, flags and reserved 0) with `dst` read as the COMPARAND (never
 * written): dev_results[i] receives exactly what modgpu_verify_rekey_device(dst, src, n, key_from, off_from, key_to, off_to, ...) would
 * have produced for entry i -- the same four fields, first_mismatch counted from the entry's own first byte; n == 0 gives
 * {0, UINT64_MAX, 0, 0}.  So the table modgpu_rekey_table_device was given checks its own result, each entry under its own pair of
 * keys and offsets.  Degenerate keystreams follow modgpu_rekey_table_device's rules (a key == 0 mod 2^31-1 leaves only the other
 * keystream, two are a plain compare, the same reduced key at offsets equal mod 2^31-2 is a plain compare); every entry runs on the
 * same kernel.  The bytes of workspace a call over n_entries needs (0 for none, or above MODGPU_TABLE_MAX_ENTRIES): */
uint64_t modgpu_verify_rekey_table_workspace_bytes(uint64_t n_entries);

/* The contract is modgpu_verify_table_device's, word for word where it applies: THREE launches (plan, finish, stream) whatever the
 * count -- path_stats().gpu_launches counts 3, modgpu_last_launch reports the stream launch as variant 13 with `bytes` = 0 --;
 * asynchronous on `hip_stream`, allocation-free, capturable into a hipGraph; the table is read when the call RUNS on the device, so a
 * replay picks up rewritten entries and starts from clean results; the workspace (modgpu_verify_rekey_table_workspace_bytes(n_entries)
 * bytes of device memory of `device`, 8-byte aligned) is the caller's, reset by the plan launch in stream order, and two calls on one
 * workspace must not overlap in time.  The workspace starts with the table call's header and the verify table call's summary line, so
 * modgpu_table_status and modgpu_verify_table_summary report this call too.
 *   * EVERYTHING BUT THE RESULTS AND THE WORKSPACE IS READ-ONLY.  There is no overlap rule at all and no _validate function.
 *   * dev_results: n_entries results in device memory of `device`, 8-byte aligned, the caller's; the call initialises them itself (the
 *     finish launch stores every entry's result whole, the stream launch then only adds to and lowers valid results).
 *   * Tier 1 (host, MODGPU_ERR_INVALID before anything is queued): modgpu_verify_table_device's tier 1 with this call's entry size and
 *     workspace size.  n_entries == 0 queues nothing.
 *   * Tier 2 (device, by the plan launch): a NULL dst or src with n > 0, nonzero flags or reserved, an entry of 1 TiB or more, more
 *     than 2^31 chunks of 64 KiB together.  Any of these makes the whole call write NO RESULT AT ALL -- dev_results stays as the caller
 *     left it --, modgpu_table_status names the lowest such entry and modgpu_verify_table_summary returns MODGPU_ERR_INVALID. */
int modgpu_verify_rekey_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, modgpu_verify_result_t *dev_results,
                                     void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);

/* ---- DIGEST TABLE: the digest call over a device-resident table of any length, in three launches -------------------------------------
 * "Are the 100 000 files of this part the files I packed?" for the caller who holds a manifest of checksums and no comparand.  One
 * entry is a modgpu_table_entry_t as it stands (40 bytes, flags 0) whose `dst` IS IGNORED -- never read, never dereferenced, never
 * written; NULL or anything else --, so the same device-resident table goes unchanged to modgpu_cycle_table_device,
 * modgpu_verify_table_device and this call.  dev_results[i] receives the record of
 *     out[j] = src_i[j] ^ ks(key_i)[stream_off_i + j],  j = 0 .. n_i - 1
 * as modgpu_digest_device defines it: {s1, s2, n, 0}, only the residues mod 65521 of s1 and s2 specified, n the entry's n; read back
 * and closed with modgpu_digest_results / modgpu_digest_adler32.  An empty entry gives {0, 0, 0, 0} (Adler-32 = 1); a key == 0 mod
 * 2^31-1 gives the plain Adler-32 of the source.  Each entry has its own key and stream offset.  The bytes of workspace a call over
 * n_entries needs (0 for none, or above MODGPU_TABLE_MAX_ENTRIES) -- modgpu_table_workspace_bytes(n_entries), the same layout: */
uint64_t modgpu_digest_table_workspace_bytes(uint64_t n_entries);

/* The contract is modgpu_verify_table_device's, word for word where it applies: THREE launches (plan, finish, stream) whatever the
 * count -- path_stats().gpu_launches counts 3, modgpu_last_launch reports the stream launch as variant 17 with `bytes` = 0 --;
 * asynchronous on `hip_stream`, allocation-free, capturable into a hipGraph; the table is read when the call RUNS on the device, so a
 * replay picks up rewritten entries; the workspace (modgpu_digest_table_workspace_bytes(n_entries) bytes of device memory of `device`,
 * 8-byte aligned) is the caller's, reset by the plan launch in stream order, and two calls on one workspace must not overlap in time.
 * The workspace starts with the table call's header, so modgpu_table_status reports this call too (it has no summary line).
 *   * EVERYTHING BUT THE RECORDS AND THE WORKSPACE IS READ-ONLY.  There is no overlap rule at all -- sources may overlap anything, each
 *     other and the records' neighbours included -- and no _validate function.
 *   * dev_results: n_entries records in device memory of `device`, 8-byte aligned, the caller's.  THE CALL INITIALISES THEM ITSELF, AND
 *     WITHOUT A MEMSET NODE: the finish launch stores every entry's record whole (the sums of the < 16 ragged bytes at either end of
 *     the entry, and n), the stream launch then only adds to valid records (64-bit atomic adds).  Nothing needs clearing beforehand; a
 *     replayed graph starts clean.
 *   * Tier 1 (host, MODGPU_ERR_INVALID before anything is queued): modgpu_verify_table_device's tier 1 with this call's workspace
 *     size: a NULL table, workspace or dev_results with n_entries > 0; one of them not 8-byte aligned; a short workspace; memory not
 *     reported as device memory of `device`; more than MODGPU_TABLE_MAX_ENTRIES entries.  n_entries == 0 queues nothing.
 *   * Tier 2 (device, by the plan launch): a NULL src with n > 0, nonzero flags, an entry of 1 TiB or more, more than 2^31 chunks of
 *     64 KiB together.  Any of these makes the whole call write NO RECORD AT ALL -- dev_results stays as the caller left it -- and
 *     modgpu_table_status names the lowest such entry. */
int modgpu_digest_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, modgpu_digest_result_t *dev_results,
                               void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);

/* ---- CYCLE DIGEST TABLE: modgpu_cycle_table_device and one digest record per entry, in the same pass and the same three launches -------
 * "Decrypt the 100 000 files of this part and tell me that they are the files that were packed", or "encrypt them and give me one
 * plaintext checksum per file": the source is read once (2n bytes of traffic, where modgpu_cycle_table_device followed by
 * modgpu_digest_table_device moves 3n).  Per entry
 *   * `dst` receives, byte for byte, what modgpu_cycle_table_device writes for the same table -- and nothing next to it is touched;
 *   * dev_records[i] receives {s1, s2, n, 0} as modgpu_digest_device defines it (only the residues mod 65521 of s1 and s2 specified),
 *     of one side of the XOR: */
#define MODGPU_DIGEST_OUTPUT 0u /* records are of out[j] = src[j] ^ ks(key)[stream_off + j]: what is stored */
#define MODGPU_DIGEST_INPUT 1u  /* records are of src[j] as read: what the cipher was applied to */
/* The ciphertext's checksum depends on the stream offset, so a packer asks for MODGPU_DIGEST_INPUT (the plaintext it read), an
 * extractor for MODGPU_DIGEST_OUTPUT (the plaintext it wrote).  Records are read back and closed with modgpu_digest_results /
 * modgpu_digest_adler32.  An empty entry gives {0, 0, 0, 0}; a key == 0 mod 2^31-1 is a copy with a checksum; dst == src cycles in
 * place, and with MODGPU_DIGEST_INPUT the record is then of the bytes as they were before the call.  The bytes of workspace a call
 * over n_entries needs (0 for none, or above MODGPU_TABLE_MAX_ENTRIES) -- modgpu_table_workspace_bytes(n_entries), the same layout: */
uint64_t modgpu_cycle_digest_table_workspace_bytes(uint64_t n_entries);

/* The contract is modgpu_cycle_table_device's for the data and modgpu_digest_table_device's for the records, word for word where each
 * applies: THREE launches (plan, finish, stream) whatever the count -- path_stats().gpu_launches counts 3, modgpu_last_launch reports
 * the stream launch as variant 18 with `bytes` = 0 and modgpu_table_kernel_source_hash() --; asynchronous on `hip_stream`,
 * allocation-free, capturable into a hipGraph; the table is read when the call RUNS on the device, so a replay picks up rewritten
 * entries; the workspace (8-byte aligned device memory of `device`) is the caller's, reset by the plan launch in stream order, and two
 * calls on one workspace must not overlap in time.  modgpu_table_status reports this call too.
 *   * dev_records: n_entries records in device memory of `device`, 8-byte aligned, the caller's.  THE CALL INITIALISES THEM ITSELF, AND
 *     WITHOUT A MEMSET NODE: the finish launch stores every entry's record whole (the sums of the < 16 ragged bytes at either end of
 *     the entry, and n), the stream launch then only adds to valid records (non-returning 64-bit atomic adds).  A replayed graph
 *     starts clean.
 *   * Tier 1 (host, MODGPU_ERR_INVALID before anything is queued): modgpu_digest_table_device's tier 1 with this call's workspace
 *     size, and a `side` that is neither of the two constants (refused whatever n_entries is).  n_entries == 0 queues nothing.
 *   * Tier 2 (device, by the plan launch): modgpu_cycle_table_device's -- a NULL dst or src with n > 0 (a NULL dst is a refusal here:
 *     modgpu_digest_table_device is the call that only reads), nonzero flags, an entry of 1 TiB or more, more than 2^31 chunks of
 *     64 KiB together.  Any of these makes the whole call write NOTHING AT ALL -- no byte of any destination and no record -- and
 *     modgpu_table_status names the lowest such entry.
 *   * Tier 3: overlaps follow modgpu_cycle_table_device's rule (modgpu_table_validate checks it on a host copy), unchecked on the
 *     device.  Records that overlap an entry's range are the caller's error. */
int modgpu_cycle_digest_table_device(const modgpu_table_entry_t *dev_entries, uint64_t n_entries, modgpu_digest_result_t *dev_records,
                                     uint32_t side, void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);

/* ---- REKEY DIGEST TABLE: modgpu_rekey_table_device and one digest record per entry, in the same pass and the same three launches ------
 * "Convert the 100 000 files of this part PS3 -> PS4 and tell me that they are the files of my manifest": the manifest holds plaintext
 * Adler-32 values, and the plaintext of a rekey pass lies between the two keystreams, in registers only -- so this call is the one way
 * to checksum it in the pass that handles it (2n bytes of traffic, where modgpu_rekey_table_device followed by
 * modgpu_digest_table_device over a second table of 40-byte entries moves 3n in six launches).  Per entry
 *   * `dst` receives, byte for byte, what modgpu_rekey_table_device writes for the same table -- and nothing next to it is touched;
 *   * dev_records[i] receives {s1, s2, n, 0} as modgpu_digest_device defines it (only the residues mod 65521 of s1 and s2 specified),
 *     of the side asked for: MODGPU_DIGEST_OUTPUT (the bytes stored), MODGPU_DIGEST_INPUT (the source bytes as read; with dst == src
 *     the bytes as they were before the call), or */
#define MODGPU_DIGEST_PLAIN 2u  /* records are of src[j] ^ ks(key_from)[off_from + j]: the plaintext between the two keystreams */
/* Records are read back and closed with modgpu_digest_results / modgpu_digest_adler32, or checked where they lie with
 * modgpu_digest_check_device.  An empty entry gives {0, 0, 0, 0}.  modgpu_cycle_digest_table_device has one keystream and keeps refusing
 * side 2.  The bytes of workspace a call over n_entries needs (0 for none, or above MODGPU_TABLE_MAX_ENTRIES) --
 * modgpu_rekey_table_workspace_bytes(n_entries), the same layout: */
uint64_t modgpu_rekey_digest_table_workspace_bytes(uint64_t n_entries);

/* The contract is modgpu_rekey_table_device's for the data and modgpu_cycle_digest_table_device's for the records, word for word where
 * each applies: the 56-byte entry as it stands; every degenerate key pair (a key == 0 mod 2^31-1 on either side or both, one key at
 * offsets equal mod 2^31-2) handled in the same pass; dst == src rekeys in place; THREE launches (plan, finish, stream) whatever the
 * count -- path_stats().gpu_launches counts 3, modgpu_last_launch reports the stream launch as variant 20 with `bytes` = 0 and
 * modgpu_rekey_table_kernel_source_hash() --; asynchronous on `hip_stream`, allocation-free, capturable into a hipGraph; the table is
 * read when the call RUNS on the device, so a replay picks up rewritten entries; the workspace (8-byte aligned device memory of
 * `device`) is the caller's, reset by the plan launch in stream order, and two calls on one workspace must not overlap in time.
 * modgpu_table_status reports this call too.
 *   * dev_records: n_entries records in device memory of `device`, 8-byte aligned, the caller's.  THE CALL INITIALISES THEM ITSELF, AND
 *     WITHOUT A MEMSET NODE: the finish launch stores every entry's record whole (the sums of the < 16 ragged bytes at either end of
 *     the entry, and n), the stream launch then only adds to valid records (non-returning 64-bit atomic adds).  A replayed graph
 *     starts clean.
 *   * Tier 1 (host, MODGPU_ERR_INVALID before anything is queued): modgpu_cycle_digest_table_device's tier 1 with this call's
 *     workspace size, and a `side` that is none of the three constants (refused whatever n_entries is).  n_entries == 0 queues nothing.
 *   * Tier 2 (device, by the plan launch): modgpu_rekey_table_device's -- a NULL dst or src with n > 0, nonzero flags or reserved, an
 *     entry of 1 TiB or more, more than 2^31 chunks of 64 KiB together.  Any of these makes the whole call write NOTHING AT ALL -- no
 *     byte of any destination and no record -- and modgpu_table_status names the lowest such entry.
 *   * Tier 3: overlaps follow modgpu_rekey_table_device's rule (modgpu_rekey_table_validate checks it on a host copy), unchecked on
 *     the device.  Records that overlap an entry's range are the caller's error. */
int modgpu_rekey_digest_table_device(const modgpu_rekey_table_entry_t *dev_entries, uint64_t n_entries, modgpu_digest_result_t *dev_records,
                                     uint32_t side, void *dev_workspace, uint64_t workspace_bytes, int device, void *hip_stream);

/* ---- DIGEST CHECK: are these records the checksums of my manifest, and if not, which entry first?  On the device, in two launches ------
 * The digest calls leave one record per entry in device memory; the caller holds a manifest of Adler-32 values.  This call closes every
 * record where it lies and compares it with the manifest, so that nobody downloads 32 bytes per entry, finalises them on the host and
 * compares in a loop -- and so that a captured graph that digests a part can decide without the host.  It takes the records of every
 * digest producer: modgpu_digest_device / _batch_device, modgpu_digest_table_device, modgpu_cycle_digest_table_device,
 * modgpu_rekey_digest_table_device, and the digesting list transfers (modgpu_cycle_host_to_device_list_digest / _device_to_host_list_digest,
 * which are synchronous: dev_table_workspace NULL).
 * Entry i is BAD when the Adler-32 of dev_records[i] differs from dev_expect[i]; the Adler-32 is exactly what modgpu_digest_adler32
 * computes (the residues of s1, s2 and n mod 65521 first; A = (1 + s1) % m, B = (n + n * s1 - s2) % m; B << 16 | A; s1 and s2 may hold
 * any 64-bit value), and both halves are compared.
 * The whole check in 32 bytes.  The layout is pinned (8-byte aligned). */
typedef struct modgpu_digest_check_summary {
    uint64_t bad_entries;     /* entries whose record does not close to expect[i] */
    uint64_t first_bad_entry; /* the lowest such i; UINT64_MAX if none */
    uint64_t entries;         /* n_entries of the call that ran */
    uint64_t refused;         /* 1: the table call that produced the records was refused (see below); else 0 */
} modgpu_digest_check_summary_t;

/* The bytes of a bitmap over n_entries: 8 * ceil(n_entries / 64); 0 for 0 or above MODGPU_TABLE_MAX_ENTRIES. */
uint64_t modgpu_digest_check_bits_bytes(uint64_t n_entries);

/* dev_records: n_entries records; dev_expect: n_entries Adler-32 values; dev_summary: the 32 bytes above; all device memory of `device`.
 *   * dev_bad_bits, when not NULL: modgpu_digest_check_bits_bytes(n_entries) bytes.  Word w holds bit b set exactly when entry
 *     64 * w + b is bad; every word of ceil(n_entries / 64) is stored whole and the tail bits are 0, so nothing needs clearing
 *     beforehand.  A caller who wants to know which entries are bad downloads n / 8 bytes instead of 32 n.
 *   * dev_table_workspace, when not NULL: the workspace of the modgpu_digest_table_device, modgpu_cycle_digest_table_device or
 *     modgpu_rekey_digest_table_device call that produced the records (only its first 64 bytes, the table call's header, which all
 *     three kinds of workspace start with, are looked at).  The check reads the header's
 *     status ON THE DEVICE WHEN IT RUNS: if that table call was refused -- its records are then whatever the caller left there -- the
 *     check compares nothing, writes {0, UINT64_MAX, n_entries, 1} and leaves dev_bad_bits untouched.  A captured "digest table + check"
 *     graph is so honest on every replay, with no host in between.  With NULL the records are taken as they are: use NULL for the
 *     records of modgpu_digest_device / _batch_device.
 *   * Asynchronous on `hip_stream`; `device` -1 = the current device, an explicit device leaves the thread's current device as it was;
 *     allocation-free; capturable into a hipGraph.  THE CALL INITIALISES ITS SUMMARY ITSELF, IN STREAM ORDER, so a replay starts clean.
 *     It draws no ticket and has no degraded route.  EVERYTHING BUT THE SUMMARY AND THE BITS IS READ-ONLY.  The caller orders the call
 *     behind the producer: the same stream, or an event.
 *   * TWO launches whatever n_entries is (the init, then the check): path_stats().gpu_launches counts 2, modgpu_last_launch reports
 *     the check launch as variant 19 with `bytes` = 0 and modgpu_verify_table_kernel_source_hash().
 *   * Tier 1 (host, MODGPU_ERR_INVALID before anything is queued, with a text in modgpu_last_error()): NULL records, expect or summary
 *     with n_entries > 0; records, summary, bits or the table workspace not 8-byte aligned; expect not 4-byte aligned; more than
 *     MODGPU_TABLE_MAX_ENTRIES entries; summary or bits overlapping the records, expect or each other; any of the given ranges (of
 *     the table workspace its first 64 bytes) not reported as device memory of `device` (both ends of a range are asked about, as
 *     modgpu_digest_results does).  n_entries == 0 queues nothing and touches nothing. */
int modgpu_digest_check_device(const modgpu_digest_result_t *dev_records, const uint32_t *dev_expect, uint64_t n_entries,
                               const void *dev_table_workspace, modgpu_digest_check_summary_t *dev_summary, uint64_t *dev_bad_bits,
                               int device, void *hip_stream);

/* The summary from device memory of `device` into host_out.  Synchronous (a small copy from the device, like
 * modgpu_verify_table_summary): call it after the caller has synchronised the stream the check ran on.  MODGPU_ERR_INVALID when
 * refused != 0 (host_out is filled all the same). */
int modgpu_digest_check_summary(const modgpu_digest_check_summary_t *dev_summary, int device, modgpu_digest_check_summary_t *host_out);

/* Replaces CEncryptionCycler::Cycle (CEncryptionCycler.cpp:4-14) for a caller-owned HOST buffer,
 * on the GPU.  Pageable memory is staged through page-locked slots owned by this library (memcpy ->
 * slot -> kernel across PCIe on the slot -> memcpy back, chunked over several host threads and
 * overlapped; below 2 GiB ONE kernel serves the whole call and takes each chunk when its copy in has
 * landed); memory from modgpu_host_alloc / modgpu_host_register is cycled where it lies by one
 * kernel across PCIe, with no staging copy.  Synchronous: on return host_buf holds the result.
 * Never retains or frees host_buf. */
int modgpu_cycle_host(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int device);

/* The library's own host loop for the same arithmetic (closed form of CEncryptionCycler.cpp:16-25,
 * sixteen independent byte states like one GPU lane-word; threads for large buffers).  This is
 * product code for hosts without a GPU -- it shares nothing with the test oracle under oracle/. */
int modgpu_cycle_scalar_host(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off);

/* What CEncryptionCycler::Cycle binds to (`if (n < threshold || !gpu_ok) cpu_loop(); else ...`).
 * n < MODGPU_MIN_GPU_BYTES -- the headers the reference's three call sites pass -- is served by the host loop,
 * which finishes such a buffer before a kernel launch would have returned; larger buffers by modgpu_cycle_host.
 * The reference's Cycle returns void and cannot fail (CEncryptionCycler.cpp:4-14) and its callers do not guard it
 * (CArk.cpp:338-339, 1135-1136, Modulate.cpp:485-486), so the host loop finishes the call
 *   - when no GPU is visible, or the GPU attempt fails before it has changed host_buf: the whole buffer;
 *   - when the GPU is lost AFTER the call has begun on ordinary (pageable) memory -- what an unmodified caller passes,
 *     `new char[]` at CArk.cpp:320, 738, 780 -- : the buffer travels in pieces through page-locked slots and a piece changes
 *     host_buf only when it is copied back whole, so the library knows which pieces have arrived; the other pipelines of the
 *     call stop at once and the host loop does exactly the pieces that have not (keystream position = stream_off + the
 *     piece's offset).  modgpu_path_stats().midcall_rescues counts such calls.
 * ONE case stays an error: page-locked memory (modgpu_host_alloc / _register) is cycled where it lies by one kernel across
 * PCIe; if that kernel dies under way nobody knows which bytes it had written, and the plaintext exists nowhere else.  The call
 * then returns MODGPU_ERR_HIP with host_buf in an undefined state.  (A caller that must survive even that keeps its own copy,
 * or passes pageable memory.)  With MODGPU_REQUIRE_GPU=1 there is no second engine: every size runs on the kernel and a GPU
 * error is returned.
 * Above the threshold the default policy is to OFFLOAD: on a host with many cores the threaded host loop is faster than one
 * GPU's PCIe link for host-resident data (the link, ~50 GB/s, is the bound), but the kernel leaves those cores to the caller
 * and scales with the number of GPUs; MODGPU_HOST_POLICY=fastest picks the faster engine per call instead. */
int modgpu_cycle_auto_host(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int device);

/* Header framing of CArk::Load (CArk.cpp:328-339) and Decode (Modulate.cpp:475-486):
 * LE u32 magic at hdr[0..3] selects the key, the cipher covers hdr[4..size).  Host buffer; the cipher call is
 * Cycle's, so the engine is chosen exactly as by modgpu_cycle_auto_host (headers are at most 512 KiB,
 * CArk.cpp:911-912: the host loop unless MODGPU_REQUIRE_GPU=1 or MODGPU_MIN_GPU_BYTES says otherwise).
 * An unknown magic is MODGPU_ERR_MAGIC before anything is touched. */
int modgpu_hdr_decrypt_host(uint8_t *hdr, uint64_t size, int device);

/* Header framing of SaveArk (CArk.cpp:914-915, 1135-1136): stores the platform magic at
 * hdr[0..3] (ps4 != 0 -> PS4) and encrypts hdr[4..size) with the platform key.  Host buffer; engine as above;
 * on failure the buffer is as it was. */
int modgpu_hdr_encrypt_host(uint8_t *hdr, uint64_t size, int ps4, int device);

/* Part-level sharding beside CArk::LoadArkData / lSaveArk (CArk.cpp:723-758, 845-899): part i
 * is an independent stream (its own Cycle from offset 0) and goes to GPU  i mod n_devices,
 * one host thread per GPU, no inter-GPU traffic.  n_devices <= 0 means all devices. */
int modgpu_cycle_parts_host(uint8_t *const *parts, const uint64_t *sizes, int n_parts,
                            int32_t key, int n_devices);

/* ONE host buffer over several GPUs: contiguous spans (multiples of 2 MiB, at least 64 MiB each), span d on GPU d with
 * stream offset stream_off + its position -- jump-ahead makes every span an independent stream, so there is still no
 * exchange step -- each through its own PCIe link, one host thread per GPU.  n_devices <= 0 means all devices;
 * a buffer under 128 MiB stays on one GPU.  Result identical to modgpu_cycle_host. */
int modgpu_cycle_host_split(uint8_t *host_buf, uint64_t n, int32_t key, uint64_t stream_off, int n_devices);

/* The same for parts that are already resident in HBM, part i on GPU devices[i] (BASELINE config 3: 8 x 4 GiB,
 * one per GPU).  The launches are asynchronous, so the calling thread alone keeps every GPU busy; the call
 * returns when all of them have finished.  No inter-GPU traffic.  Parts that share a GPU go to it through
 * modgpu_cycle_batch_device.
 * Ordering: the kernels run on a stream of the library's own per device (non-blocking).  Work the caller queued BEFORE the call
 * on a device's NULL stream or on any of its blocking streams -- an asynchronous upload or memset of a part, a kernel that
 * produces it -- is finished before that device's parts are cycled (the library's stream waits for an event recorded on the
 * NULL stream at entry).  Work on the caller's own NON-blocking streams is not ordered: synchronise those before the call. */
int modgpu_cycle_parts_device(void *const *dev_parts, const uint64_t *sizes, const int *devices, int n_parts, int32_t key);

/* ---- part files streamed through the GPU ----------------------------
 * The reference reads a part with one fread into the concatenated buffer (CArk.cpp:751) and writes
 * a slice with one fwrite (CArk.cpp:883).  These do the same transfers with the cipher applied on
 * the way, overlapped, several chunks in flight: pread into a page-locked slot -> the kernel cycles the
 * slot across PCIe (file -> memory below 2 GiB: ONE kernel launch for the whole call) -> copy / pwrite
 * out; page-locked caller memory on the SOURCE side is DMA'd from where it lies.  Each call is one
 * stream whose first byte has keystream position stream_off (0 = a part's own Cycle). */

/* Whole file src_path -> dst_path (created / truncated).  The two may name the same file, by any
 * spelling (compared by device and inode): it is then cycled in place.
 * All three file routes share one rule for a GPU that is LOST AFTER THE CALL HAS BEGUN: the source still holds every byte (a
 * destination file is written piece by piece, each only when it is finished, also in place), so the pieces that have not
 * arrived are read again and done by the library's host loop -- unless MODGPU_REQUIRE_GPU=1; modgpu_path_stats().midcall_rescues
 * counts such calls.  Without a usable GPU at the start they fail like every other kernel entry point. */
int modgpu_cycle_file(const char *src_path, const char *dst_path, int32_t key, uint64_t stream_off, int device);

/* n bytes at byte offset file_off of `path` -> host_dst[0..n) (any kind of memory; the rule above holds whatever host_dst is). */
int modgpu_cycle_file_to_host(const char *path, uint64_t file_off, uint8_t *host_dst, uint64_t n, int32_t key,
                              uint64_t stream_off, int device);

/* host_src[0..n) -> `path` (created / truncated).  host_src is not modified. */
int modgpu_cycle_host_to_file(const uint8_t *host_src, uint64_t n, const char *path, int32_t key, uint64_t stream_off,
                              int device);

/* ---- transfers: the cipher in flight between host memory (or a part file) and a buffer the caller keeps on the GPU ----------
 * dst[j] = src[j] ^ ks[stream_off + j], j = 0 .. n-1: same keystream, 64-bit offsets and key reduction as modgpu_cycle_device.
 *   modgpu_cycle_host_to_device   host_src -> dev_dst (upload: each byte crosses the link once, into device memory)
 *   modgpu_cycle_device_to_host   dev_src -> host_dst (download: each byte is read from device memory and crosses the link once)
 *   modgpu_cycle_file_to_device   n bytes at byte offset file_off of `path` -> dev_dst
 *   modgpu_cycle_device_to_file   dev_src -> `path`, written the way modgpu_cycle_host_to_file writes it (created / truncated, 0644)
 * THE SOURCE IS NEVER WRITTEN: host memory, file or device buffer.  A host side may be pageable memory, page-locked memory
 * (modgpu_host_alloc / modgpu_host_register; then the GPU reads or writes it across PCIe where it lies) or a read-only mapping.
 * SYNCHRONOUS: the result is in place when the call returns.  NO ORDERING against the caller's streams: the call does not wait for
 * work the caller has queued on any stream (the NULL stream included) -- synchronise before the call if that work touches the
 * device buffer.  The library's own work runs on its own non-blocking streams.  `device` -1 = the current device; the calling
 * thread's current device is the same afterwards.  Edge cases:
 *   - both pointers may have any byte alignment; n == 0 does nothing (the _to_file call still creates / truncates its file);
 *   - a NULL pointer with n > 0 is MODGPU_ERR_INVALID;
 *   - a device pointer that the runtime does not report as device memory of the call's device (hipPointerGetAttributes, both
 *     ends of the range) is MODGPU_ERR_INVALID, returned before anything is queued;
 *   - keys == 0 mod 2^31-1 (identity keystream) copy the bytes unchanged.
 * Kernel entry points: no host loop behind them -- no GPU is MODGPU_ERR_NO_DEVICE, a GPU lost in the middle of the call or a transfer
 * kernel that stops responding is MODGPU_ERR_HIP after a bounded wait (never a hang).  When a call fails the source is intact and the
 * destination's contents are unspecified.  path_stats().gpu_launches counts the launches: one per call (calls above ~63 GiB from
 * pageable memory or a file take one per ~63 GiB). */
int modgpu_cycle_host_to_device(void *dev_dst, const uint8_t *host_src, uint64_t n, int32_t key, uint64_t stream_off, int device);
int modgpu_cycle_device_to_host(uint8_t *host_dst, const void *dev_src, uint64_t n, int32_t key, uint64_t stream_off, int device);
int modgpu_cycle_file_to_device(const char *path, uint64_t file_off, void *dev_dst, uint64_t n, int32_t key,
                                uint64_t stream_off, int device);
int modgpu_cycle_device_to_file(const void *dev_src, uint64_t n, const char *path, int32_t key, uint64_t stream_off,
                                int device);

/* ---- transfers of a LIST of ranges: the files of a part onto or off the GPU in one call ----------------------------------------
 * host_entries is a HOST array of modgpu_table_entry_t, the 40-byte entry of the table calls (one table builder serves both):
 *   modgpu_cycle_host_to_device_list   upload: every entry's dst is device memory of `device`, its src host memory
 *   modgpu_cycle_device_to_host_list   download: every entry's dst is host memory, its src device memory of `device`
 * Per entry dst[j] = src[j] ^ ks(key)[stream_off + j], j < n -- exactly what the single transfer call above computes for it, and under
 * the single calls' contract wherever it applies: SYNCHRONOUS, NO ORDERING against the caller's streams, THE SOURCE IS NEVER WRITTEN,
 * any byte alignment on both sides of every entry, 64-bit offsets reduced mod the period, a key == 0 mod 2^31-1 copies, entries with
 * n == 0 are skipped (their pointers may be NULL); n_entries == 0, or a list with no bytes, queues nothing and returns MODGPU_OK.  No
 * GPU is MODGPU_ERR_NO_DEVICE; a GPU lost in the middle of the call or a kernel that stops responding is MODGPU_ERR_HIP after the
 * single calls' bounded wait, the sources then intact and the destinations unspecified.
 * ONE LAUNCH per call whatever n_entries is: path_stats().gpu_launches counts it, modgpu_last_launch reports it as variant 21 with
 * `bytes` = the list's total and modgpu_xfer_kernel_source_hash().  The entries' bytes travel as one packed stream through the
 * library's page-locked slots (page-locked caller memory too: it is copied like any other); the list is read, and a plan of 24 bytes
 * per non-empty entry put into device memory, before the launch.  A list of more bytes than the single call's one-launch limit (about
 * 63 GiB) IS CUT the way a single call is: one launch per ~63 GiB of the packed stream (modgpu_last_launch then reports the last, with
 * that launch's bytes).  A piece of the stream that is made of very many tiny entries (a few bytes each) is correct and slow: its
 * entries are done one after another.
 * Refused before anything is queued, MODGPU_ERR_INVALID with modgpu_last_error() naming the LOWEST entry at fault ("entry <i>: ..."):
 * a NULL list with n_entries > 0; n_entries above MODGPU_TABLE_MAX_ENTRIES; an entry with a NULL pointer and n > 0; an entry with
 * nonzero flags; an entry of 2^39 bytes or more; an entry whose device side the runtime does not report as device memory of the
 * call's device (the single call's rule, both ends of the range; entries whose device ranges touch end to start are looked up as one
 * range).  Without a GPU these refusals are the same, except the last, which needs the device.
 * NOT CHECKED: overlap.  In an upload the (device) destinations may not meet each other, in a download the (host) destinations may
 * not meet each other; sources may overlap or repeat.  Bytes in ranges that break the rule are unspecified, but nothing outside the
 * entries' [dst, dst+n) is ever written.  modgpu_table_validate checks a list against this rule. */
int modgpu_cycle_host_to_device_list(const modgpu_table_entry_t *host_entries, uint64_t n_entries, int device);
int modgpu_cycle_device_to_host_list(const modgpu_table_entry_t *host_entries, uint64_t n_entries, int device);

/* ---- list transfers WITH A DIGEST: one record of sums per entry, taken in the same launch while the bytes are in registers --------------
 * The contract for the data is the list calls' above, word for word: synchronous, no ordering against the caller's streams, the source
 * never written, any alignment, entries of n == 0 skipped, one launch per call (cut into windows above the one-launch limit), the same
 * refusals with the same texts naming the lowest entry at fault, overlap not checked.  On top of that:
 *   * dev_records is device memory of `device`, 32 bytes per entry of the list, dev_records[i] the record of host_entries[i] (empty
 *     entries included).  It receives {s1, s2, n, 0} as modgpu_digest_device defines it (only the residues mod 65521 of s1 and s2
 *     specified) of the side asked for: MODGPU_DIGEST_OUTPUT sums out[j] = src[j] ^ ks(key)[stream_off + j], what is stored;
 *     MODGPU_DIGEST_INPUT sums src[j] as read -- a packer's plaintext checksums while the ciphertext goes up, an extractor's ciphertext
 *     checksums while the plaintext comes down.  An empty entry gives {0, 0, 0, 0}; a key == 0 mod 2^31-1 is a copy with a checksum.
 *   * Records are read back and closed with modgpu_digest_results / modgpu_digest_adler32, or checked where they lie with
 *     modgpu_digest_check_device (dev_table_workspace NULL).
 *   * THE CALL WRITES ITS RECORDS ITSELF, {0, 0, n, 0} each, before its first launch: nothing needs clearing, and calling twice on the
 *     same records gives the same records.  An entry cut by a window boundary still ends with the record of the WHOLE entry.
 *   * Further refusals, MODGPU_ERR_INVALID before anything is queued (nothing written, gpu_launches unchanged): dev_records NULL with
 *     n_entries > 0; dev_records not 8-byte aligned; a `side` other than the two; a records range that the runtime does not report as
 *     device memory of the call's device (both ends); a records range that meets an entry's device range ("entry <i>: ...").
 *   * n_entries == 0 touches nothing and is MODGPU_OK.  A list with entries but no bytes still writes its records (no launch), so
 *     without a GPU it is MODGPU_ERR_NO_DEVICE.  When a call fails the records are unspecified, like the destinations.
 *   * modgpu_last_launch reports variant 22 with `bytes` = the launch's window of the packed stream. */
int modgpu_cycle_host_to_device_list_digest(const modgpu_table_entry_t *host_entries, uint64_t n_entries, uint32_t side,
                                            modgpu_digest_result_t *dev_records, int device);
int modgpu_cycle_device_to_host_list_digest(const modgpu_table_entry_t *host_entries, uint64_t n_entries, uint32_t side,
                                            modgpu_digest_result_t *dev_records, int device);

/* ---- page-locked host memory -----------------------------------------------------------------
 * Replaces the `new char[total]` of CArk::LoadArkData / BuildArk (CArk.cpp:738, 780) for callers
 * that will cycle the buffer: the GPU's DMA engines and kernels reach these pages directly, so
 * the host-buffer entry points above skip both staging copies for any range inside them.
 * Without a GPU, or if the pages cannot be locked (locked-memory limit), the memory is ordinary (64-byte
 * aligned) and everything still works through the staged route; modgpu_host_is_pinned tells which it is. */
int modgpu_host_alloc(void **host_ptr, uint64_t n);
int modgpu_host_free(void *host_ptr);
/* The same, placed for a multi-socket node: the pages are bound to the NUMA node the GPU hangs off
 * (/sys/bus/pci/devices/<bdf>/numa_node; mbind, preferred policy) before they are locked, so the bytes that
 * cross PCIe to that GPU come from its own socket's DRAM.  modgpu_host_alloc_parts makes ONE contiguous buffer
 * for a list of parts laid end to end -- the concatenated buffer of CArk::LoadArkData / BuildArk (CArk.cpp:738,
 * 780) -- with part i's pages next to GPU i mod n_devices, the GPU modgpu_cycle_parts_host sends it to
 * (n_devices <= 0: all).  With MODGPU_NUMA=0 or without a GPU both are modgpu_host_alloc.  Otherwise
 * modgpu_host_alloc_parts always takes its own route -- reserve, bind each part's pages where its GPU's node is known (a part
 * whose GPU's node cannot be read, e.g. no numa_node in a container's sysfs, is simply not bound), first-touch from several
 * threads, page-lock in place -- because that route is also the faster way to get GB-sized page-locked memory (0.27 s against
 * 0.43-0.51 s for 3.3 GB); modgpu_host_alloc_near falls back to modgpu_host_alloc when its one device's node is unknown.
 * Free with modgpu_host_free.  Worker threads of the host-buffer routes run on their GPU's node as well.  Placement is
 * best effort and changes no result. */
int modgpu_host_alloc_near(void **host_ptr, uint64_t n, int device);
int modgpu_host_alloc_parts(void **host_ptr, const uint64_t *sizes, int n_parts, int n_devices);
/* NUMA node of the GPU behind `device`, -1 if unknown or placement is off. */
int modgpu_device_numa_node(int device);
/* For callers that cannot change how their buffer is allocated: page-locks [host_ptr, host_ptr + n) where it
 * lies (hipHostRegister) so that later cycles of ranges inside it take the no-copy route.  Pinning costs
 * about as much as one staged pass over the buffer, so it pays from the second cycle on.  Unregister
 * before freeing the memory.  Without a GPU both calls succeed and do nothing. */
int modgpu_host_register(void *host_ptr, uint64_t n);
int modgpu_host_unregister(void *host_ptr);
/* 1 if [p, p+n) lies inside one page-locked, device-visible allocation or registration, else 0. */
int modgpu_host_is_pinned(const void *p, uint64_t n);

/* ---- which engine ran ---------------------------------------------------------------------- */
typedef struct modgpu_path_stats {
    uint64_t gpu_calls;      /* host-buffer / file calls served by the kernel                    */
    uint64_t gpu_bytes;      /* payload bytes those calls cycled                                 */
    uint64_t gpu_launches;   /* kernel launches, modgpu_cycle_device included                    */
    uint64_t scalar_calls;   /* calls served by the host loop (direct or through _auto_)         */
    uint64_t scalar_bytes;
    uint64_t staged_bytes;   /* of gpu_bytes: went through a pageable<->pinned memcpy            */
    uint64_t direct_bytes;   /* of gpu_bytes: DMA'd or read straight from the caller's pinned pages */
    uint64_t auto_fallbacks; /* modgpu_cycle_auto_host calls that ended on the host loop because the GPU could not serve them */
    uint64_t auto_small;     /* modgpu_cycle_auto_host calls served by the host loop because n < MODGPU_MIN_GPU_BYTES */
    uint64_t auto_policy_host; /* modgpu_cycle_auto_host calls of n >= MODGPU_MIN_GPU_BYTES that MODGPU_HOST_POLICY=fastest kept on the host loop */
    uint64_t midcall_rescues;       /* calls (modgpu_cycle_auto_host, the modgpu_cycle_file* routes) whose GPU was lost AFTER the call had begun and
                                       that the host loop finished: counted in gpu_calls AND -- for _auto_ -- in auto_fallbacks */
    uint64_t midcall_rescued_bytes; /* bytes of those calls the host loop did (in scalar_bytes, not in gpu_bytes) */
} modgpu_path_stats_t;
/* Process-wide counters since load (or the last reset).  reset != 0 zeroes them after the read. */
int modgpu_path_stats(modgpu_path_stats_t *out, int reset);
/* 1 if MODGPU_REQUIRE_GPU=1 was set when the library was loaded. */
int modgpu_gpu_required(void);
/* modgpu_cycle_auto_host's size threshold as latched from MODGPU_MIN_GPU_BYTES. */
uint64_t modgpu_min_gpu_bytes(void);
/* "offload" or "fastest": MODGPU_HOST_POLICY as latched.  Static storage. */
const char *modgpu_host_policy(void);
/* What `fastest` would decide for one call over n bytes of pageable (pinned = 0) or page-locked (1) memory on this host:
 * returns 1 for the host loop, 0 for the kernel, and the two priced durations in microseconds (either pointer may be NULL).
 * The prices come from the crossover table the library was built with (modulate_amd/csrc/crossover_table.h). */
int modgpu_host_policy_engine(uint64_t n, int pinned, double *host_us, double *kernel_us);
/* The host-loop body this process uses: "generic", "avx2" or "avx512".  Static storage. */
const char *modgpu_host_loop_isa(void);

/* ---- device-memory helpers (bench / tests / callers that keep parts resident) ---------
 * hipMalloc / hipFree / hipMemcpy / a synchronize on the named device -- plus two pieces of housekeeping that are NOT in their
 * names, both best effort (whatever fails there is retried or simply paid by the caller's first launch) and both outside
 * anybody's timed launch:
 *   modgpu_alloc   the FIRST allocation on a device in this process also prepares the device: the code object is loaded, the
 *                  work-queue kernel's ticket ring is set up, and two real, tiny work-queue launches (2 x 64 KiB of scratch) run
 *                  and are waited for on a private stream.  A process's first real launch of that kernel otherwise costs 10 ms
 *                  (code object) + 15-35 us (kernel function, ring) inside whatever the caller times
 *                  (profiles/r03_first_pass.txt, r05_first_launch.txt).
 *   modgpu_h2d     a copy of 1 MiB or more first enqueues ONE EMPTY KERNEL (one workgroup, no words) on a private non-blocking
 *                  stream that nobody waits for: an upload keeps only the DMA engines busy, the shader engines fall asleep within a
 *                  fraction of a second, and the first launch behind the upload would pay their wake-up (~15 us on a 411 MB part:
 *                  0.72 -> 0.81 of the HBM peak for that launch).  Costs the caller one asynchronous launch call per copy.
 * A caller that brings its own device memory (hipMalloc / hipMemcpy of its own, a torch tensor) gets neither -- unless it says so:
 *   modgpu_prepare(device)   both of the above by name: prepares the device if this process has not yet, and enqueues the empty
 *                  wake-up launch.  Call it when your own upload STARTS (or any time before the first modgpu_cycle_device).
 *                  Never required for correctness.  Returns MODGPU_OK, or the error of selecting the device. */
int modgpu_alloc(void **dev_ptr, uint64_t n, int device);
int modgpu_free(void *dev_ptr, int device);
int modgpu_h2d(void *dev_dst, const void *host_src, uint64_t n, int device);
int modgpu_d2h(void *host_dst, const void *dev_src, uint64_t n, int device);
int modgpu_sync(int device, void *hip_stream);
int modgpu_prepare(int device);

/* ---- host-side jump-ahead arithmetic (exposed so it can be checked without a GPU) ---- */

/* State the reference loop holds when it XORs stream byte i: a^(i+1)*key mod m, in [1, m];
 * this is what the library feeds the kernel as its per-launch base. */
uint32_t modgpu_state_at(int32_t key, uint64_t i);

/* Fills out[0..count) with the kernel's compile-time jump tables so tests can verify them
 * against independent arithmetic.  which: 0 = a^j (j<16), 1 = a^(16*t) (t<256),
 * 2 = a^(4096*b) (b<256), 3 = a^(4096*256*b) (b<256).  Returns entries written. */
int modgpu_jump_table(int which, uint32_t *out, int count);

#ifdef __cplusplus
}
#endif
#endif /* MODGPU_H */
