// standin_launch_xfer_list_digest.cpp -- the DIGEST mode of the list mode of the transfer kernels (cycle_xfer_kernel.h: XferDigestRecord,
// XferListDigestRec, modgpu_launch_cycle_xfer_list_digest) on the CPU stand-in (hip/hip_runtime.h).  Like standin_launch_xfer_list.cpp,
// which it leaves alone and shares nothing with: a launch is queued on the stream's thread and runs WHILE the library's pipelines
// gather into and scatter out of their slots -- chunk after chunk of the packed stream it waits for `ready` (or `abort`, or its
// patience), moves the chunk between its slot and the entries' device sides byte by byte, each byte's entry found in the plan and its
// state taken from the entry's base with lcg.h's arithmetic, adds every byte of the side asked for and its position in its entry -- the
// plan record's skip_mod bytes in front of the record's own first byte -- onto the entry's record mod 65521, and marks the chunk `done`.
// A second implementation, written from the record types and lcg.h: the sanitizer runs see every byte and every record the plan says
// the kernel touches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_xfer_kernel.h"
#include "../../modulate_amd/csrc/lcg.h"

namespace {
std::atomic<unsigned long long> g_launches[2] = {}, g_gave_up{0}, g_plan_errors{0};

struct DigestLaunch {
    CycleXferArgs a;
    bool upload;
};

// the plan as the header states it (the list mode's rules), and the digest mode's: records, a side, and a digest record per plan record
// whose skip_mod is a residue
bool plan_ok(const CycleXferArgs &a)
{
    if (!a.list || a.list_n == 0 || a.list[0].start != 0 || a.slot_phase != 0 || a.chunk_bytes == 0 || a.chunk_bytes % kFeedPieceBytes != 0) return false;
    if (!a.records || !a.digest || a.side > 1u) return false;
    for (uint32_t e = 0; e < a.list_n; ++e) {
        if (!a.list[e].dev || a.list[e].start >= a.list[e + 1].start || a.list[e + 1].start - a.list[e].start >= kXferListEntryMax || a.list[e].copy > 1u) return false;
        if (a.digest[e].skip_mod >= kXferDigestMod || (e > 0 && (a.digest[e].entry <= a.digest[e - 1].entry || a.digest[e].skip_mod != 0))) return false;
    }
    return a.list[a.list_n].start == a.n && a.list[a.list_n].dev == nullptr;
}

void run_list_digest(void *arg)
{
    DigestLaunch *l = static_cast<DigestLaunch *>(arg);
    const CycleXferArgs &a = l->a;
    const bool good = plan_ok(a);
    if (!good) g_plan_errors.fetch_add(1);
    const uint64_t chunk = a.chunk_bytes ? a.chunk_bytes : kFeedPieceBytes;
    const uint64_t chunks = (a.n + chunk - 1) / chunk;
    bool gave_up = !good; // (a bad plan moves nothing: the call then times out or fails its model, loudly)
    uint32_t e = 0;       // the entry of the byte at hand: only ever moves forward, the stream is walked in packed order
    for (uint64_t c = 0; c < chunks && !gave_up; ++c) {
        const auto since = std::chrono::steady_clock::now();
        while (std::atomic_ref<const uint32_t>(a.ready[c]).load(std::memory_order_acquire) == 0u) {
            const double waited_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - since).count();
            if (std::atomic_ref<const uint32_t>(*a.abort).load(std::memory_order_acquire) != 0u || waited_s * 1e8 > (double)a.patience_ticks) {
                gave_up = true;
                break;
            }
            std::this_thread::yield();
        }
        if (gave_up) break;
        const uint64_t pos = c * chunk, len = std::min<uint64_t>(chunk, a.n - pos);
        uint8_t *const h = a.slot[(c % a.pipes) * 2 + (c / a.pipes) % 2];
        uint32_t state = 0;
        uint64_t s1 = 0, s2 = 0; // the sums of the run at hand, both below 65521 * 2^32 at any time
        bool fresh = true;       // the state has to be taken from the entry's base: the first byte of a chunk, and of every entry
        auto send = [&](uint32_t entry) { // (as the kernel sends them: added onto the record, which other chunks add onto as well)
            std::atomic_ref<unsigned long long>(a.records[entry].s1).fetch_add(s1 % kXferDigestMod, std::memory_order_relaxed);
            std::atomic_ref<unsigned long long>(a.records[entry].s2).fetch_add(s2 % kXferDigestMod, std::memory_order_relaxed);
            s1 = s2 = 0;
        };
        for (uint64_t j = 0; j < len; ++j) {
            const uint64_t p = pos + j;
            while (a.list[e + 1].start <= p) {
                if (!fresh) send(a.digest[e].entry);
                ++e, fresh = true;
            }
            const XferListRec &r = a.list[e];
            const uint64_t into = p - r.start;
            if (fresh) {
                state = lcg::mulmod(r.base, lcg::powmod(lcg::A, into % lcg::PERIOD));
                fresh = false;
            }
            const uint8_t ks = r.copy ? (uint8_t)0 : (uint8_t)~state;
            const uint8_t in = l->upload ? h[j] : r.dev[into], out = in ^ ks;
            if (l->upload) r.dev[into] = out;
            else h[j] = out;
            const uint64_t x = a.side ? in : out, at = (a.digest[e].skip_mod + into) % kXferDigestMod;
            s1 += x;
            s2 = (s2 + at * x) % kXferDigestMod;
            state = lcg::mulmod(state, lcg::A);
        }
        if (!fresh) send(a.digest[e].entry);
        std::atomic_ref<uint32_t>(a.done[c]).store(1u, std::memory_order_release);
    }
    if (gave_up) {
        g_gave_up.fetch_add(1);
        std::atomic_ref<uint32_t>(a.work[1]).fetch_add(1u);
    }
    g_launches[l->upload ? 1 : 0].fetch_add(1);
    delete l;
}
} // namespace

hipError_t modgpu_launch_cycle_xfer_list_digest(const CycleXferArgs &a, bool upload, uint32_t, hipStream_t stream)
{
    if (a.list == nullptr || a.list_n == 0 || a.ready == nullptr) return hipErrorInvalidValue;
    if (a.records == nullptr || a.digest == nullptr || a.side > 1u) return hipErrorInvalidValue;
    shim::enqueue(stream, run_list_digest, new DigestLaunch{a, upload});
    return hipSuccess;
}

extern "C" {
unsigned long long modgpu_shim_xfer_list_digest_launches(int upload) { return g_launches[upload ? 1 : 0].load(); }
unsigned long long modgpu_shim_xfer_list_digest_gave_up(void) { return g_gave_up.load(); }
unsigned long long modgpu_shim_xfer_list_digest_plan_errors(void) { return g_plan_errors.load(); }
}
