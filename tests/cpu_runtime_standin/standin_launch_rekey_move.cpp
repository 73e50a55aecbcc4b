// standin_launch_rekey_move.cpp -- the move launch of the rekey kernel (cycle_rekey_kernel.h, modgpu_launch_cycle_rekey_move) on the CPU
// stand-in (hip/hip_runtime.h).  Like standin_launch_rekey.cpp: the launch is queued on the stream's thread and does, from the launch
// PLAN alone, what the kernel's move loop would do to the body -- byte by byte with lcg.h, both keystreams, IN THE DIRECTION THE PLAN
// GIVES: ascending when the destination lies below the source, descending when above.  A plan with the wrong direction therefore
// gives wrong bytes here as it would on the device.  The plan is checked on the way: one entry, lead 0, no edges, a chunk-aligned
// destination, a whole number of words, and a dependence window that is the one the shift implies and looks at lower positions only.
#include "../../modulate_amd/csrc/cycle_rekey_kernel.h"
#include "standin_entry.h"

namespace {
namespace E = standin_entry;
std::atomic<unsigned long long> g_move_launches[2] = {}, g_move_plan_errors{0};

void run_move(CycleRekeyArgs &b, int form)
{
    const CycleRekeyPart &P = b.part[0];
    const int64_t chunk = modgpu_rekey_chunk_bytes();
    const uint64_t total = (P.end + chunk - 1) / chunk;
    const uintptr_t D = reinterpret_cast<uintptr_t>(P.dst_body), S = reinterpret_cast<uintptr_t>(P.src_body);
    unsigned long long bad = 0;
    bad += b.n_parts != 1 || P.lead != 0 || P.head_n != 0 || P.tail_n != 0 || P.end == 0 || (P.end & 15) != 0 || (D & (chunk - 1)) != 0;
    bad += b.start[0] != 0;
    for (int p = 1; p <= kCycleBatchMax; ++p) bad += b.start[p] != total;
    bad += !b.move_flags || !b.move_status || b.queue_done != nullptr || D == S || (b.move_down != 0) != (D > S);
    bad += (form == CYCLE_REKEY_FUNNEL) != (((S - D) & 3) != 0);
    // the window from the addresses themselves: chunk c + m reads the dwords of the source that hold its bytes
    {
        const int64_t delta = (int64_t)(S - D);
        const int64_t around = -(delta / chunk);
        int64_t lo = 0, count = 0;
        for (int64_t m = around - 4; m <= around + 4; ++m) {
            const int64_t first = (int64_t)(S & ~(uintptr_t)3) - (int64_t)D + m * chunk;                        // the dword that holds the first source byte
            const int64_t end = (int64_t)((S + (uintptr_t)chunk + 3) & ~(uintptr_t)3) - (int64_t)D + m * chunk; // behind the dword that holds the last
            if (m == 0 || !(first < chunk && end > 0)) continue;
            if (!count) lo = m;
            ++count;
            bad += delta > 0 ? m > 0 : m < 0; // a later position
        }
        bad += count != (int64_t)b.move_win_n || (count && lo != b.move_win_lo);
    }
    bad += !E::take_pair(b); // the pair is the workspace's own: always clean
    if (!bad) {
        uint32_t sa = P.base_body[0], sb = P.base_body[1];
        if (!b.move_down) {
            for (uint64_t i = 0; i < P.end; ++i) {
                P.dst_body[i] = P.src_body[i] ^ (uint8_t)~sa ^ (uint8_t)~sb;
                sa = lcg::mulmod(sa, lcg::A);
                sb = lcg::mulmod(sb, lcg::A);
            }
        } else {
            const uint32_t back = lcg::powmod(lcg::A, lcg::PERIOD - 1); // a^-1
            const uint32_t fwd = lcg::powmod(lcg::A, (P.end - 1) % lcg::PERIOD);
            sa = lcg::mulmod(sa, fwd);
            sb = lcg::mulmod(sb, fwd);
            for (uint64_t i = P.end; i-- > 0;) {
                P.dst_body[i] = P.src_body[i] ^ (uint8_t)~sa ^ (uint8_t)~sb;
                sa = lcg::mulmod(sa, back);
                sb = lcg::mulmod(sb, back);
            }
        }
        for (uint64_t c = 0; c < total; ++c) b.move_flags[c] = 1u;
    }
    g_move_plan_errors.fetch_add(bad);
    E::sign_off_pair(b); // (the workspace's pair has no sign-off word: a plan that carries one counted as an error above)
    g_move_launches[form == CYCLE_REKEY_FUNNEL ? 1 : 0].fetch_add(1);
}
} // namespace

hipError_t modgpu_launch_cycle_rekey_move(const CycleRekeyArgs &a, int form, uint32_t *grid, hipStream_t stream)
{
    if (*grid > 256u) *grid = 256u; // what the stand-in's device "holds at once"
    if (*grid == 0) *grid = 1;
    return E::enqueue<CycleRekeyArgs, run_move>(a, form, stream);
}

extern "C" unsigned long long modgpu_shim_move_launches(int form) { return form == 0 || form == 1 ? g_move_launches[form].load() : 0; }
extern "C" unsigned long long modgpu_shim_move_plan_errors(void) { return g_move_plan_errors.load(); }
