// standin_launch_rekey_relayout_table.cpp -- the two launches the relayout call (modgpu_rekey_relayout_table_device) adds to the rekey
// move table launches (cycle_rekey_move_table_kernel.h), on the CPU stand-in: the plan and the finish launch of one SWEEP.  The window,
// move and place launches that follow each pair are standin_launch_rekey_move_table.cpp's, as they stand: to them a filtered entry is
// an empty one.  Written from the record types and the header's words alone, like the other stand-ins:
//   plan    as the move call's, but an entry of the other direction (sweep 1: dst <= src; sweep 2: dst > src) is laid as an EMPTY
//           entry -- no chunks, no ragged ends -- while it keeps its refusal, its place in the prev / last links and its chunks in the
//           record's unfiltered sum (MoveTableBlk.pad).  Sweep 2 keeps the header's stalled word, and filters everything if it is set;
//   finish  as the move call's without the direction clause; refused on the UNFILTERED chunk sum, the entry named being the first whose
//           unfiltered chunks end beyond the room; the direction forced from the sweep.
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_rekey_move_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_relayout_launches[2] = {};
constexpr uint32_t kNone = ~0u;

bool filtered(const MoveTableArgs *a, const RekeyTableEntry &E, bool halted)
{
    const bool up = E.n != 0 && at(E.dst) > at(E.src);
    return halted || up != (a->sweep == kRelayoutSweepUp);
}

void run_plan(MoveTableArgs *a)
{
    const bool halted = a->sweep == kRelayoutSweepUp && a->hdr->stalled != 0;
    if (a->sweep != kRelayoutSweepUp) a->hdr->stalled = 0;
    a->hdr->up = 0;
    for (uint64_t k = 0; k < a->cap; ++k) a->flags[k] = 0;
    uint32_t prev = 0; // 1 + the previous non-empty entry of the record (local index)
    uint64_t all = 0;  // the record's chunks with no entry filtered
    plan(a, [&](uint64_t i, uint64_t run) {
        MoveTableBlk &B = a->blk[i / kTableBlock];
        if (i % kTableBlock == 0) {
            B = MoveTableBlk{0, 0, 0, kNone, kNone, {0, 0}};
            prev = 0;
            all = 0;
        }
        const RekeyTableEntry E = a->entries[i];
        Grid g = grid_of(E, E.flags | E.reserved);
        all += g.cnt;
        B.pad[0] = (uint32_t)all;
        B.pad[1] = (uint32_t)(all >> 32);
        RekeyTableEntry L = E; // what is laid: the entry, or an empty one at its addresses
        if (filtered(a, E, halted)) {
            L.n = 0;
            const uint32_t bad = g.bad;
            g = grid_of(L, 0);
            g.bad = bad;
        }
        plan_fields(a->plan[i], L, g, run);
        a->plan[i].prev = prev;
        plan_states(a->plan[i], a->edge[i], L, g);
        if (E.n) {
            prev = (uint32_t)(i % kTableBlock) + 1;
            B.last = (uint32_t)i + 1;
        }
        return g;
    });
}

void span_rekey(uint8_t *out, const uint8_t *src, uint64_t len, uint32_t sa, uint32_t sb)
{
    for (uint64_t j = 0; j < len; ++j) {
        out[j] = (uint8_t)(src[j] ^ (uint8_t)(sa ^ sb));
        sa = step(sa, 1);
        sb = step(sb, 1);
    }
}

void run_finish(MoveTableArgs *a)
{
    const uint64_t room = std::min<uint64_t>(a->cap, kTableMaxChunks);
    uint64_t all = 0;
    for (uint32_t b = 0; b < a->n_blk; ++b) all += (uint64_t)a->blk[b].pad[0] | (uint64_t)a->blk[b].pad[1] << 32;
    const bool fits = all <= room; // decided on the UNFILTERED sum: the same in both sweeps
    a->hdr->up = a->sweep == kRelayoutSweepUp ? 1u : 0u;
    uint32_t last = 0; // 1 + the last non-empty entry of the earlier records
    uint64_t upto = 0; // unfiltered chunks up to and including the entry
    auto entry = [&](uint64_t i, MoveTablePlan &P, bool ok) {
        const uint64_t b = i / kTableBlock;
        if (i % kTableBlock == 0 && b > 0 && a->blk[b - 1].last) last = a->blk[b - 1].last;
        const RekeyTableEntry E = a->entries[i];
        upto += grid_of(E, E.flags | E.reserved).cnt;
        if (!fits && (P.bad || upto > room)) a->hdr->first_bad = std::min<uint64_t>(a->hdr->first_bad, i);
        // the order rule: each non-empty entry against the non-empty one before it, whatever the direction of either
        if (E.n != 0 && !P.bad) {
            const uint64_t d = at(E.dst), s = at(E.src);
            const uint64_t q = P.prev ? b * kTableBlock + P.prev - 1 : last ? (uint64_t)last - 1 : kTableNoBad;
            if (q != kTableNoBad) {
                const RekeyTableEntry Q = a->entries[q];
                if (s < at(Q.src) || s - at(Q.src) < Q.n || d < at(Q.dst) || d - at(Q.dst) < Q.n) a->hdr->first_bad = std::min<uint64_t>(a->hdr->first_bad, i);
            }
        }
        if (!ok) return;
        const RekeyTableEdge &X = a->edge[i];
        uint8_t *out = a->scratch + i * kMoveTableScratch;
        span_rekey(out, P.src_origin + P.lead - P.head_n, P.head_n, X.head[0], X.head[1]);
        span_rekey(out + 16, P.src_origin + P.end, P.tail_n, X.tail[0], X.tail[1]);
    };
    // The filtered sum the shared scaffold adds up is never above the unfiltered one: where that fits, the scaffold's own verdict (a bad
    // entry) and naming hold; where it does not, the call is refused here and the entry named by the unfiltered count.
    if (fits) {
        finish(a, room, entry);
    } else {
        a->hdr->total = 0;
        for (uint64_t i = 0; i < a->n; ++i) entry(i, a->plan[i], false);
    }
}
} // namespace

hipError_t modgpu_launch_rekey_relayout_plan(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream)
{
    MoveTableArgs s = a;
    s.sweep = sweep;
    return enqueue<MoveTableArgs, run_plan, g_relayout_launches, 0>(s, stream);
}
hipError_t modgpu_launch_rekey_relayout_finish(const MoveTableArgs &a, uint32_t sweep, hipStream_t stream)
{
    MoveTableArgs s = a;
    s.sweep = sweep;
    return enqueue<MoveTableArgs, run_finish, g_relayout_launches, 1>(s, stream);
}

extern "C" unsigned long long modgpu_shim_relayout_launches(int kind) { return count(g_relayout_launches, kind); }
