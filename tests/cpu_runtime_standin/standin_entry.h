// standin_entry.h -- what the six entry stand-ins (standin_launch_{to,rekey,verify,rekey_verify,to_digest,rekey_move}.cpp) have in common,
// once: the chunk geometry of a part, the rule every plan is held to (start[], the lead against the role pointer, the body's 16-byte
// alignment, the start[] tail), the funnel rule, the walk over head, body and tail with their states, the ticket pair and the enqueue
// wrapper.  Each stand-in keeps what is its own: what a byte of a span becomes, its results or records, its counters and accessors.
// A SECOND implementation of the kernels' rules, written from the record types (the *_kernel.h headers the stand-ins include) and lcg.h
// alone: no device code is included here, so that a fault in the kernels' shared code shows as a difference and not twice.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "../../modulate_amd/csrc/cycle_kernel.h" // kCycleBatchMax only
#include "../../modulate_amd/csrc/lcg.h"

namespace standin_entry {
constexpr uint64_t kChunk = 65536;

inline uint64_t at(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// A part on the chunk grid: its body's bytes, its chunks from the chunk origin, and whether the first is cut (then it is the entry's own
// workgroup's, outside the index space)
struct Geom {
    uint64_t body_bytes, n_chunks, first;
};
template <class Part> Geom geom_of(const Part &P) { return {P.end - P.lead, (P.end + kChunk - 1) / kChunk, P.lead != 0 ? 1u : 0u}; }

// The plan's errors by the rule all entry kernels share, `role(P)` being the body pointer the chunk grid lies on: every start[] is the
// chunks before it, the padding included; the lead is the role body's place in its chunk; a body starts on a 16-byte word (an entry
// shorter than its head has an empty body wherever the head ends).  own(p, P, g) adds what only that kernel asks and does the part.
template <class Args, class Role, class Own> unsigned long long for_parts(const Args &b, Role role, Own own)
{
    unsigned long long bad = 0;
    uint64_t total = 0;
    for (uint32_t p = 0; p < b.n_parts; ++p) {
        const auto &P = b.part[p];
        const Geom g = geom_of(P);
        bad += b.start[p] != total || (at(role(P)) & (kChunk - 1)) != P.lead || (g.body_bytes && (at(role(P)) & 15) != 0);
        total += g.n_chunks > g.first ? g.n_chunks - g.first : 0;
        bad += own(p, P, g);
    }
    for (uint32_t p = b.n_parts; p <= (uint32_t)kCycleBatchMax; ++p) bad += b.start[p] != total;
    return bad;
}
// The funnel rule: the plain forms read whole dwords, so a body whose source is not a whole number of dwords from the role needs a funnel form
inline bool needs_funnel(const void *role_body, const void *src_body, uint64_t body_bytes) { return body_bytes && ((at(src_body) - at(role_body)) & 3) != 0; }

// The canonical states of a span's first byte under the part's one keystream (s[1] unused) or two
struct States {
    uint32_t s[2];
};
inline States states(uint32_t one, uint32_t mul) { return {{lcg::mulmod(one, mul), 0u}}; }
inline States states(const uint32_t (&two)[2], uint32_t mul) { return {{lcg::mulmod(two[0], mul), lcg::mulmod(two[1], mul)}}; }
// The three spans of a part: span(at, n, j0, states) with `at` the span's first byte counted from the body pointers and j0 its index in
// the entry.  The body's base state stands at the chunk origin: a^lead steps it forward to the body (`keyed` false: the identity forms,
// whose states are not looked at).
template <class Part, class Span> void for_spans(const Part &P, bool keyed, Span span)
{
    const uint64_t body_bytes = P.end - P.lead;
    span(-(int64_t)P.head_n, (uint64_t)P.head_n, (uint64_t)0, states(P.base_head, 1u));
    span((int64_t)0, body_bytes, (uint64_t)P.head_n, states(P.base_body, keyed ? lcg::powmod(lcg::A, P.lead) : 1u));
    span((int64_t)body_bytes, (uint64_t)P.tail_n, P.head_n + body_bytes, states(P.base_tail, 1u));
}

// A launch lasts a while: overlaps become likely
inline void last_a_while() { std::this_thread::sleep_for(std::chrono::microseconds(200)); }
// The ticket pair, as for the work-queue shape: taken at the start of the launch (false: it was taken already, a collision), cleaned and
// signed off at its end
template <class Args> bool take_pair(Args &b)
{
    uint32_t expect = 0;
    return std::atomic_ref<uint32_t>(b.queue[0]).compare_exchange_strong(expect, 1u);
}
template <class Args> void sign_off_pair(Args &b)
{
    std::atomic_ref<uint32_t>(b.queue[0]).store(0u);
    if (b.queue_done) std::atomic_ref<uint32_t>(*b.queue_done).store(b.queue_seq, std::memory_order_release);
}

// A launch queued on the stream's thread with a copy of its plan: Run(plan, form) there, in stream order
template <class Args> struct Launch {
    Args a;
    int form;
};
template <class Args, void (*Run)(Args &, int)> hipError_t enqueue(const Args &a, int form, hipStream_t stream)
{
    shim::enqueue(
        stream,
        [](void *arg) {
            Launch<Args> *l = static_cast<Launch<Args> *>(arg);
            Run(l->a, l->form);
            delete l;
        },
        new Launch<Args>{a, form});
    return hipSuccess;
}
} // namespace standin_entry
