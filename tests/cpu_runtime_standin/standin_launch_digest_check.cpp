// standin_launch_digest_check.cpp -- the digest check launch (cycle_verify_table_kernel.h: modgpu_launch_digest_check) on the CPU
// stand-in (hip/hip_runtime.h).  Like the table stand-ins: the launch is queued on the stream's thread and does, from its arguments
// alone, what the verify table TU's finish kernel does in its check mode -- it reads the producer's header, the records and the manifest
// WHEN IT RUNS, closes every record with arithmetic written out here (big enough integers, no device code included), stores every word
// of the bitmap whole where one is given, and adds to and lowers the summary the init launch has made clean, as the kernel's atomics do.
// A refused producer: nothing compared, the summary's n and the refusal stored, the bitmap not touched.  No row of TABLE: the check is a
// mode of the verify table TU's finish kernel, not a TU.
#include "standin_table.h"

#include "../../modulate_amd/csrc/cycle_verify_table_kernel.h"

namespace {
using namespace standin_table;
std::atomic<unsigned long long> g_digest_check_launches[2] = {}, g_digest_check_plan_errors{0}; // [0] compared, [1] found the producer refused

struct CheckLaunch {
    const DigestTableRecord *records;
    const uint32_t *expect;
    uint64_t n;
    const CycleTableHdr *producer;
    CycleVerifyResult *summary;
    unsigned long long *bad_bits;
};

uint32_t close_record(const DigestTableRecord &r)
{
    const unsigned __int128 m = kDigestTableMod;
    const unsigned __int128 s1 = r.s1 % m, s2 = r.s2 % m, n = r.n % m;
    const unsigned __int128 a = (1 + s1) % m, b = (n + n * s1 + m - s2) % m;
    return (uint32_t)(b << 16 | a);
}

void run_check(void *arg)
{
    CheckLaunch *l = static_cast<CheckLaunch *>(arg);
    // the init launch ran before this one, on the same stream
    if (l->summary->mismatches != 0 || l->summary->first_mismatch != kVerifyNone || l->summary->n != 0 || l->summary->reserved != 0) g_digest_check_plan_errors.fetch_add(1);
    if (l->producer && l->producer->first_bad != kTableNoBad) {
        l->summary->n = l->n;
        l->summary->reserved = 1ull;
        g_digest_check_launches[1].fetch_add(1);
        delete l;
        return;
    }
    for (uint64_t w = 0; w * 64 < l->n; ++w) {
        unsigned long long word = 0;
        for (uint64_t b = 0; b < 64 && w * 64 + b < l->n; ++b)
            if (close_record(l->records[w * 64 + b]) != l->expect[w * 64 + b]) word |= 1ull << b;
        if (l->bad_bits) l->bad_bits[w] = word;
        if (word) {
            l->summary->mismatches += (unsigned long long)__builtin_popcountll(word);
            const unsigned long long lowest = w * 64 + (unsigned long long)__builtin_ctzll(word);
            if (lowest < l->summary->first_mismatch) l->summary->first_mismatch = lowest;
        }
    }
    l->summary->n = l->n;
    g_digest_check_launches[0].fetch_add(1);
    delete l;
}
} // namespace

hipError_t modgpu_launch_digest_check(const DigestTableRecord *records, const uint32_t *expect, uint64_t n, const CycleTableHdr *producer,
                                      CycleVerifyResult *summary, unsigned long long *bad_bits, hipStream_t stream)
{
    shim::enqueue(stream, run_check, new CheckLaunch{records, expect, n, producer, summary, bad_bits});
    return hipSuccess;
}

extern "C" unsigned long long modgpu_shim_digest_check_launches(int kind) { return count(g_digest_check_launches, kind); }
extern "C" unsigned long long modgpu_shim_digest_check_plan_errors(void) { return g_digest_check_plan_errors.load(); }
