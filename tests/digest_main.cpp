// digest_main.cpp -- modgpu_digest_device / modgpu_digest_batch_device on the CPU stand-in of the HIP runtime, as a program of its own
// (built by `make digest-main` from the library's host sources with ASan + UBSan, run directly by tests/test_digest_cpu.py).
// Every case runs in one arena of stand-in device memory and compares EVERY byte of the arena's span and EVERY record with a model
// computed here from lcg.h and the closed form of Adler-32 (A = 1 + sum of bytes, B = n + n * S1 - S2, both mod 65521, checked against
// the textbook running-sum definition below) -- not from the device code or the stand-in's.  Then every refusal the host makes before
// anything is queued, with its text.  One line per case; exit status 0 = all of it held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lcg.h"
#include "modgpu.h"
#include "modgpu_testing.h"

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
unsigned long long modgpu_shim_digest_launches(int form);
unsigned long long modgpu_shim_digest_stored(void);
unsigned long long modgpu_shim_digest_plan_errors(void);
unsigned long long modgpu_shim_to_launches(int form);
}

namespace {
constexpr uint64_t CHUNK = 65536, P = 65521;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
const uint64_t EDGE_SIZES[] = {0, 1, 15, 16, 17, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5};
const uint64_t PHASES[] = {0, 1, 15, 65520 + 15};
const int32_t KEYS[] = {PS4, PS3, 1, -1, INT32_MIN, 12345};
const int32_t ZERO_KEYS[] = {0, 0x7FFFFFFF, (int32_t)0x80000001};
const uint64_t OFFSETS[] = {0, (1ull << 32) - 17, (1ull << 32) + 5, (1ull << 63) - 9, (1ull << 63) + 11, ~0ull - 2};
constexpr uint64_t ARENA = 12 * CHUNK;
constexpr uint64_t N_RES = 20; // the largest batch's 19 records and the one behind them
int g_failed = 0, g_cases = 0;
uint8_t *g_base = nullptr; // chunk-aligned start of the arena
modgpu_digest_result_t *g_res = nullptr;
std::vector<uint8_t> g_orig, g_want;

uint64_t launches()
{
    modgpu_path_stats_t st;
    modgpu_path_stats(&st, 0);
    return st.gpu_launches;
}

// the model: out = src ^ keystream from lcg.h, byte by byte
std::vector<uint8_t> model_out(const uint8_t *src, uint64_t n, int32_t key, uint64_t off)
{
    std::vector<uint8_t> out(src, src + n);
    const uint32_t kr = lcg::key_residue(key);
    if (!kr) return out;
    uint32_t s = lcg::state_residue(kr, off % lcg::PERIOD);
    for (uint64_t i = 0; i < n; ++i) {
        out[i] ^= (uint8_t)~s;
        s = lcg::mulmod(s, lcg::A);
    }
    return out;
}
// Adler-32 as it is defined: two running sums
uint32_t adler_running(const std::vector<uint8_t> &d)
{
    uint64_t a = 1, b = 0;
    for (uint8_t x : d) {
        a = (a + x) % P;
        b = (b + a) % P;
    }
    return (uint32_t)(b << 16 | a);
}
// ... and the residues the record must carry: S1 = sum of bytes, S2 = sum of j * byte_j
void model_sums(const std::vector<uint8_t> &d, uint64_t &s1, uint64_t &s2)
{
    s1 = s2 = 0;
    for (uint64_t j = 0; j < d.size(); ++j) {
        s1 = (s1 + d[j]) % P;
        s2 = (s2 + (j % P) * d[j]) % P;
    }
}

struct Entry {
    uint64_t dst; // arena offset, or ~0: digest only
    uint64_t src, n, off;
};
constexpr uint64_t NONE = ~0ull;

bool record_ok(const modgpu_digest_result_t &r, const std::vector<uint8_t> &out)
{
    uint64_t s1, s2;
    model_sums(out, s1, s2);
    return r.s1 % P == s1 && r.s2 % P == s2 && r.n == out.size() && r.reserved == 0 && modgpu_digest_adler32(&r) == adler_running(out);
}

// one call (single when es.size() == 1 and !batch) over entries of the arena; compares the arena's `span` bytes and every record
void run_case(const std::vector<Entry> &es, int32_t key, bool batch, uint64_t span, const char *what)
{
    const int n = (int)es.size();
    std::memcpy(g_base, g_orig.data(), span);
    std::memcpy(g_want.data(), g_orig.data(), span);
    std::vector<std::vector<uint8_t>> outs;
    int nonempty = 0;
    for (const Entry &e : es) {
        outs.push_back(model_out(g_orig.data() + e.src, e.n, key, e.off));
        if (e.dst != NONE && e.n) std::memcpy(g_want.data() + e.dst, outs.back().data(), e.n);
        nonempty += e.n ? 1 : 0;
    }
    std::memset(g_res, 0xA5, sizeof(modgpu_digest_result_t) * (n + 1)); // the call zeroes its records itself; the one behind them stays
    const uint64_t before = launches();
    int rc;
    if (!batch) {
        const Entry &e = es[0];
        rc = modgpu_digest_device(e.dst == NONE ? nullptr : g_base + e.dst, g_base + e.src, e.n, key, e.off, g_res, -1, nullptr);
    } else {
        std::vector<void *> d(n);
        std::vector<const void *> s(n);
        std::vector<uint64_t> z(n), o(n);
        bool any_dst = false;
        for (int i = 0; i < n; ++i) {
            d[i] = es[i].dst == NONE ? nullptr : g_base + es[i].dst;
            any_dst = any_dst || d[i];
            s[i] = es[i].n ? g_base + es[i].src : nullptr; // (an empty entry's pointers are not looked at)
            z[i] = es[i].n;
            o[i] = es[i].off;
        }
        rc = modgpu_digest_batch_device(any_dst ? d.data() : nullptr, s.data(), z.data(), o.data(), n, key, g_res, -1, nullptr);
    }
    bool ok = rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK;
    const bool same = std::memcmp(g_base, g_want.data(), span) == 0;
    std::vector<modgpu_digest_result_t> host(n + 1);
    std::vector<uint32_t> adler(n + 1);
    ok = ok && modgpu_digest_results(g_res, (uint64_t)n, -1, host.data(), adler.data()) == MODGPU_OK;
    bool records = true;
    for (int i = 0; i < n && ok; ++i) records = records && record_ok(g_res[i], outs[i]) && std::memcmp(&host[i], &g_res[i], sizeof host[i]) == 0 && adler[i] == adler_running(outs[i]);
    const uint8_t *behind = reinterpret_cast<const uint8_t *>(g_res + n);
    records = records && std::all_of(behind, behind + sizeof(modgpu_digest_result_t), [](uint8_t b) { return b == 0xA5; });
    const bool counted = launches() - before == (uint64_t)((nonempty + 15) / 16);
    modgpu_launch_info_t li{};
    bool reported = true;
    if (nonempty) {
        uint64_t last_bytes = 0; // of the last launch's run of up to 16 non-empty entries
        int k = 0;
        for (const Entry &e : es)
            if (e.n) last_bytes = (k++ % 16 == 0) ? e.n : last_bytes + e.n;
        reported = modgpu_last_launch(&li) == MODGPU_OK && li.variant == 16 && li.bytes == last_bytes && li.grid >= 1 &&
                   std::string(li.source_hash) == modgpu_to_kernel_source_hash();
    }
    ++g_cases;
    const bool pass = ok && same && records && counted && reported;
    if (!pass) ++g_failed;
    std::printf("%s %s entries=%d n0=%llu src0=%llu dst0=%lld key=%d rc=%d%s%s%s%s\n", pass ? "ok  " : "FAIL", what, n, (unsigned long long)es[0].n,
                (unsigned long long)es[0].src, es[0].dst == NONE ? -1ll : (long long)es[0].dst, key, rc, same ? "" : " BYTES", records ? "" : " RECORDS",
                counted ? "" : " LAUNCHES", reported ? "" : " REPORT");
    if (rc != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
}

void refuse(const char *what, int rc, const char *text)
{
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID && std::strstr(modgpu_last_error(), text) != nullptr;
    if (!pass) ++g_failed;
    std::printf("%s refusal: %s rc=%d (%s)\n", pass ? "ok  " : "FAIL", what, rc, modgpu_last_error());
}
} // namespace

int main()
{
    uint8_t *raw = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0));
    g_res = static_cast<modgpu_digest_result_t *>(modgpu_shim_xfer_alloc(N_RES * sizeof(modgpu_digest_result_t), 0));
    if (!raw || !g_res) return 2;
    g_base = raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1));
    g_orig.resize(ARENA);
    g_want.resize(ARENA);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : g_orig) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }

    // the closed form itself, on the model's own sums: pure host arithmetic, with multiples of 65521 added to the words
    for (uint64_t n : {0ull, 1ull, 65521ull, 100003ull}) {
        std::vector<uint8_t> d(g_orig.begin(), g_orig.begin() + n);
        uint64_t s1, s2;
        model_sums(d, s1, s2);
        const modgpu_digest_result_t plain{s1, s2, n, 0}, lifted{s1 + 7 * P, s2 + (1ull << 40) * P, n, 0};
        ++g_cases;
        const bool pass = modgpu_digest_adler32(&plain) == adler_running(d) && modgpu_digest_adler32(&lifted) == adler_running(d) && modgpu_digest_adler32(nullptr) == 1u;
        if (!pass) ++g_failed;
        std::printf("%s closed form n=%llu\n", pass ? "ok  " : "FAIL", (unsigned long long)n);
    }

    // every edge size x source phase, digest only and fused (destination phases 0 / 1 / 3 against the source, and dst == src), keys
    // and offsets in rotation; identity keys on every size
    const uint64_t SRC0 = CHUNK, DST0 = 6 * CHUNK;
    int rot = 0;
    for (uint64_t n : EDGE_SIZES)
        for (uint64_t ph : PHASES) {
            const int32_t key = KEYS[rot % 6];
            const uint64_t off = OFFSETS[rot % 6];
            ++rot;
            const uint64_t src = SRC0 + ph;
            run_case({{NONE, src, n, off}}, key, false, ARENA, "digest-only");
            run_case({{DST0 + (ph + (uint64_t)rot) % 4 + 16 * (rot % 3), src, n, off}}, key, false, ARENA, "fused      ");
            run_case({{src, src, n, off}}, key, false, ARENA, "fused alias");
            const int32_t z = ZERO_KEYS[rot % 3];
            run_case({{NONE, src, n, off}}, z, false, ARENA, "identity   ");
            run_case({{DST0 + 1 + ph % 16, src, n, off}}, z, false, ARENA, "identity fu");
        }

    // batches of 1, 16 and 17 with empty entries, destinations on some and not on others, sources that overlap where nothing is written
    for (int count : {1, 16, 17}) {
        for (int32_t key : {PS4, ZERO_KEYS[1]}) {
            std::vector<Entry> es;
            uint64_t s = CHUNK / 2 + 3, d = 6 * CHUNK + 5;
            for (int i = 0; i < count + 2; ++i) {
                const uint64_t n = i == 1 || i == count + 1 ? 0 : i % 5 == 0 ? 1 : i % 5 == 1 ? 70001 : i % 5 == 2 ? 17 : i % 5 == 3 ? 4099 : 15;
                const bool with_dst = i % 3 != 1;
                es.push_back({with_dst ? d : NONE, s - (with_dst ? 0 : std::min<uint64_t>(s, 9)), n, OFFSETS[i % 6] + i});
                s += n + 7;
                if (with_dst) d += n + 13;
            }
            // (two of the count + 2 entries are empty: 1, 16 and 17 non-empty ones -- one launch, one, two)
            run_case(es, key, true, ARENA, "batch      ");
        }
    }
    run_case({{NONE, 0, 0, 5}, {NONE, 0, 0, 0}}, PS3, true, ARENA, "batch empty");

    // timing entry point: the same call through time_calls
    {
        float ms = -1.f;
        const int rc = modgpu_time_digest_device(nullptr, g_base + 5, 70001, PS3, 9, g_res, -1, nullptr, 2, &ms);
        const std::vector<uint8_t> out = model_out(g_orig.data() + 5, 70001, PS3, 9);
        ++g_cases;
        const bool pass = rc == MODGPU_OK && ms >= 0.f && modgpu_sync(-1, nullptr) == MODGPU_OK && record_ok(g_res[0], out);
        if (!pass) ++g_failed;
        std::printf("%s timed digest rc=%d\n", pass ? "ok  " : "FAIL", rc);
    }

    // refusals, all before anything is queued
    {
        std::memcpy(g_base, g_orig.data(), ARENA);
        uint8_t *s = g_base + CHUNK + 3, *d = g_base + 6 * CHUNK;
        const uint64_t n = 200000, before = launches();
        std::memset(g_res, 0xA5, N_RES * sizeof *g_res);
        refuse("null source", modgpu_digest_device(nullptr, nullptr, n, PS3, 0, g_res, -1, nullptr), "null buffer");
        refuse("null result", modgpu_digest_device(nullptr, s, n, PS3, 0, nullptr, -1, nullptr), "null result");
        refuse("misaligned result", modgpu_digest_device(nullptr, s, n, PS3, 0, reinterpret_cast<modgpu_digest_result_t *>(reinterpret_cast<uint8_t *>(g_res) + 4), -1, nullptr), "not 8-byte aligned");
        modgpu_digest_result_t host_res{};
        refuse("result in host memory", modgpu_digest_device(nullptr, s, n, PS3, 0, &host_res, -1, nullptr), "not device memory");
        refuse("partial overlap, dst above", modgpu_digest_device(s + 1, s, n, PS3, 0, g_res, -1, nullptr), "partly overlaps");
        refuse("partial overlap, dst below", modgpu_digest_device(s - 1, s, n, PS3, 0, g_res, -1, nullptr), "partly overlaps");
        refuse("partial overlap by one byte", modgpu_digest_device(s + n - 1, s, n, PS3, 0, g_res, -1, nullptr), "partly overlaps");
        refuse("2^24 chunks", modgpu_digest_device(nullptr, s, 1ull << 40, PS3, 0, g_res, -1, nullptr), "2^24 chunks");
        refuse("2^24 chunks by the source's phase", modgpu_digest_device(nullptr, s + 14, (1ull << 40) - 16, PS3, 0, g_res, -1, nullptr), "2^24 chunks");
        {
            void *dd[2] = {d, d + 5};
            const void *ss[2] = {s, s + 100};
            const uint64_t zz[2] = {10, 10};
            refuse("two destinations meet", modgpu_digest_batch_device(dd, ss, zz, nullptr, 2, PS3, g_res, -1, nullptr), "meets another entry");
            void *d2[2] = {d, s};
            refuse("a destination meets another entry's source", modgpu_digest_batch_device(d2, ss, zz, nullptr, 2, PS3, g_res, -1, nullptr), "meets another entry");
            void *d3[2] = {nullptr, s};
            const void *s3[2] = {s + 5, d};
            refuse("a destination meets a digest-only entry's source", modgpu_digest_batch_device(d3, s3, zz, nullptr, 2, PS3, g_res, -1, nullptr), "meets another entry");
            const void *s4[2] = {s, nullptr};
            refuse("null source in a batch", modgpu_digest_batch_device(nullptr, s4, zz, nullptr, 2, PS3, g_res, -1, nullptr), "null buffer");
            refuse("negative count", modgpu_digest_batch_device(nullptr, ss, zz, nullptr, -1, PS3, g_res, -1, nullptr), "bad entry list");
            refuse("null sizes", modgpu_digest_batch_device(nullptr, ss, nullptr, nullptr, 2, PS3, g_res, -1, nullptr), "bad entry list");
            refuse("null sources", modgpu_digest_batch_device(nullptr, nullptr, zz, nullptr, 2, PS3, g_res, -1, nullptr), "bad entry list");
            refuse("null results of a batch", modgpu_digest_batch_device(nullptr, ss, zz, nullptr, 2, PS3, nullptr, -1, nullptr), "null result");
        }
        modgpu_digest_result_t out[1];
        refuse("results: null device pointer", modgpu_digest_results(nullptr, 1, -1, out, nullptr), "null results");
        refuse("results: null out pointer", modgpu_digest_results(g_res, 1, -1, nullptr, nullptr), "null results");
        refuse("results: host memory", modgpu_digest_results(&host_res, 1, -1, out, nullptr), "not device memory");
        float ms = 0;
        refuse("timed: partial overlap", modgpu_time_digest_device(s + 1, s, n, PS3, 0, g_res, -1, nullptr, 2, &ms), "partly overlaps");
        ++g_cases;
        const uint8_t *r = reinterpret_cast<const uint8_t *>(g_res);
        const bool quiet = launches() == before && std::memcmp(g_base, g_orig.data(), ARENA) == 0 && std::all_of(r, r + N_RES * sizeof *g_res, [](uint8_t b) { return b == 0xA5; }) &&
                           modgpu_digest_batch_device(nullptr, nullptr, nullptr, nullptr, 0, PS3, nullptr, -1, nullptr) == MODGPU_OK &&
                           modgpu_digest_results(nullptr, 0, -1, nullptr, nullptr) == MODGPU_OK && launches() == before;
        if (!quiet) ++g_failed;
        std::printf("%s refusals queued nothing and wrote nothing; an empty batch does nothing\n", quiet ? "ok  " : "FAIL");
    }

    ++g_cases;
    const bool plans = modgpu_shim_digest_plan_errors() == 0 && modgpu_shim_digest_launches(0) > 0 && modgpu_shim_digest_launches(1) > 0 &&
                       modgpu_shim_digest_stored() > 0 && modgpu_shim_to_launches(0) + modgpu_shim_to_launches(1) == 0;
    if (!plans) ++g_failed;
    std::printf("%s launch plans: %llu plan errors, %llu plain and %llu funnel digest launches, %llu entries stored, %llu out-of-place launches\n", plans ? "ok  " : "FAIL",
                modgpu_shim_digest_plan_errors(), modgpu_shim_digest_launches(0), modgpu_shim_digest_launches(1), modgpu_shim_digest_stored(),
                modgpu_shim_to_launches(0) + modgpu_shim_to_launches(1));
    modgpu_shim_xfer_free(g_res);
    modgpu_shim_xfer_free(raw);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
