// entry_calls_main.cpp -- the entry-list calls that share one host plan (modgpu_cycle_(batch_)device_to, modgpu_rekey_(batch_)device_to,
// modgpu_verify_(batch_)device, modgpu_verify_rekey_(batch_)device) on the CPU stand-in of the HIP runtime, as a program of its own
// (built by `make entry-calls-main` from the library's host sources with ASan + UBSan, run directly by tests/test_entry_calls_cpu.py;
// the digest calls have tests/digest_main.cpp).  Every case runs in one arena of stand-in device memory that starts on a 64 KiB
// boundary and compares EVERY byte of the arena and EVERY result record with a model computed here from lcg.h, byte by byte -- not from
// the device code or the stand-ins'.  Each line also prints what the host's plan led to: the stand-ins' launch counts per form, their
// collisions and plan errors, and the last launch as modgpu_last_launch reports it.  Nothing that depends on the run (addresses,
// times) is printed: the output of one commit is compared byte for byte with another's.  Exit status 0 = all of it held.
#include <hip/hip_runtime.h> // (the stand-in's: shim::enqueue, for the gate that keeps the ring's holder in flight)

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "lcg.h"
#include "modgpu.h"
#include "modgpu_testing.h"

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
int modgpu_shim_stream_create(void **s);
int modgpu_shim_stream_destroy(void *s);
unsigned long long modgpu_shim_launches(int variant);
unsigned long long modgpu_shim_pair_collisions(void);
unsigned long long modgpu_shim_batch_plan_errors(void);
unsigned long long modgpu_shim_to_launches(int form);
unsigned long long modgpu_shim_to_collisions(void);
unsigned long long modgpu_shim_to_plan_errors(void);
unsigned long long modgpu_shim_rekey_launches(int form);
unsigned long long modgpu_shim_rekey_collisions(void);
unsigned long long modgpu_shim_rekey_plan_errors(void);
unsigned long long modgpu_shim_verify_launches(int form);
unsigned long long modgpu_shim_verify_inits(void);
unsigned long long modgpu_shim_verify_plan_errors(void);
unsigned long long modgpu_shim_rekey_verify_launches(int form);
unsigned long long modgpu_shim_rekey_verify_plan_errors(void);
}

namespace {
constexpr uint64_t CHUNK = 65536;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
const uint64_t SIZES[] = {0, 1, 15, 16, 17, 65535, 65536, 65536 + 17, 3 * CHUNK + 77};
const uint64_t ROLE_PHASES[] = {0, 1, 65520 + 15};
const uint64_t SRC_PHASES[] = {0, 3, 4}; // against the role pointer's: a whole dword apart (0, 4) or not (3: the funnel forms)
const int32_t KEYS[] = {PS4, PS3, 1, -1, INT32_MIN, 12345};
const int32_t ZERO_KEYS[] = {0, 0x7FFFFFFF, (int32_t)0x80000001};
const uint64_t OFFSETS[] = {0, (1ull << 32) - 17, (1ull << 32) + 5, (1ull << 63) - 9, (1ull << 63) + 11, ~0ull - 2};
constexpr uint64_t ARENA = 40 * CHUNK, SRC0 = CHUNK, ROLE0 = 20 * CHUNK; // sources in the lower half, destinations / expects in the upper
constexpr uint64_t HOLD = 14 * CHUNK;                                    // the ring's holder: HOLD_N bytes from here to HOLD + HOLD_N
constexpr uint64_t HOLD_N = CHUNK + 17;
constexpr int N_RES = 40;

enum Call { TO, REKEY, VERIFY, VREKEY };
const char *const NAMES[4] = {"cycle to", "rekey", "verify", "verify rekey"};
bool two_keys(Call c) { return c == REKEY || c == VREKEY; }
bool verifies(Call c) { return c == VERIFY || c == VREKEY; }

int g_failed = 0, g_cases = 0;
uint8_t *g_base = nullptr; // the arena, from a 64 KiB boundary
modgpu_verify_result_t *g_res = nullptr;
std::vector<uint8_t> g_orig, g_want;

// queued on the holder's stream ahead of the holder: its launch has drawn the ring's line and cannot sign off before the case is done
std::atomic<bool> g_gate_open{false};
void gate(void *)
{
    while (!g_gate_open.load(std::memory_order_acquire)) std::this_thread::yield();
}

uint64_t launches()
{
    modgpu_path_stats_t st;
    modgpu_path_stats(&st, 0);
    return st.gpu_launches;
}

// what the stand-ins counted: a case prints how much each moved
struct Counts {
    unsigned long long v[19];
    static Counts now()
    {
        Counts c{};
        int k = 0;
        for (int f = 0; f < 2; ++f) c.v[k++] = modgpu_shim_to_launches(f);
        for (int f = 0; f < 2; ++f) c.v[k++] = modgpu_shim_rekey_launches(f);
        for (int f = 0; f < 4; ++f) c.v[k++] = modgpu_shim_verify_launches(f);
        c.v[k++] = modgpu_shim_verify_inits();
        for (int f = 0; f < 2; ++f) c.v[k++] = modgpu_shim_rekey_verify_launches(f);
        for (int f = 0; f < 3; ++f) c.v[k++] = modgpu_shim_launches(f); // the in-place shapes of the routes without a ticket pair
        c.v[k++] = modgpu_shim_to_collisions() + modgpu_shim_rekey_collisions() + modgpu_shim_pair_collisions();
        c.v[k++] = modgpu_shim_to_plan_errors();
        c.v[k++] = modgpu_shim_rekey_plan_errors();
        c.v[k++] = modgpu_shim_verify_plan_errors();
        c.v[k++] = modgpu_shim_rekey_verify_plan_errors() + modgpu_shim_batch_plan_errors();
        return c;
    }
};
std::string plan_text(const Counts &a, const Counts &b)
{
    unsigned long long d[19];
    for (int k = 0; k < 19; ++k) d[k] = b.v[k] - a.v[k];
    char buf[512];
    std::snprintf(buf, sizeof buf, "to=%llu/%llu rekey=%llu/%llu verify=%llu/%llu/%llu/%llu init=%llu rv=%llu/%llu inplace=%llu/%llu/%llu coll=%llu planerr=%llu", d[0],
                  d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], d[13], d[14], d[15] + d[16] + d[17] + d[18]);
    modgpu_launch_info_t li{};
    std::string s = buf;
    if (modgpu_last_launch(&li) == MODGPU_OK && li.kernel) {
        std::snprintf(buf, sizeof buf, " last=[%s v=%d grid=%u block=%u chunk=%u bytes=%llu]", li.kernel, li.variant, li.grid, li.block, li.chunk_bytes,
                      (unsigned long long)li.bytes);
        s += buf;
    }
    return s;
}
bool plan_errors(const Counts &a, const Counts &b) { return b.v[15] + b.v[16] + b.v[17] + b.v[18] != a.v[15] + a.v[16] + a.v[17] + a.v[18]; }

// the model, byte by byte: out[j] = src[j] ^ ks(key_from)[off_from + j] (^ ks(key_to)[off_to + j] for the two-key calls)
std::vector<uint8_t> model_out(Call c, const uint8_t *src, uint64_t n, int32_t kf, uint64_t of, int32_t kt, uint64_t ot)
{
    std::vector<uint8_t> out(src, src + n);
    const uint32_t rf = lcg::key_residue(kf), rt = two_keys(c) ? lcg::key_residue(kt) : 0;
    uint32_t sf = rf ? lcg::state_residue(rf, of % lcg::PERIOD) : 0, st = rt ? lcg::state_residue(rt, ot % lcg::PERIOD) : 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (rf) out[j] ^= (uint8_t)~sf, sf = lcg::mulmod(sf, lcg::A);
        if (rt) out[j] ^= (uint8_t)~st, st = lcg::mulmod(st, lcg::A);
    }
    return out;
}

struct Entry {
    uint64_t role, src, n, of, ot; // arena offsets of the destination / expect and the source
    std::vector<uint64_t> plant;   // (verifying calls) positions in the entry where expect is made wrong
};
enum Offs { GIVEN, NULL_OFFS };

int call_it(Call c, const std::vector<Entry> &es, int32_t kf, int32_t kt, bool batch, Offs offs, int device = -1, void *stream = nullptr,
            modgpu_verify_result_t *res = g_res)
{
    const int n = (int)es.size();
    if (!batch) {
        const Entry &e = es[0];
        switch (c) {
        case TO: return modgpu_cycle_device_to(g_base + e.role, g_base + e.src, e.n, kf, e.of, device, stream);
        case REKEY: return modgpu_rekey_device_to(g_base + e.role, g_base + e.src, e.n, kf, e.of, kt, e.ot, device, stream);
        case VERIFY: return modgpu_verify_device(g_base + e.role, g_base + e.src, e.n, kf, e.of, res, device, stream);
        default: return modgpu_verify_rekey_device(g_base + e.role, g_base + e.src, e.n, kf, e.of, kt, e.ot, res, device, stream);
        }
    }
    std::vector<void *> d(n);
    std::vector<const void *> s(n);
    std::vector<uint64_t> z(n), f(n), t(n);
    for (int i = 0; i < n; ++i) {
        d[i] = es[i].n ? g_base + es[i].role : nullptr; // (an empty entry's pointers are not looked at)
        s[i] = es[i].n ? g_base + es[i].src : nullptr;
        z[i] = es[i].n;
        f[i] = es[i].of;
        t[i] = es[i].ot;
    }
    const uint64_t *pf = offs == NULL_OFFS ? nullptr : f.data(), *pt = offs == NULL_OFFS ? nullptr : t.data();
    switch (c) {
    case TO: return modgpu_cycle_batch_device_to(d.data(), s.data(), z.data(), pf, n, kf, device, stream);
    case REKEY: return modgpu_rekey_batch_device_to(d.data(), s.data(), z.data(), pf, pt, n, kf, kt, device, stream);
    case VERIFY: return modgpu_verify_batch_device(d.data(), s.data(), z.data(), pf, n, kf, res, device, stream);
    default: return modgpu_verify_rekey_batch_device(d.data(), s.data(), z.data(), pf, pt, n, kf, kt, res, device, stream);
    }
}

// one call over entries of the arena; compares the whole arena and, for the verifying calls, every record and the one behind them
void run_case(Call c, std::vector<Entry> es, int32_t kf, int32_t kt, bool batch, Offs offs, const std::string &what, bool hold_ring = false)
{
    const int n = (int)es.size();
    if (offs == NULL_OFFS)
        for (Entry &e : es) e.of = e.ot = 0;
    std::memcpy(g_want.data(), g_orig.data(), ARENA);
    std::vector<modgpu_verify_result_t> want_res(n, modgpu_verify_result_t{0, ~0ull, 0, 0});
    for (int i = 0; i < n; ++i) {
        const Entry &e = es[i];
        std::vector<uint8_t> out = model_out(c, g_orig.data() + e.src, e.n, kf, e.of, kt, e.ot);
        if (verifies(c)) {
            want_res[i].n = e.n;
            for (uint64_t j : e.plant) {
                out[j] ^= 0x40;
                ++want_res[i].mismatches;
                want_res[i].first_mismatch = std::min<uint64_t>(want_res[i].first_mismatch, j);
            }
        }
        if (e.n) std::memcpy(g_want.data() + e.role, out.data(), e.n);
    }
    // the verifying calls read an arena that already holds what they expect; the writing ones start from the original
    std::memcpy(g_base, verifies(c) ? g_want.data() : g_orig.data(), ARENA);
    std::memset(g_res, 0xA5, sizeof(modgpu_verify_result_t) * N_RES);
    void *holder = nullptr;
    if (hold_ring) { // a launch in flight on another stream holds the ring's only line: this call finds no ticket pair
        const std::vector<uint8_t> h = model_out(REKEY, g_orig.data() + HOLD, HOLD_N, PS3, 1, PS4, 2);
        std::memcpy(g_want.data() + HOLD, h.data(), HOLD_N);
        modgpu_debug_set_queue_ring(1);
        g_gate_open.store(false);
        if (modgpu_shim_stream_create(&holder) != 0) std::abort();
        shim::enqueue(static_cast<hipStream_t>(holder), gate, nullptr);
        if (modgpu_rekey_device_to(g_base + HOLD, g_base + HOLD, HOLD_N, PS3, 1, PS4, 2, -1, holder) != MODGPU_OK) std::abort();
    }
    const Counts before = Counts::now();
    const int rc = call_it(c, es, kf, kt, batch, offs);
    bool ok = rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK;
    if (hold_ring) {
        g_gate_open.store(true, std::memory_order_release);
        ok = ok && modgpu_sync(-1, holder) == MODGPU_OK;
        modgpu_debug_set_queue_ring(0);
        modgpu_shim_stream_destroy(holder);
    }
    const Counts after = Counts::now();
    const bool same = std::memcmp(g_base, g_want.data(), ARENA) == 0;
    bool records = true;
    if (verifies(c)) {
        for (int i = 0; i < n; ++i) records = records && std::memcmp(&g_res[i], &want_res[i], sizeof g_res[i]) == 0;
        if (n) {
            std::vector<modgpu_verify_result_t> host(n);
            records = records && modgpu_verify_results(g_res, (uint64_t)n, -1, host.data()) == MODGPU_OK && std::memcmp(host.data(), g_res, sizeof(host[0]) * n) == 0;
        }
    }
    const uint8_t *behind = reinterpret_cast<const uint8_t *>(g_res + (verifies(c) ? n : 0));
    records = records && std::all_of(behind, reinterpret_cast<const uint8_t *>(g_res + N_RES), [](uint8_t b) { return b == 0xA5; });
    const bool planned = !plan_errors(before, after);
    ++g_cases;
    const bool pass = ok && same && records && planned;
    if (!pass) ++g_failed;
    std::printf("%s %s: %s entries=%d rc=%d%s%s%s | %s\n", pass ? "ok  " : "FAIL", NAMES[c], what.c_str(), n, rc, same ? "" : " BYTES", records ? "" : " RECORDS",
                planned ? "" : " PLAN", plan_text(before, after).c_str());
    if (rc != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
}

void refuse(Call c, const char *what, int rc, const char *text, int want_rc = MODGPU_ERR_INVALID)
{
    ++g_cases;
    const bool pass = rc == want_rc && std::strstr(modgpu_last_error(), text) != nullptr;
    if (!pass) ++g_failed;
    std::printf("%s %s: refusal: %s rc=%d (%s)\n", pass ? "ok  " : "FAIL", NAMES[c], what, rc, modgpu_last_error());
}

// a batch of `count` non-empty entries with empty ones interleaved (one at the run boundary: index 16 of the non-empty ones' list)
std::vector<Entry> make_batch(int count, bool equal_offsets_mixed)
{
    std::vector<Entry> es;
    uint64_t s = SRC0 + 3, d = ROLE0 + 5;
    for (int made = 0; made < count; ++made) {
        if (made == 1 || made % 6 == 4 || made == 16) es.push_back({d, s, 0, OFFSETS[made % 6], 7, {}});
        const uint64_t n = made % 5 == 0 ? 1 : made % 5 == 1 ? 70001 : made % 5 == 2 ? 17 : made % 5 == 3 ? 4099 : 15;
        const uint64_t of = OFFSETS[made % 6] + (uint64_t)made;
        // (mixed: every third entry has both streams at one position, literally or a whole period apart)
        const uint64_t ot = !equal_offsets_mixed ? OFFSETS[(made + 2) % 6] + 3 : made % 3 == 0 ? of : made % 3 == 1 ? of % lcg::PERIOD + lcg::PERIOD : of + 1;
        es.push_back({d, s, n, of, ot, {}});
        s += n + 7 + (uint64_t)(made % 4);
        d += n + 13;
    }
    es.push_back({d, s, 0, 1, 2, {}});
    return es;
}
} // namespace

int main()
{
    uint8_t *raw = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0));
    g_res = static_cast<modgpu_verify_result_t *>(modgpu_shim_xfer_alloc(N_RES * sizeof(modgpu_verify_result_t), 0));
    if (!raw || !g_res) return 2;
    g_base = raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1));
    g_orig.resize(ARENA);
    g_want.resize(ARENA);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : g_orig) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }

    for (Call c : {TO, REKEY, VERIFY, VREKEY}) {
        // every size at every phase of the role pointer and of the source against it, single calls, keys and offsets in rotation
        int rot = 0;
        for (uint64_t rp : ROLE_PHASES)
            for (uint64_t sp : SRC_PHASES)
                for (uint64_t n : SIZES) {
                    const int32_t kf = KEYS[rot % 6], kt = KEYS[(rot + 1) % 6];
                    const uint64_t of = OFFSETS[rot % 6], ot = OFFSETS[(rot + 3) % 6];
                    ++rot;
                    char what[96];
                    std::snprintf(what, sizeof what, "size %llu at role phase %llu src phase %llu", (unsigned long long)n, (unsigned long long)rp, (unsigned long long)sp);
                    run_case(c, {{ROLE0 + rp, SRC0 + rp + sp, n, of, ot, {}}}, kf, kt, false, GIVEN, what);
                }
        // in place (dst == src) for the writing calls; an expect that is its own source for the verifying ones, under identity keys
        if (!verifies(c)) run_case(c, {{ROLE0 + 1, ROLE0 + 1, CHUNK + 17, 9, 11, {}}}, PS3, PS4, false, GIVEN, "dst == src");
        else run_case(c, {{ROLE0 + 1, ROLE0 + 1, CHUNK + 17, 9, 11, {}}}, 0, 0, false, GIVEN, "expect == src under identity keys");

        // batches across the run boundary, empty entries interleaved
        for (int count : {1, 16, 17, 33}) {
            run_case(c, make_batch(count, false), PS4, PS3, true, GIVEN, "batch of " + std::to_string(count));
            run_case(c, make_batch(count, false), PS4, PS3, true, NULL_OFFS, "batch of " + std::to_string(count) + " with null offsets");
        }
        run_case(c, {{ROLE0, SRC0, 0, 5, 6, {}}, {ROLE0, SRC0, 0, 0, 0, {}}}, PS3, PS4, true, GIVEN, "empty entries only");
        run_case(c, {}, PS3, PS4, true, GIVEN, "no entries");

        // degenerate keys: == 0 mod m (each key of the two-key calls, and both), equal keys at equal and at unequal offsets in one batch
        for (int32_t z : ZERO_KEYS) {
            run_case(c, make_batch(17, false), z, PS3, true, GIVEN, "key_from == 0 mod m (" + std::to_string(z) + ")");
            if (two_keys(c)) {
                run_case(c, make_batch(17, false), PS4, z, true, GIVEN, "key_to == 0 mod m (" + std::to_string(z) + ")");
                run_case(c, make_batch(17, false), z, ZERO_KEYS[1], true, GIVEN, "both keys == 0 mod m (" + std::to_string(z) + ")");
            }
        }
        if (two_keys(c)) {
            run_case(c, make_batch(33, true), PS3, PS3, true, GIVEN, "equal keys at equal and unequal offsets");
            run_case(c, make_batch(17, true), PS3, (int32_t)((int64_t)PS3 + 0x7FFFFFFF), true, GIVEN, "keys equal mod m at equal and unequal offsets");
            run_case(c, make_batch(17, true), PS3, PS3, true, NULL_OFFS, "equal keys with null offsets");
            run_case(c, {{ROLE0 + 1, SRC0 + 4, CHUNK + 17, 77, 77 + (uint64_t)lcg::PERIOD, {}}}, PS4, PS4, false, GIVEN, "equal keys a period apart, single");
        }

        // the ring exhausted: the routes that need no ticket pair (the verifying calls draw none: the same launches as ever)
        run_case(c, {{ROLE0 + 1, SRC0 + 4, 4099, 3, 4, {}}}, PS3, PS4, false, GIVEN, "ring exhausted, single", true);
        run_case(c, make_batch(17, true), PS3, PS3, true, GIVEN, "ring exhausted, batch of 17", true);
        if (!verifies(c)) run_case(c, {{ROLE0 + 1, ROLE0 + 1, 4099, 3, 4, {}}}, PS3, PS4, false, GIVEN, "ring exhausted, in place", true);

        // planted mismatches: head (15 bytes at role phase 1), body, tail
        if (verifies(c)) {
            const uint64_t n = 3 * CHUNK + 77;
            run_case(c, {{ROLE0 + 1, SRC0 + 4, n, 5, 6, {3}}}, PS3, PS4, false, GIVEN, "planted in the head");
            run_case(c, {{ROLE0 + 1, SRC0 + 4, n, 5, 6, {70000}}}, PS3, PS4, false, GIVEN, "planted in the body");
            run_case(c, {{ROLE0 + 1, SRC0 + 4, n, 5, 6, {n - 1}}}, PS3, PS4, false, GIVEN, "planted in the tail");
            run_case(c, {{ROLE0 + 1, SRC0 + 4, n, 5, 6, {14, 15, CHUNK - 2, CHUNK - 1, 2 * CHUNK, n - 2}}}, PS3, PS4, false, GIVEN, "planted at the edges");
            std::vector<Entry> es = make_batch(17, true);
            for (Entry &e : es)
                if (e.n >= 17) e.plant = {e.n / 2, e.n - 1};
            es[0].plant = {0};
            run_case(c, es, PS3, PS3, true, GIVEN, "planted across a batch of both kinds of entry");
            run_case(c, es, 0, PS3, true, GIVEN, "planted across a batch under one identity key");
        }

        // every refusal, before anything is queued, with its text; where two rules are broken, the one that wins
        {
            std::memcpy(g_base, g_orig.data(), ARENA);
            std::memset(g_res, 0xA5, sizeof(modgpu_verify_result_t) * N_RES);
            const uint64_t before = launches(), n = 200000;
            const Entry good{ROLE0 + 3, SRC0 + 3, n, 1, 2, {}};
            auto single = [&](Entry e, int device = -1) { return call_it(c, {e}, PS3, PS4, false, GIVEN, device); };
            uint8_t *const r0 = g_base + ROLE0 + 3;
            const uint8_t *const s0 = g_base + SRC0 + 3;
            void *dd[2] = {r0, r0 + 500};
            const void *ss[2] = {s0, s0 + 500};
            const uint64_t zz[2] = {10, 10};
            auto batch = [&](void *const *d, const void *const *s, const uint64_t *z, int cnt, modgpu_verify_result_t *res) {
                switch (c) {
                case TO: return modgpu_cycle_batch_device_to(d, s, z, nullptr, cnt, PS3, -1, nullptr);
                case REKEY: return modgpu_rekey_batch_device_to(d, s, z, nullptr, nullptr, cnt, PS3, PS4, -1, nullptr);
                case VERIFY: return modgpu_verify_batch_device(d, s, z, nullptr, cnt, PS3, res, -1, nullptr);
                default: return modgpu_verify_rekey_batch_device(d, s, z, nullptr, nullptr, cnt, PS3, PS4, res, -1, nullptr);
                }
            };
            refuse(c, "negative count", batch(dd, ss, zz, -1, g_res), "bad entry list");
            refuse(c, "null role list", batch(nullptr, ss, zz, 2, g_res), "bad entry list");
            refuse(c, "null source list", batch(dd, nullptr, zz, 2, g_res), "bad entry list");
            refuse(c, "null sizes", batch(dd, ss, nullptr, 2, g_res), "bad entry list");
            {
                void *d1[2] = {r0, nullptr};
                const void *s1[2] = {s0, nullptr};
                refuse(c, "null role pointer in a batch", batch(d1, ss, zz, 2, g_res), "null buffer");
                refuse(c, "null source in a batch", batch(dd, s1, zz, 2, g_res), "null buffer");
            }
            if (!verifies(c)) {
                refuse(c, "partial overlap, dst above", single({SRC0 + 4, SRC0 + 3, n, 0, 0, {}}), "partly overlaps");
                refuse(c, "partial overlap, dst below", single({SRC0 + 2, SRC0 + 3, n, 0, 0, {}}), "partly overlaps");
                refuse(c, "partial overlap by one byte", single({SRC0 + 3 + n - 1, SRC0 + 3, n, 0, 0, {}}), "partly overlaps");
                void *d2[2] = {r0, r0 + 5};
                refuse(c, "two destinations meet", batch(d2, ss, zz, 2, nullptr), "meets another entry");
                void *d3[2] = {r0, const_cast<uint8_t *>(s0)};
                const void *s3[2] = {s0 + 5, r0 + 100};
                refuse(c, "a destination meets another entry's source", batch(d3, s3, zz, 2, nullptr), "meets another entry");
                // two rules broken: the partial overlap of entry 0 is found before the null pointer of entry 1, and before the meeting
                void *d4[2] = {const_cast<uint8_t *>(s0) + 1, nullptr};
                refuse(c, "partial overlap before a later null", batch(d4, ss, zz, 2, nullptr), "partly overlaps");
                void *d5[2] = {nullptr, r0};
                refuse(c, "null before a later partial overlap", batch(d5, ss, zz, 2, nullptr), "null buffer");
                void *d6[2] = {const_cast<uint8_t *>(s0) + 1, const_cast<uint8_t *>(s0) + 3};
                refuse(c, "partial overlap before a meeting", batch(d6, ss, zz, 2, nullptr), "partly overlaps");
                refuse(c, "a device that does not exist", single(good, 99), "", MODGPU_ERR_INVALID);
                refuse(c, "partial overlap before the device", single({SRC0 + 4, SRC0 + 3, n, 0, 0, {}}, 99), "partly overlaps");
            } else {
                modgpu_verify_result_t *const odd = reinterpret_cast<modgpu_verify_result_t *>(reinterpret_cast<uint8_t *>(g_res) + 4);
                modgpu_verify_result_t host_res{};
                refuse(c, "null result", call_it(c, {good}, PS3, PS4, false, GIVEN, -1, nullptr, nullptr), "null result");
                refuse(c, "null results of a batch", batch(dd, ss, zz, 2, nullptr), "null result");
                refuse(c, "misaligned result", call_it(c, {good}, PS3, PS4, false, GIVEN, -1, nullptr, odd), "result not 8-byte aligned");
                refuse(c, "result in host memory", call_it(c, {good}, PS3, PS4, false, GIVEN, -1, nullptr, &host_res), "not device memory");
                refuse(c, "result in host memory under an identity key", call_it(c, {good}, 0, PS4, false, GIVEN, -1, nullptr, &host_res), "not device memory");
                refuse(c, "2^24 chunks", call_it(c, {{ROLE0, SRC0, 1ull << 40, 0, 0, {}}}, PS3, PS4, false, GIVEN), "2^24 chunks of 64 KiB or more (1 TiB)");
                refuse(c, "2^24 chunks by the phase of expect", call_it(c, {{ROLE0 + 14, SRC0, (1ull << 40) - 16, 0, 0, {}}}, PS3, PS4, false, GIVEN), "2^24 chunks");
                refuse(c, "2^41 bytes", call_it(c, {{ROLE0, SRC0, 1ull << 41, 0, 0, {}}}, PS3, PS4, false, GIVEN), "2^24 chunks");
                // two rules broken: the list, then the result (null, then alignment), then the entries in their order
                refuse(c, "bad list before null result", batch(dd, ss, nullptr, 2, nullptr), "bad entry list");
                {
                    void *d1[2] = {nullptr, r0};
                    refuse(c, "null result before a null buffer", batch(d1, ss, zz, 2, nullptr), "null result");
                    const uint64_t big[2] = {10, 1ull << 40};
                    refuse(c, "misaligned result before a null buffer", batch(d1, ss, zz, 2, odd), "result not 8-byte aligned");
                    refuse(c, "null buffer before a later oversized entry", batch(d1, ss, big, 2, g_res), "null buffer");
                    void *d2[2] = {r0, nullptr};
                    const uint64_t big2[2] = {1ull << 40, 10};
                    refuse(c, "oversized entry before a later null buffer", batch(d2, ss, big2, 2, g_res), "2^24 chunks");
                }
                refuse(c, "a device that does not exist", call_it(c, {good}, PS3, PS4, false, GIVEN, 99), "", MODGPU_ERR_INVALID);
                refuse(c, "misaligned result before the device", call_it(c, {good}, PS3, PS4, false, GIVEN, 99, nullptr, odd), "result not 8-byte aligned");
            }
            ++g_cases;
            const uint8_t *r = reinterpret_cast<const uint8_t *>(g_res);
            const bool quiet = launches() == before && std::memcmp(g_base, g_orig.data(), ARENA) == 0 &&
                               std::all_of(r, r + N_RES * sizeof *g_res, [](uint8_t b) { return b == 0xA5; });
            if (!quiet) ++g_failed;
            std::printf("%s %s: refusals queued nothing and wrote nothing\n", quiet ? "ok  " : "FAIL", NAMES[c]);
        }
    }

    ++g_cases;
    const Counts zero{}, all = Counts::now();
    const bool plans = !plan_errors(zero, all) && all.v[14] == 0;
    if (!plans) ++g_failed;
    std::printf("%s launches: %s\n", plans ? "ok  " : "FAIL", plan_text(zero, all).c_str());
    modgpu_shim_xfer_free(g_res);
    modgpu_shim_xfer_free(raw);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
