// table_calls_main.cpp -- the four three-launch table calls (modgpu_cycle_table_device, modgpu_rekey_table_device,
// modgpu_verify_table_device, modgpu_verify_rekey_table_device) on the CPU stand-in of the HIP runtime, as a program of its own (built by
// `make table-calls-main` from the library's host sources with ASan + UBSan, run directly by tests/test_table_calls_cpu.py).
// Every case lays a table over one arena of stand-in device memory -- destinations (or comparands) in its first part, sources in its
// second -- and compares EVERY byte of the arena, and every result record, with a model computed here from modgpu_cycle_scalar_host:
// the writing calls must leave the arena as it was with each entry's source, both keystreams XORed in, at its destination; the verifying
// calls must leave it untouched and count and locate exactly the bytes this program flipped in the comparands (an entry's first and last
// byte, its body's first and last byte: head, tail, first and last chunk), in each entry's result and in the summary.  Then the refusals
// of the device tier (nothing written, the status naming the lowest entry, the results untouched), every refusal the host makes before
// anything is queued with the text it reports, and the timing entry points.  One line per case; exit status 0 = all of it held.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "modgpu.h"
#include "modgpu_testing.h"

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
unsigned long long modgpu_shim_table_launches(int kind);
unsigned long long modgpu_shim_rekey_table_launches(int kind);
unsigned long long modgpu_shim_verify_table_launches(int kind);
unsigned long long modgpu_shim_rekey_verify_table_launches(int kind);
}

namespace {
constexpr uint64_t CHUNK = 65536;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
const int32_t KEYS[6] = {PS3, PS4, 0, 0x7FFFFFFF, INT_MIN, -1};
const uint64_t OFFS[6] = {0, 1, 77, (1ull << 32) + 1000003, 0x7FFFFFFDull, (5ull << 40) + 3};
const uint64_t SIZES[9] = {0, 1, 15, 16, 17, 65535, 65536, 65537, 2 * CHUNK + 77};
constexpr uint64_t DST_BYTES = 2ull << 20, SRC_BYTES = 1ull << 20, ARENA = DST_BYTES + SRC_BYTES; // sources start at DST_BYTES
constexpr uint64_t MAX_ENTRIES = 4097;
constexpr uint64_t NONE = UINT64_MAX;
int g_failed = 0, g_cases = 0;

enum Kind { CYCLE, REKEY, VERIFY, VERIFY_REKEY };
struct Call {
    const char *name;
    bool two, verify; // two keystreams; results instead of destinations
    int variant;
    const char *kernel, *short_ws;
    unsigned long long (*shim_launches)(int);
};
const Call CALLS[4] = {
    {"cycle table", false, false, 8, "shim table stream", "workspace smaller than modgpu_table_workspace_bytes(n_entries)", modgpu_shim_table_launches},
    {"rekey table", true, false, 9, "shim rekey table stream", "workspace smaller than modgpu_rekey_table_workspace_bytes(n_entries)", modgpu_shim_rekey_table_launches},
    {"verify table", false, true, 11, "shim verify table stream", "workspace smaller than modgpu_verify_table_workspace_bytes(n_entries)", modgpu_shim_verify_table_launches},
    {"verify rekey table", true, true, 13, "shim rekey verify table stream", "workspace smaller than modgpu_verify_rekey_table_workspace_bytes(n_entries)",
     modgpu_shim_rekey_verify_table_launches},
};

uint8_t *g_base = nullptr; // chunk-aligned start of the arena
std::vector<uint8_t> g_orig, g_want;
uint8_t *g_table = nullptr, *g_ws = nullptr; // MAX_ENTRIES entries of 56 bytes; a workspace for the refusals and the timed calls (9 entries)
modgpu_verify_result_t *g_res = nullptr;
uint64_t g_ws_bytes = 0;

uint64_t ws_bytes(int k, uint64_t n)
{
    return k == CYCLE ? modgpu_table_workspace_bytes(n) : k == REKEY ? modgpu_rekey_table_workspace_bytes(n) : k == VERIFY ? modgpu_verify_table_workspace_bytes(n)
                                                                                                                           : modgpu_verify_rekey_table_workspace_bytes(n);
}
int call(int k, const void *t, uint64_t n, void *res, void *ws, uint64_t wsb)
{
    auto t40 = static_cast<const modgpu_table_entry_t *>(t);
    auto t56 = static_cast<const modgpu_rekey_table_entry_t *>(t);
    auto r = static_cast<modgpu_verify_result_t *>(res);
    return k == CYCLE ? modgpu_cycle_table_device(t40, n, ws, wsb, -1, nullptr) : k == REKEY ? modgpu_rekey_table_device(t56, n, ws, wsb, -1, nullptr)
         : k == VERIFY ? modgpu_verify_table_device(t40, n, r, ws, wsb, -1, nullptr) : modgpu_verify_rekey_table_device(t56, n, r, ws, wsb, -1, nullptr);
}
int time_call(int k, uint64_t n, int iters, float *ms)
{
    const uint64_t w = ws_bytes(k, n);
    return k == CYCLE ? modgpu_time_cycle_table_device(g_table, n, g_ws, w, -1, nullptr, iters, ms) : k == REKEY ? modgpu_time_rekey_table_device(g_table, n, g_ws, w, -1, nullptr, iters, ms)
         : k == VERIFY ? modgpu_time_verify_table_device(g_table, n, g_res, g_ws, w, -1, nullptr, iters, ms) : modgpu_time_verify_rekey_table_device(g_table, n, g_res, g_ws, w, -1, nullptr, iters, ms);
}

// stand-in device memory of exactly n bytes: whatever a launch touches beyond it, ASan reports
struct Dev {
    uint8_t *p;
    explicit Dev(uint64_t n) : p(static_cast<uint8_t *>(modgpu_shim_xfer_alloc(n, 0))) {}
    ~Dev() { modgpu_shim_xfer_free(p); }
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
};

uint64_t launches()
{
    modgpu_path_stats_t st;
    modgpu_path_stats(&st, 0);
    return st.gpu_launches;
}

// one entry in the rekey table's form; the single-keystream calls read key_from / off_from as key / stream_off
typedef modgpu_rekey_table_entry_t Entry;
Entry entry(uint64_t dst, uint64_t src, uint64_t n, int i, int c)
{
    Entry e{};
    e.dst = g_base + dst;
    e.src = g_base + DST_BYTES + src;
    e.n = n;
    const int a = (i + c) % 6;
    e.key_from = KEYS[a];
    e.key_to = KEYS[(a + c) % 6]; // (c a multiple of 6: the same key on both sides)
    e.off_from = OFFS[(i + 2 * c) % 6];
    e.off_to = OFFS[(i + c + 3) % 6];
    return e;
}
void store(int k, const std::vector<Entry> &t)
{
    for (size_t i = 0; i < t.size(); ++i) {
        if (CALLS[k].two) {
            std::memcpy(g_table + i * sizeof(Entry), &t[i], sizeof(Entry));
        } else {
            modgpu_table_entry_t e{t[i].dst, t[i].src, t[i].n, t[i].off_from, t[i].key_from, t[i].flags};
            std::memcpy(g_table + i * sizeof e, &e, sizeof e);
        }
    }
}
uint64_t at(const void *p) { return (uint64_t)(static_cast<const uint8_t *>(p) - g_base); }

// what the call must compute for entry e, from the arena as it was
std::vector<uint8_t> model(int k, const Entry &e, bool &ok)
{
    if (!e.n) return {}; // (an empty entry's pointers may be anything)
    std::vector<uint8_t> out(g_orig.begin() + (ptrdiff_t)at(e.src), g_orig.begin() + (ptrdiff_t)(at(e.src) + e.n));
    ok = ok && modgpu_cycle_scalar_host(out.data(), e.n, e.key_from, e.off_from) == MODGPU_OK;
    if (CALLS[k].two) ok = ok && modgpu_cycle_scalar_host(out.data(), e.n, e.key_to, e.off_to) == MODGPU_OK;
    return out;
}

// runs table t through call k and compares the arena, the results and the summary with the model.  `plant`: for the verifying calls,
// the entries i with (i + plant) % 3 != 0 get their first and last byte and their body's first and last byte flipped (plant < 0: none)
void run_table(int k, const std::vector<Entry> &t, int plant, const std::string &what)
{
    const Call &C = CALLS[k];
    const uint64_t n = t.size();
    std::memcpy(g_want.data(), g_orig.data(), ARENA);
    bool ok = n <= MAX_ENTRIES;
    std::vector<modgpu_verify_result_t> want_res(n);
    modgpu_verify_table_summary_t want_sum{0, NONE, n, 0};
    for (uint64_t i = 0; i < n && ok; ++i) {
        const Entry &e = t[i];
        const std::vector<uint8_t> m = model(k, e, ok);
        if (e.n) std::memcpy(g_want.data() + at(e.dst), m.data(), e.n);
        if (!C.verify) continue;
        std::vector<uint64_t> flips;
        if (plant >= 0 && e.n && (i + (uint64_t)plant) % 3 != 0) {
            const uint64_t d = reinterpret_cast<uintptr_t>(e.dst), head = std::min<uint64_t>(e.n, (16 - (d & 15)) & 15), body = (e.n - head) / 16 * 16;
            flips = {0, e.n - 1};
            if (body) flips.push_back(head), flips.push_back(head + body - 1);
            std::sort(flips.begin(), flips.end());
            flips.erase(std::unique(flips.begin(), flips.end()), flips.end());
            for (uint64_t j : flips) g_want[at(e.dst) + j] ^= (uint8_t)(1u << (j % 8));
        }
        want_res[i] = {flips.size(), flips.empty() ? NONE : flips[0], e.n, 0};
        want_sum.mismatches += flips.size();
        if (!flips.empty() && want_sum.first_bad_entry == NONE) want_sum.first_bad_entry = i;
    }
    // the writing calls start from the arena as it was; the verifying calls from the comparands in place, which they must leave alone
    std::memcpy(g_base, C.verify ? g_want.data() : g_orig.data(), ARENA);
    store(k, t);
    const uint64_t before = launches(), w = ws_bytes(k, n);
    const Dev ws(w), res(n * sizeof(modgpu_verify_result_t)); // the workspace and the results at their exact sizes
    modgpu_verify_result_t *const got = reinterpret_cast<modgpu_verify_result_t *>(res.p);
    std::memset(res.p, 0xA5, n * sizeof *got);
    const int rc = call(k, g_table, n, got, ws.p, w);
    ok = ok && w != 0 && ws.p && res.p && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 3;
    uint64_t bad = 0;
    ok = ok && modgpu_table_status(ws.p, -1, &bad) == MODGPU_OK && bad == NONE;
    modgpu_launch_info_t info{};
    ok = ok && modgpu_last_launch(&info) == MODGPU_OK && info.variant == C.variant && std::strcmp(info.kernel, C.kernel) == 0 && info.block == 1024 && info.chunk_bytes == CHUNK &&
         info.bytes == 0 && info.grid >= 1 && info.main_groups == info.grid && info.source_hash && std::strlen(info.source_hash) == 64;
    const bool same = std::memcmp(g_base, g_want.data(), ARENA) == 0;
    bool results = true;
    if (C.verify) {
        modgpu_verify_table_summary_t sum{};
        results = modgpu_verify_table_summary(ws.p, -1, &sum) == MODGPU_OK && std::memcmp(&sum, &want_sum, sizeof sum) == 0;
        results = results && std::memcmp(static_cast<const void *>(got), want_res.data(), n * sizeof *got) == 0;
    }
    ++g_cases;
    const bool pass = ok && same && results;
    if (!pass) ++g_failed;
    std::printf("%s %s: %s entries=%llu rc=%d%s%s\n", pass ? "ok  " : "FAIL", C.name, what.c_str(), (unsigned long long)n, rc, same ? "" : " BYTES", results ? "" : " RESULTS");
    if (!same) {
        uint64_t first = 0;
        while (g_base[first] == g_want[first]) ++first;
        std::printf("     first differing byte at arena offset %llu\n", (unsigned long long)first);
    }
    if (rc != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
}

// the nine sizes, each destination at phase p16 mod 16 and p64k mod 64 KiB, each source at phase ps mod 4
std::vector<Entry> shapes(uint64_t p16, uint64_t p64k, uint64_t ps, int c)
{
    std::vector<Entry> t;
    uint64_t d = 0, s = 0;
    for (int i = 0; i < 9; ++i) {
        d = (d + CHUNK - 1) / CHUNK * CHUNK + p64k + p16;
        s = (s + 63) / 64 * 64 + ps;
        t.push_back(entry(d, s, SIZES[(i + c) % 9], i, c));
        d += t.back().n;
        s += t.back().n;
    }
    return t;
}

// n entries of 16 .. 55 bytes at every phase, with a large one first, last and on either side of the second 1024-entry record
std::vector<Entry> table_of(uint64_t n, int c)
{
    std::vector<Entry> t;
    uint64_t d = 5, s = 3;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t size = i == 0 ? 65537 : i == n - 1 ? 2 * CHUNK + 77 : i == 1023 || i == 1024 ? 65536 : 16 + i * 7 % 40;
        t.push_back(entry(d, s, size, (int)(i % 6), c));
        d += size + i % 5;
        s += size + i % 3;
    }
    return t;
}

// a table the device must refuse whole: nothing written, the status naming entry `want`, the results untouched
void refuse_table(int k, const std::vector<Entry> &t, uint64_t want, const char *what)
{
    const Call &C = CALLS[k];
    std::memcpy(g_base, g_orig.data(), ARENA);
    store(k, t);
    const uint64_t before = launches(), w = ws_bytes(k, t.size());
    const Dev ws(w), res(t.size() * sizeof(modgpu_verify_result_t));
    modgpu_verify_result_t *const got = reinterpret_cast<modgpu_verify_result_t *>(res.p);
    std::memset(res.p, 0xA5, t.size() * sizeof *got);
    const int rc = call(k, g_table, t.size(), got, ws.p, w);
    bool ok = ws.p && res.p && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 3;
    uint64_t bad = 0;
    ok = ok && modgpu_table_status(ws.p, -1, &bad) == MODGPU_ERR_INVALID && bad == want;
    ok = ok && std::string(modgpu_last_error()).find("the device refused entry " + std::to_string(want) + " (the call wrote nothing)") != std::string::npos;
    modgpu_verify_table_summary_t sum{1, 2, 3, 4};
    if (C.verify)
        ok = ok && modgpu_verify_table_summary(ws.p, -1, &sum) == MODGPU_ERR_INVALID && sum.mismatches == 1 && sum.reserved == 4 &&
             std::string(modgpu_last_error()).find("the device refused entry " + std::to_string(want) + " (the call wrote no result)") != std::string::npos;
    ok = ok && std::memcmp(g_base, g_orig.data(), ARENA) == 0;
    for (size_t i = 0; i < t.size() * sizeof *got; ++i) ok = ok && res.p[i] == 0xA5;
    ++g_cases;
    if (!ok) ++g_failed;
    std::printf("%s %s: device refusal: %s rc=%d bad=%llu\n", ok ? "ok  " : "FAIL", C.name, what, rc, (unsigned long long)bad);
}

// a call the host must refuse before anything is queued, saying `text`
void refuse(int k, const char *what, const char *text, int rc, uint64_t before)
{
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID && launches() == before && std::strstr(modgpu_last_error(), text) != nullptr;
    if (!pass) ++g_failed;
    std::printf("%s %s: refusal: %s rc=%d\n", pass ? "ok  " : "FAIL", CALLS[k].name, what, rc);
    if (!pass) std::printf("     %s\n", modgpu_last_error());
}
} // namespace

int main()
{
    uint8_t *raw = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0));
    g_table = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(MAX_ENTRIES * sizeof(Entry), 0));
    g_res = static_cast<modgpu_verify_result_t *>(modgpu_shim_xfer_alloc(9 * sizeof(modgpu_verify_result_t), 0));
    for (int k = 0; k < 4; ++k) g_ws_bytes = std::max(g_ws_bytes, ws_bytes(k, 9));
    g_ws = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(g_ws_bytes, 0));
    if (!raw || !g_table || !g_res || !g_ws || !g_ws_bytes) return 2;
    g_base = raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1));
    g_orig.resize(ARENA);
    g_want.resize(ARENA);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : g_orig) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }

    // workspace sizes: 0 where documented, whole lines, growing with the table, each call's extra sections on top of the table call's
    {
        bool okw = true;
        for (int k = 0; k < 4; ++k) {
            okw = okw && ws_bytes(k, 0) == 0 && ws_bytes(k, MODGPU_TABLE_MAX_ENTRIES + 1ull) == 0 && ws_bytes(k, MODGPU_TABLE_MAX_ENTRIES) > 0;
            for (uint64_t n = 1; n < MODGPU_TABLE_MAX_ENTRIES; n = n * 3 + 1) okw = okw && ws_bytes(k, n) % 64 == 0 && ws_bytes(k, n * 3 + 1 <= MODGPU_TABLE_MAX_ENTRIES ? n * 3 + 1 : n) >= ws_bytes(k, n);
        }
        for (uint64_t n : {1ull, 17ull, 1025ull, 4097ull})
            okw = okw && ws_bytes(VERIFY, n) == ws_bytes(CYCLE, n) + 64 && ws_bytes(VERIFY_REKEY, n) == ws_bytes(REKEY, n) + 64 && ws_bytes(REKEY, n) == ws_bytes(CYCLE, n) + (n * 16 + 63) / 64 * 64;
        ++g_cases;
        if (!okw) ++g_failed;
        std::printf("%s workspace sizes\n", okw ? "ok  " : "FAIL");
    }

    // (1) every size at every destination phase (0, 1, 15 mod 16; 0, 65520 mod 64 KiB) and source phase (0, 1, 3 mod 4); the keys and
    // offsets rotate through the lists from case to case
    int c = 0;
    for (uint64_t p64k : {0ull, 65520ull})
        for (uint64_t p16 : {0ull, 1ull, 15ull})
            for (uint64_t ps : {0ull, 1ull, 3ull}) {
                for (int k = 0; k < 4; ++k)
                    run_table(k, shapes(p16, p64k, ps, c), c % 3, "sizes at dst phase " + std::to_string(p64k) + "+" + std::to_string(p16) + " src phase " + std::to_string(ps));
                ++c;
            }
    // (2) table lengths: one level, two levels, a level edge, a second 1024-entry record, three levels
    for (uint64_t n : {1ull, 16ull, 17ull, 1024ull, 1025ull, 4097ull})
        for (int k = 0; k < 4; ++k) run_table(k, table_of(n, c++), (int)(n % 3), "length " + std::to_string(n));
    // (3) the verifying calls over comparands that are all as they should be; every call over a table of empty entries only
    for (int k = 0; k < 4; ++k) {
        if (CALLS[k].verify) run_table(k, shapes(1, 65520, 3, 7), -1, "nothing planted");
        std::vector<Entry> empty = shapes(15, 0, 1, 4);
        for (Entry &e : empty) e.n = 0;
        run_table(k, empty, 0, "empty entries only");
    }

    // (4) refusals on the device
    for (int k = 0; k < 4; ++k) {
        const std::vector<Entry> good = shapes(1, 0, 3, 5);
        auto with = [&](auto change) {
            std::vector<Entry> u = good;
            change(u);
            return u;
        };
        refuse_table(k, with([](auto &u) { u[8].src = nullptr; }), 8, "a null source");
        refuse_table(k, with([](auto &u) { u[3].dst = nullptr; u[6].src = nullptr; }), 3, "a null destination, the lowest of two");
        refuse_table(k, with([](auto &u) { u[7].flags = 1; }), 7, "nonzero flags");
        if (CALLS[k].two) refuse_table(k, with([](auto &u) { u[5].reserved = 1u << 31; u[6].flags = 2; }), 5, "nonzero reserved, the lowest of two");
        std::vector<Entry> tib = shapes(0, 65520, 3, 5); // (from 65520 mod 64 KiB, 1 TiB lies on 2^24 + 1 chunks)
        tib[0].n = 1ull << 40;
        tib[2].flags = 1;
        refuse_table(k, tib, 0, "an entry of 1 TiB, the lowest of two");
    }

    // (5) refusals of the host, all before anything is queued, and the timing entry points
    for (int k = 0; k < 4; ++k) {
        const Call &C = CALLS[k];
        std::memcpy(g_base, g_orig.data(), ARENA);
        const std::vector<Entry> good = shapes(1, 0, 3, 5);
        store(k, good);
        const uint64_t n = good.size(), w = ws_bytes(k, n), before = launches();
        std::vector<uint64_t> host(w / 8 + 64);
        refuse(k, "too many entries", "more than 4194304 entries (the table call's limit)", call(k, g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull, g_res, g_ws, ~0ull), before);
        refuse(k, "null table", "null table or workspace", call(k, nullptr, n, g_res, g_ws, w), before);
        refuse(k, "null workspace", "null table or workspace", call(k, g_table, n, g_res, nullptr, w), before);
        refuse(k, "misaligned table", "table or workspace not 8-byte aligned", call(k, g_table + 4, n, g_res, g_ws, w), before);
        refuse(k, "misaligned workspace", "table or workspace not 8-byte aligned", call(k, g_table, n, g_res, g_ws + 4, w), before);
        refuse(k, "short workspace", C.short_ws, call(k, g_table, n, g_res, g_ws, w - 1), before);
        refuse(k, "table that is not device memory", "the table or the workspace is not device memory of the call's device", call(k, host.data(), n, g_res, g_ws, w), before);
        refuse(k, "workspace that is not device memory", "the table or the workspace is not device memory of the call's device", call(k, g_table, n, g_res, host.data(), w), before);
        if (C.verify) {
            refuse(k, "null results", "null results", call(k, g_table, n, nullptr, g_ws, w), before);
            refuse(k, "misaligned results", "results not 8-byte aligned", call(k, g_table, n, reinterpret_cast<uint8_t *>(g_res) + 4, g_ws, w), before);
            refuse(k, "results that are not device memory", "the results are not device memory of the call's device", call(k, g_table, n, host.data(), g_ws, w), before);
            modgpu_verify_table_summary_t sum;
            refuse(k, "summary of a null workspace", "null workspace or out pointer", modgpu_verify_table_summary(nullptr, -1, &sum), before);
            refuse(k, "summary without an out pointer", "null workspace or out pointer", modgpu_verify_table_summary(g_ws, -1, nullptr), before);
            refuse(k, "summary of host memory", "the workspace is not device memory of the call's device", modgpu_verify_table_summary(host.data(), -1, &sum), before);
        }
        uint64_t bad = 0;
        refuse(k, "status of a null workspace", "null workspace or out pointer", modgpu_table_status(nullptr, -1, &bad), before);
        refuse(k, "status without an out pointer", "null workspace or out pointer", modgpu_table_status(g_ws, -1, nullptr), before);
        refuse(k, "status of host memory", "the workspace is not device memory of the call's device", modgpu_table_status(host.data(), -1, &bad), before);
        float ms = -1.f;
        refuse(k, "timing without iterations", "bad timing arguments", time_call(k, n, 0, &ms), before);
        refuse(k, "timing without an out pointer", "bad timing arguments", time_call(k, n, 2, nullptr), before);
        refuse(k, "timing a call the host refuses", "null table or workspace", time_call(k, n, 2, &ms) == MODGPU_OK ? call(k, nullptr, n, g_res, g_ws, w) : -1, before + 6);
        ++g_cases;
        const bool quiet = launches() == before + 6 && ms >= 0.f && modgpu_sync(-1, nullptr) == MODGPU_OK && call(k, nullptr, 0, nullptr, nullptr, 0) == MODGPU_OK && launches() == before + 6 &&
                           (C.verify || std::memcmp(g_base + DST_BYTES, g_orig.data() + DST_BYTES, SRC_BYTES) == 0);
        if (!quiet) ++g_failed;
        std::printf("%s %s: refusals queued nothing; two timed calls queued six launches; no entries does nothing\n", quiet ? "ok  " : "FAIL", C.name);
    }

    ++g_cases;
    bool plans = true;
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 3; ++l) plans = plans && CALLS[k].shim_launches(l) == CALLS[k].shim_launches(0) && CALLS[k].shim_launches(l) > 0;
    if (!plans) ++g_failed;
    std::printf("%s launches: %llu + %llu + %llu + %llu calls of three launches\n", plans ? "ok  " : "FAIL", CALLS[0].shim_launches(0), CALLS[1].shim_launches(0),
                CALLS[2].shim_launches(0), CALLS[3].shim_launches(0));
    modgpu_shim_xfer_free(g_ws);
    modgpu_shim_xfer_free(g_res);
    modgpu_shim_xfer_free(g_table);
    modgpu_shim_xfer_free(raw);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
