// digest_table_main.cpp -- modgpu_digest_table_device on the CPU stand-in of the HIP runtime, as a program of its own (built by
// `make digest-table-main` from the library's host sources with ASan + UBSan, run directly by tests/test_digest_table_cpu.py).
// Every case lays a table over one arena of stand-in device memory and compares every record with a model computed here -- the bytes
// modgpu_cycle_scalar_host makes of the entry's source, summed as include/modgpu.h defines the record, and closed with
// modgpu_digest_adler32 against an Adler-32 written out here -- and the arena with what it was: the call reads and never writes it.
// An entry's dst is NULL, garbage, or a real address in turn: it must make no difference.  Then the refusals of the device tier
// (no record written, the status naming the lowest entry), every refusal the host makes before anything is queued with the text it
// reports, and the timing entry point.  One line per case; exit status 0 = all of it held.
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
unsigned long long modgpu_shim_digest_table_launches(int kind);
unsigned long long modgpu_shim_digest_table_plan_errors(void);
unsigned long long modgpu_shim_verify_table_launches(int kind);
}

namespace {
constexpr uint64_t CHUNK = 65536, MOD = 65521;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
const int32_t KEYS[6] = {PS3, PS4, 0, 0x7FFFFFFF, INT_MIN, -1};
const uint64_t OFFS[6] = {0, 1, 77, (1ull << 32) + 1000003, 0x7FFFFFFDull, (5ull << 40) + 3};
const uint64_t SIZES[9] = {0, 1, 15, 16, 17, 65535, 65536, 65537, 2 * CHUNK + 77};
constexpr uint64_t ARENA = 2ull << 20;
constexpr uint64_t MAX_ENTRIES = 4097;
constexpr uint64_t NONE = UINT64_MAX;
const char *const SHORT_WS = "workspace smaller than modgpu_digest_table_workspace_bytes(n_entries)";
int g_failed = 0, g_cases = 0;

uint8_t *g_base = nullptr; // chunk-aligned start of the arena
std::vector<uint8_t> g_orig;
modgpu_table_entry_t *g_table = nullptr;
uint8_t *g_ws = nullptr; // a workspace for the refusals and the timed calls (9 entries)
modgpu_digest_result_t *g_res = nullptr;

struct Dev { // stand-in device memory of exactly n bytes: whatever a launch touches beyond it, ASan reports
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

// dst by turns: NULL, an address nothing is mapped at, an odd address inside the arena
void *any_dst(uint64_t i) { return i % 3 == 0 ? nullptr : i % 3 == 1 ? reinterpret_cast<void *>(0xDEAD0000BEEF0001ull + i) : g_base + (i * 7919) % ARENA; }

modgpu_table_entry_t entry(uint64_t src, uint64_t n, uint64_t i, int c)
{
    modgpu_table_entry_t e{};
    e.dst = any_dst(i + (uint64_t)c);
    e.src = g_base + src;
    e.n = n;
    e.key = KEYS[(i + (uint64_t)c) % 6];
    e.stream_off = OFFS[(i + 2 * (uint64_t)c) % 6];
    return e;
}

uint32_t adler32(const uint8_t *p, uint64_t n)
{
    uint64_t a = 1, b = 0;
    for (uint64_t j = 0; j < n; ++j) {
        a = (a + p[j]) % MOD;
        b = (b + a) % MOD;
    }
    return (uint32_t)(b << 16 | a);
}

// runs table t and compares every record and the arena with the model
void run_table(const std::vector<modgpu_table_entry_t> &t, const std::string &what)
{
    const uint64_t n = t.size();
    bool ok = n <= MAX_ENTRIES;
    std::memcpy(g_base, g_orig.data(), ARENA);
    std::memcpy(static_cast<void *>(g_table), t.data(), n * sizeof t[0]);
    const uint64_t before = launches(), w = modgpu_digest_table_workspace_bytes(n);
    const Dev ws(w), res(n * sizeof(modgpu_digest_result_t)); // the workspace and the records at their exact sizes
    modgpu_digest_result_t *const got = reinterpret_cast<modgpu_digest_result_t *>(res.p);
    std::memset(res.p, 0xA5, n * sizeof *got);
    const int rc = modgpu_digest_table_device(g_table, n, got, ws.p, w, -1, nullptr);
    ok = ok && w != 0 && ws.p && res.p && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 3;
    uint64_t bad = 0;
    ok = ok && modgpu_table_status(ws.p, -1, &bad) == MODGPU_OK && bad == NONE;
    modgpu_launch_info_t info{};
    ok = ok && modgpu_last_launch(&info) == MODGPU_OK && info.variant == 17 && std::strcmp(info.kernel, "shim verify table stream") == 0 && info.block == 1024 &&
         info.chunk_bytes == CHUNK && info.bytes == 0 && info.grid >= 1 && info.main_groups == info.grid && info.source_hash &&
         std::strcmp(info.source_hash, modgpu_verify_table_kernel_source_hash()) == 0;
    const bool same = std::memcmp(g_base, g_orig.data(), ARENA) == 0;
    std::vector<modgpu_digest_result_t> host(n);
    std::vector<uint32_t> adler(n);
    bool results = n == 0 || modgpu_digest_results(got, n, -1, host.data(), adler.data()) == MODGPU_OK;
    uint64_t first_wrong = NONE;
    for (uint64_t i = 0; i < n && results; ++i) {
        const modgpu_table_entry_t &e = t[i];
        std::vector<uint8_t> out(e.n);
        if (e.n) {
            std::memcpy(out.data(), e.src, e.n);
            results = results && modgpu_cycle_scalar_host(out.data(), e.n, e.key, e.stream_off) == MODGPU_OK;
        }
        uint64_t s1 = 0, s2 = 0;
        for (uint64_t j = 0; j < e.n; ++j) {
            s1 += out[j];
            s2 = (s2 + (j % MOD) * out[j]) % MOD;
        }
        const bool one = host[i].s1 % MOD == s1 % MOD && host[i].s2 % MOD == s2 && host[i].n == e.n && host[i].reserved == 0 && adler[i] == adler32(out.data(), e.n) &&
                         modgpu_digest_adler32(&host[i]) == adler[i] && (e.n != 0 || (host[i].s1 == 0 && host[i].s2 == 0 && adler[i] == 1));
        if (!one && first_wrong == NONE) first_wrong = i;
        results = results && one;
    }
    ++g_cases;
    const bool pass = ok && same && results;
    if (!pass) ++g_failed;
    std::printf("%s digest table: %s entries=%llu rc=%d%s%s\n", pass ? "ok  " : "FAIL", what.c_str(), (unsigned long long)n, rc, same ? "" : " BYTES", results ? "" : " RECORDS");
    if (first_wrong != NONE) std::printf("     first wrong record: entry %llu\n", (unsigned long long)first_wrong);
    if (rc != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
}

// the nine sizes, each source at phase p16 mod 16 and p64k mod 64 KiB
std::vector<modgpu_table_entry_t> shapes(uint64_t p16, uint64_t p64k, int c)
{
    std::vector<modgpu_table_entry_t> t;
    uint64_t s = 0;
    for (uint64_t i = 0; i < 9; ++i) {
        s = (s + CHUNK - 1) / CHUNK * CHUNK + p64k + p16;
        t.push_back(entry(s, SIZES[(i + (uint64_t)c) % 9], i, c));
        s += t.back().n;
    }
    return t;
}

// n entries of 16 .. 55 bytes at every phase, with a large one first, last and on either side of the second 1024-entry record
std::vector<modgpu_table_entry_t> table_of(uint64_t n, int c)
{
    std::vector<modgpu_table_entry_t> t;
    uint64_t s = 3;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t size = i == 0 ? 65537 : i == n - 1 ? 2 * CHUNK + 77 : i == 1023 || i == 1024 ? 65536 : 16 + i * 7 % 40;
        t.push_back(entry(s, size, i, c));
        s += size + i % 3;
    }
    return t;
}

// a table the device must refuse whole: no record written, the status naming entry `want`
void refuse_table(const std::vector<modgpu_table_entry_t> &t, uint64_t want, const char *what)
{
    std::memcpy(g_base, g_orig.data(), ARENA);
    std::memcpy(static_cast<void *>(g_table), t.data(), t.size() * sizeof t[0]);
    const uint64_t before = launches(), w = modgpu_digest_table_workspace_bytes(t.size());
    const Dev ws(w), res(t.size() * sizeof(modgpu_digest_result_t));
    modgpu_digest_result_t *const got = reinterpret_cast<modgpu_digest_result_t *>(res.p);
    std::memset(res.p, 0xA5, t.size() * sizeof *got);
    const int rc = modgpu_digest_table_device(g_table, t.size(), got, ws.p, w, -1, nullptr);
    bool ok = ws.p && res.p && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 3;
    uint64_t bad = 0;
    ok = ok && modgpu_table_status(ws.p, -1, &bad) == MODGPU_ERR_INVALID && bad == want;
    ok = ok && std::string(modgpu_last_error()).find("the device refused entry " + std::to_string(want) + " (the call wrote nothing)") != std::string::npos;
    ok = ok && std::memcmp(g_base, g_orig.data(), ARENA) == 0;
    for (size_t i = 0; i < t.size() * sizeof *got; ++i) ok = ok && res.p[i] == 0xA5;
    ++g_cases;
    if (!ok) ++g_failed;
    std::printf("%s digest table: device refusal: %s rc=%d bad=%llu\n", ok ? "ok  " : "FAIL", what, rc, (unsigned long long)bad);
}

// a call the host must refuse before anything is queued, saying `text`
void refuse(const char *what, const char *text, int rc, uint64_t before)
{
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID && launches() == before && std::strstr(modgpu_last_error(), text) != nullptr;
    if (!pass) ++g_failed;
    std::printf("%s digest table: refusal: %s rc=%d\n", pass ? "ok  " : "FAIL", what, rc);
    if (!pass) std::printf("     %s\n", modgpu_last_error());
}
} // namespace

int main()
{
    uint8_t *raw = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0));
    g_table = static_cast<modgpu_table_entry_t *>(modgpu_shim_xfer_alloc(MAX_ENTRIES * sizeof(modgpu_table_entry_t), 0));
    g_res = static_cast<modgpu_digest_result_t *>(modgpu_shim_xfer_alloc(9 * sizeof(modgpu_digest_result_t), 0));
    const uint64_t ws9 = modgpu_digest_table_workspace_bytes(9);
    g_ws = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ws9, 0));
    if (!raw || !g_table || !g_res || !g_ws || !ws9) return 2;
    g_base = raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1));
    g_orig.resize(ARENA);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : g_orig) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }

    // the workspace is the out-of-place table call's, for every n
    {
        bool okw = modgpu_digest_table_workspace_bytes(0) == 0 && modgpu_digest_table_workspace_bytes(MODGPU_TABLE_MAX_ENTRIES + 1ull) == 0;
        for (uint64_t n = 1; n <= MODGPU_TABLE_MAX_ENTRIES; n = n * 3 + 1) okw = okw && modgpu_digest_table_workspace_bytes(n) == modgpu_table_workspace_bytes(n) && modgpu_table_workspace_bytes(n) > 0;
        okw = okw && modgpu_digest_table_workspace_bytes(MODGPU_TABLE_MAX_ENTRIES) == modgpu_table_workspace_bytes(MODGPU_TABLE_MAX_ENTRIES);
        ++g_cases;
        if (!okw) ++g_failed;
        std::printf("%s workspace sizes\n", okw ? "ok  " : "FAIL");
    }

    // (1) every size at every source phase (0, 1, 5, 15 mod 16; 0, 65520 mod 64 KiB); the keys and offsets rotate from case to case
    int c = 0;
    for (uint64_t p64k : {0ull, 65520ull})
        for (uint64_t p16 : {0ull, 1ull, 5ull, 15ull}) run_table(shapes(p16, p64k, c++), "sizes at src phase " + std::to_string(p64k) + "+" + std::to_string(p16));
    // (2) table lengths: one level, two levels, a level edge, a second 1024-entry record, three levels
    for (uint64_t n : {1ull, 16ull, 17ull, 1024ull, 1025ull, 4097ull}) run_table(table_of(n, c++), "length " + std::to_string(n));
    // (3) a table of empty entries only, their sources NULL or not
    {
        std::vector<modgpu_table_entry_t> empty = shapes(15, 0, 4);
        for (size_t i = 0; i < empty.size(); ++i) {
            empty[i].n = 0;
            if (i % 2) empty[i].src = nullptr;
        }
        run_table(empty, "empty entries only");
    }

    // (4) refusals on the device
    {
        const std::vector<modgpu_table_entry_t> good = shapes(1, 0, 5);
        auto with = [&](auto change) {
            std::vector<modgpu_table_entry_t> u = good;
            change(u);
            return u;
        };
        refuse_table(with([](auto &u) { u[8].src = nullptr; }), 8, "a null source");
        refuse_table(with([](auto &u) { u[3].src = nullptr; u[6].flags = 4; }), 3, "a null source, the lowest of two");
        refuse_table(with([](auto &u) { u[7].flags = 1; }), 7, "nonzero flags");
        std::vector<modgpu_table_entry_t> tib = shapes(0, 65520, 5); // (from 65520 mod 64 KiB, 1 TiB lies on 2^24 + 1 chunks)
        tib[0].n = 1ull << 40;
        tib[2].flags = 1;
        refuse_table(tib, 0, "an entry of 1 TiB, the lowest of two");
    }

    // (5) refusals of the host, all before anything is queued, and the timing entry point
    {
        std::memcpy(g_base, g_orig.data(), ARENA);
        const std::vector<modgpu_table_entry_t> good = shapes(1, 0, 5);
        std::memcpy(static_cast<void *>(g_table), good.data(), good.size() * sizeof good[0]);
        const uint64_t n = good.size(), w = ws9, before = launches();
        std::vector<uint64_t> host(w / 8 + 64);
        auto call = [&](const void *t, uint64_t cnt, void *r, void *ws, uint64_t wsb) {
            return modgpu_digest_table_device(static_cast<const modgpu_table_entry_t *>(t), cnt, static_cast<modgpu_digest_result_t *>(r), ws, wsb, -1, nullptr);
        };
        uint8_t *const tb = reinterpret_cast<uint8_t *>(g_table);
        refuse("too many entries", "more than 4194304 entries (the table call's limit)", call(g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull, g_res, g_ws, ~0ull), before);
        refuse("null table", "null table or workspace", call(nullptr, n, g_res, g_ws, w), before);
        refuse("null workspace", "null table or workspace", call(g_table, n, g_res, nullptr, w), before);
        refuse("misaligned table", "table or workspace not 8-byte aligned", call(tb + 4, n, g_res, g_ws, w), before);
        refuse("misaligned workspace", "table or workspace not 8-byte aligned", call(g_table, n, g_res, g_ws + 4, w), before);
        refuse("short workspace", SHORT_WS, call(g_table, n, g_res, g_ws, w - 1), before);
        refuse("table that is not device memory", "the table or the workspace is not device memory of the call's device", call(host.data(), n, g_res, g_ws, w), before);
        refuse("workspace that is not device memory", "the table or the workspace is not device memory of the call's device", call(g_table, n, g_res, host.data(), w), before);
        refuse("null results", "null results", call(g_table, n, nullptr, g_ws, w), before);
        refuse("misaligned results", "results not 8-byte aligned", call(g_table, n, reinterpret_cast<uint8_t *>(g_res) + 4, g_ws, w), before);
        refuse("results that are not device memory", "the results are not device memory of the call's device", call(g_table, n, host.data(), g_ws, w), before);
        uint64_t bad = 0;
        refuse("status of host memory", "the workspace is not device memory of the call's device", modgpu_table_status(host.data(), -1, &bad), before);
        float ms = -1.f;
        refuse("timing without iterations", "bad timing arguments", modgpu_time_digest_table_device(g_table, n, g_res, g_ws, w, -1, nullptr, 0, &ms), before);
        refuse("timing without an out pointer", "bad timing arguments", modgpu_time_digest_table_device(g_table, n, g_res, g_ws, w, -1, nullptr, 2, nullptr), before);
        refuse("timing a call the host refuses", "null table or workspace",
               modgpu_time_digest_table_device(g_table, n, g_res, g_ws, w, -1, nullptr, 2, &ms) == MODGPU_OK ? call(nullptr, n, g_res, g_ws, w) : -1, before + 6);
        ++g_cases;
        const bool quiet = launches() == before + 6 && ms >= 0.f && modgpu_sync(-1, nullptr) == MODGPU_OK && call(nullptr, 0, nullptr, nullptr, 0) == MODGPU_OK && launches() == before + 6 &&
                           std::memcmp(g_base, g_orig.data(), ARENA) == 0;
        if (!quiet) ++g_failed;
        std::printf("%s digest table: refusals queued nothing; two timed calls queued six launches; no entries does nothing\n", quiet ? "ok  " : "FAIL");
    }

    ++g_cases;
    bool plans = modgpu_shim_digest_table_plan_errors() == 0 && modgpu_shim_verify_table_launches(0) == 0; // (never the compare mode's launches)
    for (int l = 0; l < 3; ++l) plans = plans && modgpu_shim_digest_table_launches(l) == modgpu_shim_digest_table_launches(0) && modgpu_shim_digest_table_launches(l) > 0;
    if (!plans) ++g_failed;
    std::printf("%s launches: %llu calls of three launches, %llu plan errors\n", plans ? "ok  " : "FAIL", modgpu_shim_digest_table_launches(0), modgpu_shim_digest_table_plan_errors());
    modgpu_shim_xfer_free(g_ws);
    modgpu_shim_xfer_free(g_res);
    modgpu_shim_xfer_free(g_table);
    modgpu_shim_xfer_free(raw);
    std::printf("%d passed, %d failed\n", g_cases - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
