// digest_check_main.cpp -- modgpu_digest_check_device on the CPU stand-in of the HIP runtime, as a program of its own (built by
// `make digest-check-main` from the library's host sources with ASan + UBSan, run directly by tests/test_digest_check_cpu.py).
// Synthetic records at the lane, wave and workgroup edges of one thread per entry -- s1 and s2 over the whole 64-bit range, n up to
// 2^40 -- against a manifest closed here with 128-bit integers, with nothing, the first entry, the last entry and every entry made bad
// (in the A half and in the B half by turns): the summary, every word of the bitmap, 64 guard bytes on either side of both, and the
// records and the manifest unchanged.  Then the records of the digest table stand-in end to end against Adler-32 written out here, one
// source byte flipped, and the same table refused on the device; every refusal the host makes before anything is queued with the text
// it reports, and the timing entry point.  One line per case; exit status 0 = all of it held.
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
unsigned long long modgpu_shim_digest_check_launches(int kind);
unsigned long long modgpu_shim_digest_check_plan_errors(void);
unsigned long long modgpu_shim_verify_inits(void);
}

namespace {
constexpr uint64_t MOD = 65521, NONE = UINT64_MAX, GUARD = 64;
constexpr uint8_t FILL = 0xA5;
int g_failed = 0, g_cases = 0;

struct Dev { // stand-in device memory of exactly n bytes: whatever a launch touches beyond it, ASan reports
    uint8_t *p;
    explicit Dev(uint64_t n) : p(static_cast<uint8_t *>(modgpu_shim_xfer_alloc(n ? n : 1, 0))) {}
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

uint64_t g_x = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

// the record closed as include/modgpu.h defines it, in integers wide enough for anything
uint32_t close_record(const modgpu_digest_result_t &r)
{
    const unsigned __int128 m = MOD, s1 = r.s1 % m, s2 = r.s2 % m, n = r.n % m;
    return (uint32_t)(((n + n * s1 + m - s2) % m) << 16 | (1 + s1) % m);
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

// The summary and the bitmap of one call, each between 64 guard bytes, all of it filled with a pattern before the call
struct Out {
    uint64_t words;
    Dev mem;
    explicit Out(uint64_t n) : words((n + 63) / 64), mem(3 * GUARD + 32 + 8 * words) { std::memset(mem.p, FILL, 3 * GUARD + 32 + 8 * words); }
    modgpu_digest_check_summary_t *summary() const { return reinterpret_cast<modgpu_digest_check_summary_t *>(mem.p + GUARD); }
    uint64_t *bits() const { return reinterpret_cast<uint64_t *>(mem.p + 2 * GUARD + 32); }
    bool guards() const
    {
        bool ok = true;
        for (uint64_t i = 0; i < GUARD; ++i) ok = ok && mem.p[i] == FILL && mem.p[GUARD + 32 + i] == FILL && mem.p[2 * GUARD + 32 + 8 * words + i] == FILL;
        return ok;
    }
    bool bits_untouched() const
    {
        bool ok = true;
        for (uint64_t i = 0; i < 8 * words; ++i) ok = ok && mem.p[2 * GUARD + 32 + i] == FILL;
        return ok;
    }
};

// what a check over `bad` (one flag per entry) must leave: the summary and every word of the bitmap
bool matches(const Out &o, const std::vector<uint8_t> &bad, bool with_bits)
{
    const uint64_t n = bad.size();
    uint64_t count = 0, first = NONE;
    std::vector<uint64_t> words(o.words, 0);
    for (uint64_t i = 0; i < n; ++i)
        if (bad[i]) {
            ++count;
            if (first == NONE) first = i;
            words[i / 64] |= 1ull << (i % 64);
        }
    modgpu_digest_check_summary_t s{};
    bool ok = modgpu_digest_check_summary(o.summary(), -1, &s) == MODGPU_OK && s.bad_entries == count && s.first_bad_entry == first && s.entries == n && s.refused == 0;
    ok = ok && std::memcmp(o.summary(), &s, sizeof s) == 0 && o.guards();
    if (with_bits) ok = ok && std::memcmp(o.bits(), words.data(), 8 * o.words) == 0;
    else ok = ok && o.bits_untouched();
    return ok;
}

bool last_is_check(uint64_t n)
{
    modgpu_launch_info_t info{};
    return modgpu_last_launch(&info) == MODGPU_OK && info.variant == 19 && std::strcmp(info.kernel, "modgpu_cycle_verify_table_finish") == 0 && info.block == 1024 &&
           info.grid == (n + 1023) / 1024 && info.chunk_bytes == 0 && info.bytes == 0 && info.source_hash &&
           std::strcmp(info.source_hash, modgpu_verify_table_kernel_source_hash()) == 0;
}

// n synthetic records, `plant` = which entries are made bad: 0 none, 1 the first, 2 the last, 3 all
void synthetic(uint64_t n, int plant)
{
    static const uint64_t PLANTED[5] = {0, 65520, 65521, 1ull << 63, UINT64_MAX};
    static const uint64_t NS[7] = {0, 1, 65520, 65521, 65522, (1ull << 32) + 5, (1ull << 40) - 1};
    const Dev rec(n * 32), exp(n * 4);
    std::vector<modgpu_digest_result_t> r(n);
    std::vector<uint32_t> e(n);
    std::vector<uint8_t> bad(n, 0);
    for (uint64_t i = 0; i < n; ++i) {
        r[i].s1 = i % 7 == 3 ? PLANTED[i / 7 % 5] : rnd();
        r[i].s2 = i % 5 == 2 ? PLANTED[i / 5 % 5] : rnd();
        r[i].n = NS[(i + i / 7) % 7];
        r[i].reserved = 0;
        e[i] = close_record(r[i]);
        bad[i] = plant == 3 || (plant == 1 && i == 0) || (plant == 2 && i == n - 1);
        // a bad value differs in ONE half only, the halves by turns; each half stays a residue
        if (bad[i]) e[i] = i % 2 ? (e[i] & 0xFFFFu) | ((e[i] >> 16) + 1) % MOD << 16 : (e[i] & 0xFFFF0000u) | ((e[i] & 0xFFFFu) + 1) % MOD;
    }
    std::memcpy(rec.p, r.data(), n * 32);
    std::memcpy(exp.p, e.data(), n * 4);
    const modgpu_digest_result_t *const records = reinterpret_cast<const modgpu_digest_result_t *>(rec.p);
    const uint32_t *const expect = reinterpret_cast<const uint32_t *>(exp.p);
    bool ok = true;
    for (int with_bits = 1; with_bits >= 0; --with_bits) {
        const Out o(n);
        const uint64_t before = launches();
        const int rc = modgpu_digest_check_device(records, expect, n, nullptr, o.summary(), with_bits ? o.bits() : nullptr, -1, nullptr);
        ok = ok && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 2 && last_is_check(n) && matches(o, bad, with_bits != 0);
    }
    ok = ok && std::memcmp(rec.p, r.data(), n * 32) == 0 && std::memcmp(exp.p, e.data(), n * 4) == 0;
    ++g_cases;
    if (!ok) ++g_failed;
    static const char *const names[4] = {"clean", "first bad", "last bad", "all bad"};
    std::printf("%s digest check: synthetic n=%llu %s\n", ok ? "ok  " : "FAIL", (unsigned long long)n, names[plant]);
    if (!ok) std::printf("     %s\n", modgpu_last_error());
}

// a call the host must refuse before anything is queued, saying `text`
void refuse(const char *what, const char *text, int rc, uint64_t before)
{
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID && launches() == before && std::strstr(modgpu_last_error(), text) != nullptr;
    if (!pass) ++g_failed;
    std::printf("%s digest check: refusal: %s rc=%d\n", pass ? "ok  " : "FAIL", what, rc);
    if (!pass) std::printf("     %s\n", modgpu_last_error());
}
} // namespace

int main()
{
    // (1) synthetic records
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull})
        for (int plant = 0; plant < 4; ++plant) synthetic(n, plant);

    // (2) the digest table stand-in's records end to end: clean, one source byte flipped, the table refused on the device
    {
        constexpr uint64_t N = 70, ARENA = 1ull << 20;
        const Dev arena(ARENA), table(N * sizeof(modgpu_table_entry_t)), rec(N * 32), exp(N * 4);
        const uint64_t w = modgpu_digest_table_workspace_bytes(N);
        const Dev ws(w);
        for (uint64_t i = 0; i < ARENA; ++i) arena.p[i] = (uint8_t)(rnd() >> 56);
        std::vector<modgpu_table_entry_t> t(N);
        std::vector<uint32_t> e(N);
        uint64_t at = 3;
        for (uint64_t i = 0; i < N; ++i) {
            const uint64_t size = i == 0 ? 65537 : i == 9 ? 0 : i == N - 1 ? 2 * 65536 + 77 : 1 + i * 37 % 200;
            t[i] = modgpu_table_entry_t{};
            t[i].src = arena.p + at;
            t[i].n = size;
            t[i].key = i % 3 ? (int32_t)0xC64EED30 : 0;
            t[i].stream_off = i * 1000003;
            std::vector<uint8_t> out(arena.p + at, arena.p + at + size);
            if (size) modgpu_cycle_scalar_host(out.data(), size, t[i].key, t[i].stream_off);
            e[i] = adler32(out.data(), size);
            at += size + i % 3;
        }
        std::memcpy(static_cast<void *>(table.p), t.data(), N * sizeof t[0]);
        std::memcpy(exp.p, e.data(), N * 4);
        const modgpu_table_entry_t *const entries = reinterpret_cast<const modgpu_table_entry_t *>(table.p);
        modgpu_digest_result_t *const records = reinterpret_cast<modgpu_digest_result_t *>(rec.p);
        const uint32_t *const expect = reinterpret_cast<const uint32_t *>(exp.p);
        auto run = [&](const std::vector<uint8_t> &bad, const char *what) {
            const Out o(N);
            std::memset(rec.p, FILL, N * 32);
            const uint64_t before = launches();
            bool ok = modgpu_digest_table_device(entries, N, records, ws.p, w, -1, nullptr) == MODGPU_OK &&
                      modgpu_digest_check_device(records, expect, N, ws.p, o.summary(), o.bits(), -1, nullptr) == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK &&
                      launches() - before == 5 && last_is_check(N) && matches(o, bad, true);
            ++g_cases;
            if (!ok) ++g_failed;
            std::printf("%s digest check: digest table records: %s\n", ok ? "ok  " : "FAIL", what);
            if (!ok) std::printf("     %s\n", modgpu_last_error());
        };
        std::vector<uint8_t> bad(N, 0);
        run(bad, "clean");
        for (uint64_t k : {uint64_t(0), uint64_t(33), N - 1}) {
            uint8_t *const byte = const_cast<uint8_t *>(static_cast<const uint8_t *>(t[k].src)) + (k == 0 ? 40000 : 0);
            *byte ^= 0x10;
            bad[k] = 1;
            run(bad, ("a source byte of entry " + std::to_string(k) + " flipped").c_str());
            *byte ^= 0x10;
            bad[k] = 0;
        }
        // refused on the device: the records and the bitmap keep what the caller left there
        {
            t[5].flags = 1;
            std::memcpy(static_cast<void *>(table.p), t.data(), N * sizeof t[0]);
            const Out o(N);
            std::memset(rec.p, FILL, N * 32);
            const uint64_t before = launches();
            bool ok = modgpu_digest_table_device(entries, N, records, ws.p, w, -1, nullptr) == MODGPU_OK &&
                      modgpu_digest_check_device(records, expect, N, ws.p, o.summary(), o.bits(), -1, nullptr) == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK &&
                      launches() - before == 5;
            modgpu_digest_check_summary_t s{};
            ok = ok && modgpu_digest_check_summary(o.summary(), -1, &s) == MODGPU_ERR_INVALID && std::strstr(modgpu_last_error(), "the table call that produced the records was refused") != nullptr;
            ok = ok && s.bad_entries == 0 && s.first_bad_entry == NONE && s.entries == N && s.refused == 1 && o.guards() && o.bits_untouched();
            for (uint64_t i = 0; i < N * 32; ++i) ok = ok && rec.p[i] == FILL;
            // ... and without the workspace the same records are taken as they are: the pattern closes to no entry's value
            const Out o2(N);
            ok = ok && modgpu_digest_check_device(records, expect, N, nullptr, o2.summary(), o2.bits(), -1, nullptr) == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK &&
                 matches(o2, std::vector<uint8_t>(N, 1), true);
            ++g_cases;
            if (!ok) ++g_failed;
            std::printf("%s digest check: refused producer\n", ok ? "ok  " : "FAIL");
            t[5].flags = 0;
        }

        // (3) refusals of the host, all before anything is queued, and the timing entry point
        const Out o(N);
        std::vector<uint64_t> host(N * 4 + 64);
        modgpu_digest_check_summary_t *const sum = o.summary();
        uint64_t *const bits = o.bits();
        const uint64_t before = launches();
        auto call = [&](const void *r, const void *x, uint64_t cnt, const void *tw, void *s, void *b) {
            return modgpu_digest_check_device(static_cast<const modgpu_digest_result_t *>(r), static_cast<const uint32_t *>(x), cnt, tw,
                                              static_cast<modgpu_digest_check_summary_t *>(s), static_cast<uint64_t *>(b), -1, nullptr);
        };
        const char *const FOREIGN = "the records, the manifest, the summary or the bits are not device memory of the call's device";
        const char *const MEET = "the summary or the bits overlap the records, the manifest or each other";
        refuse("too many entries", "more entries than a table call takes (4194304)", call(records, expect, MODGPU_TABLE_MAX_ENTRIES + 1ull, ws.p, sum, bits), before);
        refuse("null records", "null records, manifest or summary", call(nullptr, expect, N, ws.p, sum, bits), before);
        refuse("null manifest", "null records, manifest or summary", call(records, nullptr, N, ws.p, sum, bits), before);
        refuse("null summary", "null records, manifest or summary", call(records, expect, N, ws.p, nullptr, bits), before);
        refuse("misaligned records", "records, summary or bits not 8-byte aligned", call(rec.p + 4, expect, N - 1, ws.p, sum, bits), before);
        refuse("misaligned summary", "records, summary or bits not 8-byte aligned", call(records, expect, N, ws.p, o.mem.p + GUARD + 4, bits), before);
        refuse("misaligned bits", "records, summary or bits not 8-byte aligned", call(records, expect, N, ws.p, sum, reinterpret_cast<uint8_t *>(bits) + 4), before);
        refuse("misaligned manifest", "manifest not 4-byte aligned", call(records, exp.p + 2, N - 1, ws.p, sum, bits), before);
        refuse("misaligned table workspace", "table workspace not 8-byte aligned", call(records, expect, N, ws.p + 4, sum, bits), before);
        refuse("summary inside the records", MEET, call(records, expect, N, ws.p, rec.p + 64, bits), before);
        refuse("summary inside the manifest", MEET, call(records, expect, N, ws.p, exp.p + 8, bits), before);
        refuse("bits inside the records", MEET, call(records, expect, N, ws.p, sum, rec.p + N * 32 - 8), before);
        refuse("bits inside the manifest", MEET, call(records, expect, N, ws.p, sum, exp.p), before);
        refuse("bits over the summary", MEET, call(records, expect, N, ws.p, sum, reinterpret_cast<uint8_t *>(sum) + 24), before);
        refuse("records that are not device memory", FOREIGN, call(host.data(), expect, N, ws.p, sum, bits), before);
        refuse("manifest that is not device memory", FOREIGN, call(records, host.data(), N, ws.p, sum, bits), before);
        refuse("summary that is not device memory", FOREIGN, call(records, expect, N, ws.p, host.data(), bits), before);
        refuse("bits that are not device memory", FOREIGN, call(records, expect, N, ws.p, sum, host.data()), before);
        refuse("table workspace that is not device memory", "the table workspace is not device memory of the call's device", call(records, expect, N, host.data(), sum, bits), before);
        modgpu_digest_check_summary_t s{};
        refuse("summary read from a null pointer", "null summary or out pointer", modgpu_digest_check_summary(nullptr, -1, &s), before);
        refuse("summary read without an out pointer", "null summary or out pointer", modgpu_digest_check_summary(sum, -1, nullptr), before);
        refuse("summary read from host memory", "the summary is not device memory of the call's device",
               modgpu_digest_check_summary(reinterpret_cast<modgpu_digest_check_summary_t *>(host.data()), -1, &s), before);
        float ms = -1.f;
        refuse("timing without iterations", "bad timing arguments", modgpu_time_digest_check_device(records, expect, N, nullptr, sum, bits, -1, nullptr, 0, &ms), before);
        refuse("timing without an out pointer", "bad timing arguments", modgpu_time_digest_check_device(records, expect, N, nullptr, sum, bits, -1, nullptr, 2, nullptr), before);
        ++g_cases;
        bool quiet = o.guards() && o.bits_untouched();
        for (uint64_t i = 0; i < 32; ++i) quiet = quiet && reinterpret_cast<uint8_t *>(sum)[i] == FILL;
        quiet = quiet && call(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == MODGPU_OK && call(records, expect, 0, ws.p, sum, bits) == MODGPU_OK && launches() == before;
        for (uint64_t i = 0; i < 32; ++i) quiet = quiet && reinterpret_cast<uint8_t *>(sum)[i] == FILL;
        quiet = quiet && modgpu_time_digest_check_device(records, expect, N, nullptr, sum, bits, -1, nullptr, 3, &ms) == MODGPU_OK && ms >= 0.f && launches() == before + 6 &&
                modgpu_sync(-1, nullptr) == MODGPU_OK;
        if (!quiet) ++g_failed;
        std::printf("%s digest check: refusals queued nothing; no entries does nothing; three timed calls queued six launches\n", quiet ? "ok  " : "FAIL");
    }

    {
        bool okb = modgpu_digest_check_bits_bytes(0) == 0 && modgpu_digest_check_bits_bytes(1) == 8 && modgpu_digest_check_bits_bytes(64) == 8 &&
                   modgpu_digest_check_bits_bytes(65) == 16 && modgpu_digest_check_bits_bytes(MODGPU_TABLE_MAX_ENTRIES) == MODGPU_TABLE_MAX_ENTRIES / 8 &&
                   modgpu_digest_check_bits_bytes(MODGPU_TABLE_MAX_ENTRIES + 1ull) == 0;
        ++g_cases;
        if (!okb) ++g_failed;
        std::printf("%s bitmap sizes\n", okb ? "ok  " : "FAIL");
    }
    ++g_cases;
    const unsigned long long ran = modgpu_shim_digest_check_launches(0), refused = modgpu_shim_digest_check_launches(1);
    const bool plans = modgpu_shim_digest_check_plan_errors() == 0 && ran > 0 && refused == 1 && modgpu_shim_verify_inits() == ran + refused;
    if (!plans) ++g_failed;
    std::printf("%s launches: %llu checks that compared, %llu behind a refused producer, one init launch each, %llu plan errors\n", plans ? "ok  " : "FAIL", ran, refused,
                modgpu_shim_digest_check_plan_errors());
    std::printf("%d passed, %d failed\n", g_cases - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
