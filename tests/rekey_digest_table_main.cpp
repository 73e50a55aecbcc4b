// rekey_digest_table_main.cpp -- modgpu_rekey_digest_table_device on the CPU stand-in of the HIP runtime, as a program of its own (built
// by `make rekey-digest-table-main` from the library's host sources with ASan + UBSan, run directly by
// tests/test_rekey_digest_table_cpu.py).  Every case lays a table over two arenas of stand-in device memory -- sources and destinations
// -- and compares with a model written here from lcg.h: every destination byte with src ^ ks(key_from) ^ ks(key_to), every byte next to
// an entry and every source byte with what it was, and every record with the sums of the stored bytes, of the source bytes or of the
// plaintext between the keystreams (the call's side), closed with modgpu_digest_adler32 against the closed form A = 1 + s1,
// B = n + n * s1 - s2 and against an Adler-32 written out here.  Then dst == src, the refusals of the device tier (no byte and no record
// written, the status naming the lowest entry), every refusal the host makes before anything is queued with the text it reports, and
// the timing entry point.  One line per case; exit status 0 = all of it held.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lcg.h"
#include "modgpu.h"
#include "modgpu_testing.h"

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
unsigned long long modgpu_shim_rekey_digest_table_launches(int kind);
unsigned long long modgpu_shim_rekey_digest_table_plan_errors(void);
unsigned long long modgpu_shim_rekey_table_launches(int kind);
}

namespace {
constexpr uint64_t CHUNK = 65536, MOD = 65521;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
// the key pairs: a conversion, one key at two offsets, key_from == 0, key_to == 0 (as 2^31-1), both == 0, one key at offsets equal
// modulo the period (the two keystreams cancel), and two more ordinary ones with negative keys
struct Pair {
    int32_t from, to;
    uint64_t off_from, off_to;
};
const Pair PAIRS[8] = {{PS3, PS4, 0, 0},
                       {PS3, PS3, 77, (1ull << 32) + 1000003},
                       {0, PS4, 1, 0x7FFFFFFDull},
                       {PS4, 0x7FFFFFFF, (5ull << 40) + 3, 9},
                       {0, 0x7FFFFFFF, 5, UINT64_MAX},
                       {PS4, PS4, 1000, 1000 + lcg::PERIOD},
                       {INT_MIN, -1, UINT64_MAX, 1ull << 32},
                       {-1, PS3, lcg::PERIOD - 1, lcg::PERIOD}};
const uint64_t SIZES[11] = {0, 1, 5, 15, 16, 17, 4095, 65535, 65536, 65537, 3 * CHUNK + 5};
const uint32_t SIDES[3] = {MODGPU_DIGEST_OUTPUT, MODGPU_DIGEST_INPUT, MODGPU_DIGEST_PLAIN};
constexpr uint64_t ARENA = 4ull << 20;
constexpr uint64_t MAX_ENTRIES = 1025;
constexpr uint64_t NONE = UINT64_MAX;
const char *const SHORT_WS = "workspace smaller than modgpu_rekey_digest_table_workspace_bytes(n_entries)";
const char *const BAD_SIDE = "side is neither the output side (0), the input side (1) nor the plaintext between the keystreams (2)";
int g_failed = 0, g_cases = 0;

uint8_t *g_src = nullptr, *g_dst = nullptr; // chunk-aligned starts of the two arenas
std::vector<uint8_t> g_src_orig, g_dst_orig;
modgpu_rekey_table_entry_t *g_table = nullptr;
uint8_t *g_ws = nullptr; // a workspace for the refusals and the timed calls (11 entries)
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

void reset_arenas()
{
    std::memcpy(g_src, g_src_orig.data(), ARENA);
    std::memcpy(g_dst, g_dst_orig.data(), ARENA);
}

// the model's keystream: byte j of the stream of `key` from offset `off` is the complement of the low byte of key * a^(off + 1 + j);
// a key == 0 mod 2^31-1 is the identity
void keystream(std::vector<uint8_t> &ks, int32_t key, uint64_t off)
{
    const uint32_t k = lcg::key_residue(key);
    uint32_t s = k ? lcg::mulmod(k, lcg::powmod(lcg::A, (off % lcg::PERIOD + 1) % lcg::PERIOD)) : 0;
    for (auto &b : ks) {
        b = k ? (uint8_t)~s : 0;
        s = lcg::mulmod(s, lcg::A);
    }
}

// an entry from offset s of the source arena to offset d of the destination arena (in_place: of the destination arena, onto itself)
modgpu_rekey_table_entry_t entry(uint64_t d, uint64_t s, uint64_t n, uint64_t pair, bool in_place = false)
{
    const Pair &p = PAIRS[pair % 8];
    modgpu_rekey_table_entry_t e{};
    e.dst = g_dst + d;
    e.src = in_place ? g_dst + d : g_src + s;
    e.n = n;
    e.key_from = p.from;
    e.key_to = p.to;
    e.off_from = p.off_from;
    e.off_to = p.off_to;
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

// runs table t on `side` and compares both arenas and every record with the model
void run_table(const std::vector<modgpu_rekey_table_entry_t> &t, uint32_t side, const std::string &what)
{
    const uint64_t n = t.size();
    bool ok = n <= MAX_ENTRIES;
    reset_arenas();
    // the model first: the arenas as they must be afterwards, and what each record is of
    std::vector<uint8_t> want_dst = g_dst_orig;
    std::vector<std::vector<uint8_t>> summed(n);
    for (uint64_t i = 0; i < n; ++i) {
        const modgpu_rekey_table_entry_t &e = t[i];
        std::vector<uint8_t> in(e.n), plain(e.n), out(e.n), ka(e.n), kb(e.n);
        if (e.n) {
            std::memcpy(in.data(), e.src, e.n);
            keystream(ka, e.key_from, e.off_from);
            keystream(kb, e.key_to, e.off_to);
            for (uint64_t j = 0; j < e.n; ++j) {
                plain[j] = (uint8_t)(in[j] ^ ka[j]);
                out[j] = (uint8_t)(plain[j] ^ kb[j]);
            }
            std::memcpy(want_dst.data() + (static_cast<uint8_t *>(e.dst) - g_dst), out.data(), e.n);
        }
        summed[i] = side == MODGPU_DIGEST_INPUT ? in : side == MODGPU_DIGEST_PLAIN ? plain : out;
    }
    std::memcpy(static_cast<void *>(g_table), t.data(), n * sizeof t[0]);
    const uint64_t before = launches(), w = modgpu_rekey_digest_table_workspace_bytes(n);
    const Dev ws(w), res(n * sizeof(modgpu_digest_result_t)); // the workspace and the records at their exact sizes
    modgpu_digest_result_t *const got = reinterpret_cast<modgpu_digest_result_t *>(res.p);
    std::memset(res.p, 0xA5, n * sizeof *got);
    const int rc = modgpu_rekey_digest_table_device(g_table, n, got, side, ws.p, w, -1, nullptr);
    ok = ok && w != 0 && w == modgpu_rekey_table_workspace_bytes(n) && ws.p && res.p && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 3;
    uint64_t bad = 0;
    ok = ok && modgpu_table_status(ws.p, -1, &bad) == MODGPU_OK && bad == NONE;
    modgpu_launch_info_t info{};
    ok = ok && modgpu_last_launch(&info) == MODGPU_OK && info.variant == 20 && std::strcmp(info.kernel, "shim rekey table stream") == 0 && info.block == 1024 &&
         info.chunk_bytes == CHUNK && info.bytes == 0 && info.grid >= 1 && info.main_groups == info.grid && info.source_hash &&
         std::strcmp(info.source_hash, modgpu_rekey_table_kernel_source_hash()) == 0;
    // with dst == src the "source arena" of the entries is the destination arena, whose bytes the model has rekeyed too
    const bool same = std::memcmp(g_dst, want_dst.data(), ARENA) == 0 && std::memcmp(g_src, g_src_orig.data(), ARENA) == 0;
    std::vector<modgpu_digest_result_t> host(n);
    std::vector<uint32_t> adler(n);
    bool results = n == 0 || modgpu_digest_results(got, n, -1, host.data(), adler.data()) == MODGPU_OK;
    uint64_t first_wrong = NONE;
    for (uint64_t i = 0; i < n && results; ++i) {
        const std::vector<uint8_t> &x = summed[i];
        uint64_t s1 = 0, s2 = 0;
        for (uint64_t j = 0; j < x.size(); ++j) {
            s1 = (s1 + x[j]) % MOD;
            s2 = (s2 + (j % MOD) * x[j]) % MOD;
        }
        const uint64_t nm = x.size() % MOD;
        const uint32_t closed = (uint32_t)(((nm + nm * s1 + MOD - s2) % MOD) << 16 | (1 + s1) % MOD);
        const bool one = host[i].s1 % MOD == s1 && host[i].s2 % MOD == s2 && host[i].n == x.size() && host[i].reserved == 0 && adler[i] == closed &&
                         adler[i] == adler32(x.data(), x.size()) && modgpu_digest_adler32(&host[i]) == adler[i] &&
                         (!x.empty() || (host[i].s1 == 0 && host[i].s2 == 0 && adler[i] == 1));
        if (!one && first_wrong == NONE) first_wrong = i;
        results = results && one;
    }
    ++g_cases;
    const bool pass = ok && same && results;
    if (!pass) ++g_failed;
    std::printf("%s rekey digest table: %s side=%u entries=%llu rc=%d%s%s\n", pass ? "ok  " : "FAIL", what.c_str(), side, (unsigned long long)n, rc, same ? "" : " BYTES",
                results ? "" : " RECORDS");
    if (first_wrong != NONE) std::printf("     first wrong record: entry %llu\n", (unsigned long long)first_wrong);
    if (rc != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
}

// the eleven sizes, each destination at phase `phase` mod 64 KiB and its source `diff` bytes further into its own arena's chunk; the
// key pairs rotate with c
std::vector<modgpu_rekey_table_entry_t> shapes(uint64_t phase, uint64_t diff, int c, bool in_place = false)
{
    std::vector<modgpu_rekey_table_entry_t> t;
    uint64_t d = 0;
    for (uint64_t i = 0; i < 11; ++i) {
        d = (d + CHUNK - 1) / CHUNK * CHUNK + phase;
        t.push_back(entry(d, d + diff, SIZES[(i + (uint64_t)c) % 11], i + 3 * (uint64_t)c, in_place));
        d += t.back().n + diff;
    }
    return t;
}

// n entries of 0 .. 55 bytes at every phase of both sides (every seventh empty), with a large one first, last and on either side of the
// second 1024-entry record
std::vector<modgpu_rekey_table_entry_t> table_of(uint64_t n, int c)
{
    std::vector<modgpu_rekey_table_entry_t> t;
    uint64_t d = 3, s = 1;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t size = i == 0 ? 65537 : i == n - 1 ? 2 * CHUNK + 77 : i == 1023 || i == 1024 ? 65536 : i % 7 == 3 ? 0 : 16 + i * 7 % 40;
        t.push_back(entry(d, s, size, i + (uint64_t)c));
        d += size + i % 3;
        s += size + i % 5;
    }
    return t;
}

// a table the device must refuse whole: no byte and no record written, the status naming entry `want`
void refuse_table(const std::vector<modgpu_rekey_table_entry_t> &t, uint64_t want, const char *what)
{
    reset_arenas();
    std::memcpy(static_cast<void *>(g_table), t.data(), t.size() * sizeof t[0]);
    const uint64_t before = launches(), w = modgpu_rekey_digest_table_workspace_bytes(t.size());
    const Dev ws(w), res(t.size() * sizeof(modgpu_digest_result_t));
    modgpu_digest_result_t *const got = reinterpret_cast<modgpu_digest_result_t *>(res.p);
    std::memset(res.p, 0xA5, t.size() * sizeof *got);
    const int rc = modgpu_rekey_digest_table_device(g_table, t.size(), got, MODGPU_DIGEST_PLAIN, ws.p, w, -1, nullptr);
    bool ok = ws.p && res.p && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 3;
    uint64_t bad = 0;
    ok = ok && modgpu_table_status(ws.p, -1, &bad) == MODGPU_ERR_INVALID && bad == want;
    ok = ok && std::string(modgpu_last_error()).find("the device refused entry " + std::to_string(want) + " (the call wrote nothing)") != std::string::npos;
    ok = ok && std::memcmp(g_dst, g_dst_orig.data(), ARENA) == 0 && std::memcmp(g_src, g_src_orig.data(), ARENA) == 0;
    for (size_t i = 0; i < t.size() * sizeof *got; ++i) ok = ok && res.p[i] == 0xA5;
    ++g_cases;
    if (!ok) ++g_failed;
    std::printf("%s rekey digest table: device refusal: %s rc=%d bad=%llu\n", ok ? "ok  " : "FAIL", what, rc, (unsigned long long)bad);
}

// a call the host must refuse before anything is queued, saying `text`
void refuse(const char *what, const char *text, int rc, uint64_t before)
{
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID && launches() == before && std::strstr(modgpu_last_error(), text) != nullptr;
    if (!pass) ++g_failed;
    std::printf("%s rekey digest table: refusal: %s rc=%d\n", pass ? "ok  " : "FAIL", what, rc);
    if (!pass) std::printf("     %s\n", modgpu_last_error());
}

uint8_t *aligned(uint8_t *raw) { return raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1)); }
} // namespace

int main()
{
    uint8_t *raw_s = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0)), *raw_d = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0));
    g_table = static_cast<modgpu_rekey_table_entry_t *>(modgpu_shim_xfer_alloc(MAX_ENTRIES * sizeof(modgpu_rekey_table_entry_t), 0));
    g_res = static_cast<modgpu_digest_result_t *>(modgpu_shim_xfer_alloc(11 * sizeof(modgpu_digest_result_t), 0));
    const uint64_t ws11 = modgpu_rekey_digest_table_workspace_bytes(11);
    g_ws = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ws11, 0));
    if (!raw_s || !raw_d || !g_table || !g_res || !g_ws || !ws11) return 2;
    g_src = aligned(raw_s);
    g_dst = aligned(raw_d);
    g_src_orig.resize(ARENA);
    g_dst_orig.resize(ARENA);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto *v : {&g_src_orig, &g_dst_orig})
        for (auto &b : *v) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            b = (uint8_t)(x >> 56);
        }

    // the workspace is the rekey table call's, for every n
    {
        bool okw = modgpu_rekey_digest_table_workspace_bytes(0) == 0 && modgpu_rekey_digest_table_workspace_bytes(MODGPU_TABLE_MAX_ENTRIES + 1ull) == 0;
        for (uint64_t n = 1; n <= MODGPU_TABLE_MAX_ENTRIES; n = n * 3 + 1)
            okw = okw && modgpu_rekey_digest_table_workspace_bytes(n) == modgpu_rekey_table_workspace_bytes(n) && modgpu_rekey_table_workspace_bytes(n) > 0;
        okw = okw && modgpu_rekey_digest_table_workspace_bytes(MODGPU_TABLE_MAX_ENTRIES) == modgpu_rekey_table_workspace_bytes(MODGPU_TABLE_MAX_ENTRIES);
        ++g_cases;
        if (!okw) ++g_failed;
        std::printf("%s workspace sizes\n", okw ? "ok  " : "FAIL");
    }

    // (1) every size at every destination phase, the source 0, 1, 3 bytes off it, all three sides; the key pairs rotate from case to
    // case, so that every size meets every pair
    int c = 0;
    for (uint64_t phase : {0ull, 1ull, 15ull, 65520ull + 15ull})
        for (uint64_t diff : {0ull, 1ull, 3ull})
            for (uint32_t side : SIDES) run_table(shapes(phase, diff, c++), side, "sizes at dst phase " + std::to_string(phase) + " src +" + std::to_string(diff));
    // (2) every degenerate key pair over all the sizes, on the plaintext side and the output side
    for (uint64_t pair = 0; pair < 8; ++pair)
        for (uint32_t side : {MODGPU_DIGEST_PLAIN, MODGPU_DIGEST_OUTPUT}) {
            std::vector<modgpu_rekey_table_entry_t> t = shapes(15, 3, 0);
            for (auto &e : t) {
                const modgpu_rekey_table_entry_t k = entry(0, 0, 0, pair);
                e.key_from = k.key_from, e.key_to = k.key_to, e.off_from = k.off_from, e.off_to = k.off_to;
            }
            run_table(t, side, "key pair " + std::to_string(pair));
        }
    // (3) table lengths: one level, two levels, a level edge, a second 1024-entry record; empty entries among them
    for (uint64_t n : {1ull, 16ull, 17ull, 1024ull, 1025ull}) run_table(table_of(n, c), SIDES[c % 3], "length " + std::to_string(n)), ++c;
    // (4) a table of empty entries only, their pointers NULL or not
    for (uint32_t side : SIDES) {
        std::vector<modgpu_rekey_table_entry_t> empty = shapes(15, 1, 4);
        for (size_t i = 0; i < empty.size(); ++i) {
            empty[i].n = 0;
            if (i % 2) empty[i].src = nullptr;
            if (i % 3 == 0) empty[i].dst = nullptr;
        }
        run_table(empty, side, "empty entries only");
    }
    // (5) dst == src: in place; the input side's records are of the bytes as they were
    for (uint32_t side : SIDES)
        for (uint64_t phase : {0ull, 5ull, 65520ull + 15ull}) run_table(shapes(phase, 0, c++, true), side, "dst == src at phase " + std::to_string(phase));

    // (6) refusals on the device
    {
        const std::vector<modgpu_rekey_table_entry_t> good = shapes(1, 3, 5);
        auto with = [&](auto change) {
            std::vector<modgpu_rekey_table_entry_t> u = good;
            change(u);
            return u;
        };
        refuse_table(with([](auto &u) { u[8].src = nullptr; }), 8, "a null source");
        refuse_table(with([](auto &u) { u[5].dst = nullptr; }), 5, "a null destination");
        refuse_table(with([](auto &u) { u[3].src = nullptr; u[6].flags = 4; }), 3, "a null source, the lowest of two");
        refuse_table(with([](auto &u) { u[7].flags = 1; }), 7, "nonzero flags");
        refuse_table(with([](auto &u) { u[9].reserved = 1; }), 9, "nonzero reserved");
        std::vector<modgpu_rekey_table_entry_t> tib = shapes(65520, 0, 5); // (from 65520 mod 64 KiB, 1 TiB lies on 2^24 + 1 chunks)
        tib[0].n = 1ull << 40;
        tib[2].flags = 1;
        refuse_table(tib, 0, "an entry of 1 TiB, the lowest of two");
    }

    // (7) refusals of the host, all before anything is queued, and the timing entry point
    {
        reset_arenas();
        const std::vector<modgpu_rekey_table_entry_t> good = shapes(1, 3, 5);
        std::memcpy(static_cast<void *>(g_table), good.data(), good.size() * sizeof good[0]);
        const uint64_t n = good.size(), w = ws11, before = launches();
        std::vector<uint64_t> host(w / 8 + 64);
        auto call = [&](const void *t, uint64_t cnt, void *r, void *ws, uint64_t wsb, uint32_t side = MODGPU_DIGEST_PLAIN) {
            return modgpu_rekey_digest_table_device(static_cast<const modgpu_rekey_table_entry_t *>(t), cnt, static_cast<modgpu_digest_result_t *>(r), side, ws, wsb, -1, nullptr);
        };
        uint8_t *const tb = reinterpret_cast<uint8_t *>(g_table);
        refuse("a side that is none of the three", BAD_SIDE, call(g_table, n, g_res, g_ws, w, 3u), before);
        refuse("a side that is none of the three, no entries", BAD_SIDE, call(nullptr, 0, nullptr, nullptr, 0, ~0u), before);
        refuse("too many entries", "more than 4194304 entries (the table call's limit)", call(g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull, g_res, g_ws, ~0ull), before);
        refuse("too many entries and null records", "more than 4194304 entries (the table call's limit)", call(g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull, nullptr, g_ws, ~0ull), before);
        refuse("null table", "null table or workspace", call(nullptr, n, g_res, g_ws, w), before);
        refuse("null table and null records", "null table or workspace", call(nullptr, n, nullptr, g_ws, w), before);
        refuse("null workspace", "null table or workspace", call(g_table, n, g_res, nullptr, w), before);
        refuse("misaligned table", "table or workspace not 8-byte aligned", call(tb + 4, n, g_res, g_ws, w), before);
        refuse("misaligned workspace", "table or workspace not 8-byte aligned", call(g_table, n, g_res, g_ws + 4, w), before);
        refuse("short workspace", SHORT_WS, call(g_table, n, g_res, g_ws, w - 1), before);
        refuse("the out-of-place table's workspace size", SHORT_WS, call(g_table, n, g_res, g_ws, modgpu_table_workspace_bytes(n)), before);
        refuse("table that is not device memory", "the table or the workspace is not device memory of the call's device", call(host.data(), n, g_res, g_ws, w), before);
        refuse("workspace that is not device memory", "the table or the workspace is not device memory of the call's device", call(g_table, n, g_res, host.data(), w), before);
        refuse("null results", "null results", call(g_table, n, nullptr, g_ws, w), before);
        refuse("misaligned results", "results not 8-byte aligned", call(g_table, n, reinterpret_cast<uint8_t *>(g_res) + 4, g_ws, w), before);
        refuse("results that are not device memory", "the results are not device memory of the call's device", call(g_table, n, host.data(), g_ws, w), before);
        {
            const Dev cws(modgpu_cycle_digest_table_workspace_bytes(n));
            refuse("the cycle digest table call still refuses side 2", "side is neither the output side (0) nor the input side (1)",
                   modgpu_cycle_digest_table_device(reinterpret_cast<const modgpu_table_entry_t *>(g_table), n, g_res, MODGPU_DIGEST_PLAIN, cws.p,
                                                    modgpu_cycle_digest_table_workspace_bytes(n), -1, nullptr),
                   before);
        }
        float ms = -1.f;
        refuse("timing without iterations", "bad timing arguments", modgpu_time_rekey_digest_table_device(g_table, n, g_res, MODGPU_DIGEST_INPUT, g_ws, w, -1, nullptr, 0, &ms), before);
        refuse("timing without an out pointer", "bad timing arguments", modgpu_time_rekey_digest_table_device(g_table, n, g_res, MODGPU_DIGEST_INPUT, g_ws, w, -1, nullptr, 2, nullptr), before);
        refuse("timing with a side that is none of the three", "side is neither", modgpu_time_rekey_digest_table_device(g_table, n, g_res, 7u, g_ws, w, -1, nullptr, 2, &ms), before);
        const bool untouched = std::memcmp(g_dst, g_dst_orig.data(), ARENA) == 0 && std::memcmp(g_src, g_src_orig.data(), ARENA) == 0;
        refuse("timing a call the host refuses", "null table or workspace",
               modgpu_time_rekey_digest_table_device(g_table, n, g_res, MODGPU_DIGEST_INPUT, g_ws, w, -1, nullptr, 2, &ms) == MODGPU_OK ? call(nullptr, n, g_res, g_ws, w) : -1, before + 6);
        ++g_cases;
        const bool quiet = untouched && launches() == before + 6 && ms >= 0.f && modgpu_sync(-1, nullptr) == MODGPU_OK && call(nullptr, 0, nullptr, nullptr, 0) == MODGPU_OK &&
                           launches() == before + 6 && std::memcmp(g_src, g_src_orig.data(), ARENA) == 0;
        if (!quiet) ++g_failed;
        std::printf("%s rekey digest table: refusals queued nothing; two timed calls queued six launches; no entries does nothing\n", quiet ? "ok  " : "FAIL");
    }

    ++g_cases;
    bool plans = modgpu_shim_rekey_digest_table_plan_errors() == 0 && modgpu_shim_rekey_table_launches(0) == 0; // (never the plain mode's launches)
    for (int l = 0; l < 3; ++l)
        plans = plans && modgpu_shim_rekey_digest_table_launches(l) == modgpu_shim_rekey_digest_table_launches(0) && modgpu_shim_rekey_digest_table_launches(l) > 0;
    if (!plans) ++g_failed;
    std::printf("%s launches: %llu calls of three launches, %llu plan errors\n", plans ? "ok  " : "FAIL", modgpu_shim_rekey_digest_table_launches(0),
                modgpu_shim_rekey_digest_table_plan_errors());
    modgpu_shim_xfer_free(g_ws);
    modgpu_shim_xfer_free(g_res);
    modgpu_shim_xfer_free(g_table);
    modgpu_shim_xfer_free(raw_d);
    modgpu_shim_xfer_free(raw_s);
    std::printf("%d passed, %d failed\n", g_cases - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
