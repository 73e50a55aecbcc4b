// rekey_move_table_main.cpp -- modgpu_rekey_move_table_device on the CPU stand-in of the HIP runtime, as a program of its own (built by
// `make rekey-move-table-main` from the library's host sources with ASan + UBSan, run directly by tests/test_rekey_move_table_cpu.py).
// Every case lays a table over one arena of stand-in device memory and compares EVERY byte of the arena's span with a model computed
// here: want = the arena as it was, then for each entry the source copied out of the ORIGINAL arena, both keystreams XORed in with
// modgpu_cycle_scalar_host, the result put in place.  The stand-in walks the chunks in position order and stores each before it loads
// the next, so a wrong direction, order or window gives wrong bytes, and it counts a plan error for a window that names a chunk not
// yet loaded.  Then the refusals of the device tier (the arena untouched, the status naming the lowest bad entry, the host validator
// agreeing) and those the host makes before anything is queued.  One line per case; exit status 0 = all of it held.
// The matrix is the GPU test's (tests/test_gpu_rekey_move_table.py) at reduced size: the 40-chunk segment runs once per direction.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "modgpu.h"

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
unsigned long long modgpu_shim_move_table_launches(int kind);
unsigned long long modgpu_shim_move_table_plan_errors(void);
}

namespace {
constexpr uint64_t CHUNK = 65536;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
constexpr uint64_t BIG = 40 * CHUNK + 77;
constexpr uint64_t ARENA = 12ull << 20;
int g_failed = 0, g_cases = 0;

struct Keys {
    const char *name;
    int32_t kf, kt;
    uint64_t of, ot;
    bool compaction; // ot follows the shift: a byte that slides down by d drops d in its stream
};
const Keys KEYS[] = {
    {"ps3->ps4", PS3, PS4, 3, 22, false},
    {"compaction", PS4, PS4, (1ull << 32) + 1000000, 0, true},
    {"plain", PS3, PS3, 77, 77, false},
    {"from-identity", 0, PS4, 5, 9, false},
    {"to-identity", PS3, 0x7FFFFFFF, 5, 9, false},
    {"both-identity", 0, (int32_t)0x80000001, 1, 2, false},
};
constexpr int N_KEYS = sizeof KEYS / sizeof KEYS[0];

uint8_t *g_base = nullptr; // chunk-aligned start of the arena
std::vector<uint8_t> g_orig, g_want;
modgpu_rekey_table_entry_t *g_table = nullptr;
constexpr uint64_t MAX_ENTRIES = 512;
uint8_t *g_ws = nullptr;
uint64_t g_ws_bytes = 0;

uint64_t g_rng = 0x243F6A8885A308D3ull;
uint64_t rnd(uint64_t n)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (g_rng >> 33) % n;
}

uint64_t launches()
{
    modgpu_path_stats_t st;
    modgpu_path_stats(&st, 0);
    return st.gpu_launches;
}

struct Seg {
    uint64_t dst, src, n; // offsets from the arena's base
    int keys;             // index into KEYS
};

modgpu_rekey_table_entry_t entry_of(const Seg &s)
{
    const Keys &k = KEYS[s.keys];
    modgpu_rekey_table_entry_t e{};
    e.dst = g_base + s.dst;
    e.src = g_base + s.src;
    e.n = s.n;
    e.off_from = k.of + s.src;
    e.off_to = k.compaction ? k.of + s.dst : k.ot + s.src;
    e.key_from = k.kf;
    e.key_to = k.kt;
    return e;
}

// runs the table over the arena and compares its whole span with the model
void run_table(const std::vector<Seg> &segs, const std::string &what)
{
    uint64_t span = 0, total = 0;
    for (const Seg &s : segs) span = std::max(span, std::max(s.dst, s.src) + s.n), total += s.n;
    span = std::min<uint64_t>(ARENA, span + CHUNK);
    std::memcpy(g_base, g_orig.data(), span);
    std::memcpy(g_want.data(), g_orig.data(), span);
    bool ok = segs.size() <= MAX_ENTRIES;
    for (size_t i = 0; i < segs.size() && ok; ++i) {
        const modgpu_rekey_table_entry_t e = entry_of(segs[i]);
        g_table[i] = e;
        std::vector<uint8_t> moved(g_orig.begin() + (ptrdiff_t)segs[i].src, g_orig.begin() + (ptrdiff_t)(segs[i].src + segs[i].n));
        ok = ok && modgpu_cycle_scalar_host(moved.data(), e.n, e.key_from, e.off_from) == MODGPU_OK &&
             modgpu_cycle_scalar_host(moved.data(), e.n, e.key_to, e.off_to) == MODGPU_OK;
        if (e.n) std::memcpy(g_want.data() + segs[i].dst, moved.data(), e.n);
    }
    const int valid = modgpu_rekey_move_table_validate(g_table, segs.size());
    const uint64_t before = launches();
    const int rc = modgpu_rekey_move_table_device(g_table, segs.size(), total, g_ws, g_ws_bytes, -1, nullptr);
    ok = ok && valid == MODGPU_OK && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 5;
    uint64_t bad = 0, stalled = 0, bad2 = 0;
    ok = ok && modgpu_rekey_move_table_status(g_ws, -1, &bad, &stalled) == MODGPU_OK && bad == UINT64_MAX && stalled == UINT64_MAX;
    ok = ok && modgpu_table_status(g_ws, -1, &bad2) == MODGPU_OK && bad2 == UINT64_MAX;
    const bool same = std::memcmp(g_base, g_want.data(), span) == 0;
    uint64_t first = 0;
    if (!same)
        while (g_base[first] == g_want[first]) ++first;
    ++g_cases;
    const bool pass = ok && same;
    if (!pass) ++g_failed;
    std::printf("%s %s entries=%zu bytes=%llu rc=%d valid=%d%s\n", pass ? "ok  " : "FAIL", what.c_str(), segs.size(), (unsigned long long)total, rc, valid,
                same ? "" : " BYTES");
    if (!same) std::printf("     first differing byte at arena offset %llu\n", (unsigned long long)first);
    if (rc != MODGPU_OK || valid != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
}

// `down`: the segments packed from `start`, their sources the gaps further up each; else the sources packed and the gaps opened
std::vector<Seg> layout(const std::vector<uint64_t> &sizes, const std::vector<uint64_t> &gaps, bool down, uint64_t start, int keys, bool mixed)
{
    std::vector<Seg> segs;
    uint64_t packed = start, spread = start;
    for (size_t i = 0; i < sizes.size(); ++i) {
        spread += gaps[i];
        segs.push_back(down ? Seg{packed, spread, sizes[i], mixed ? (int)(i % N_KEYS) : keys} : Seg{spread, packed, sizes[i], mixed ? (int)(i % N_KEYS) : keys});
        packed += sizes[i];
        spread += sizes[i];
    }
    return segs;
}

// the chunks the plan lays an entry on
uint64_t chunks_of(const modgpu_rekey_table_entry_t &e)
{
    const uint64_t d = reinterpret_cast<uintptr_t>(e.dst), head = std::min<uint64_t>(e.n, (16 - (d & 15)) & 15), words = (e.n - head) / 16;
    return words ? (((d + head) & (CHUNK - 1)) + words * 16 + CHUNK - 1) / CHUNK : 0;
}
// the first entry whose chunks pass what a workspace for total_bytes holds
uint64_t first_past(const std::vector<modgpu_rekey_table_entry_t> &t, uint64_t total_bytes)
{
    uint64_t sum = 0;
    for (size_t i = 0; i < t.size(); ++i)
        if ((sum += chunks_of(t[i])) > total_bytes / CHUNK + 2 * t.size()) return i;
    return UINT64_MAX;
}

// a table that the device must refuse whole: the arena untouched, the status and the validator naming entry `want`
void refuse_table(std::vector<modgpu_rekey_table_entry_t> t, uint64_t total, uint64_t want, bool validator_sees_it, const char *what)
{
    std::memcpy(g_base, g_orig.data(), ARENA);
    std::copy(t.begin(), t.end(), g_table);
    const int valid = modgpu_rekey_move_table_validate(g_table, t.size());
    const bool named = std::string(modgpu_last_error()).find("entry " + std::to_string(want) + ":") != std::string::npos;
    const int rc = modgpu_rekey_move_table_device(g_table, t.size(), total, g_ws, modgpu_rekey_move_table_workspace_bytes(t.size(), total), -1, nullptr);
    bool ok = rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK;
    uint64_t bad = 0, stalled = 0, bad2 = 0;
    ok = ok && modgpu_rekey_move_table_status(g_ws, -1, &bad, &stalled) == MODGPU_ERR_INVALID && bad == want && stalled == UINT64_MAX;
    ok = ok && modgpu_table_status(g_ws, -1, &bad2) == MODGPU_ERR_INVALID && bad2 == want;
    ok = ok && (validator_sees_it ? valid == MODGPU_ERR_INVALID && named : valid == MODGPU_OK);
    ok = ok && std::memcmp(g_base, g_orig.data(), ARENA) == 0;
    ++g_cases;
    if (!ok) ++g_failed;
    std::printf("%s device refusal: %s rc=%d valid=%d bad=%llu\n", ok ? "ok  " : "FAIL", what, rc, valid, (unsigned long long)bad);
}

void refuse(const char *what, int rc)
{
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID;
    if (!pass) ++g_failed;
    std::printf("%s refusal: %s rc=%d\n", pass ? "ok  " : "FAIL", what, rc);
}
} // namespace

int main()
{
    uint8_t *raw = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(ARENA + CHUNK, 0));
    g_table = static_cast<modgpu_rekey_table_entry_t *>(modgpu_shim_xfer_alloc(MAX_ENTRIES * sizeof(modgpu_rekey_table_entry_t), 0));
    g_ws_bytes = modgpu_rekey_move_table_workspace_bytes(MAX_ENTRIES, ARENA);
    g_ws = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(g_ws_bytes, 0));
    if (!raw || !g_table || !g_ws || !g_ws_bytes) return 2;
    g_base = raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1));
    g_orig.resize(ARENA);
    g_want.resize(ARENA);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : g_orig) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }

    // workspace sizes: 0 where documented, non-decreasing in both arguments
    {
        auto w = modgpu_rekey_move_table_workspace_bytes;
        bool okw = w(0, 1000) == 0 && w(MODGPU_TABLE_MAX_ENTRIES + 1ull, 1000) == 0 && w(1, ~0ull) == 0 && w(1, 0) > 0;
        for (uint64_t n = 1; n <= MODGPU_TABLE_MAX_ENTRIES; n = n * 5 + 1)
            for (uint64_t b = 0; b < (1ull << 44); b = b * 7 + 3) okw = okw && w(n, b) > 0 && w(n, b) % 8 == 0 && w(n * 5 + 1 <= MODGPU_TABLE_MAX_ENTRIES ? n * 5 + 1 : n, b) >= w(n, b) && w(n, b * 7 + 3) >= w(n, b);
        ++g_cases;
        if (!okw) ++g_failed;
        std::printf("%s workspace sizes\n", okw ? "ok  " : "FAIL");
    }

    // (1) the matrix at reduced size: five segments, sizes and gaps drawn from the lists, both directions, three destination phases,
    // every key pair and one table that mixes all six
    const uint64_t SIZES[] = {1, 15, 17, 65535, 65537, 131073};
    const uint64_t GAPS[] = {1, 3, 16, 17, 4096, 65535, 65536, 65537, 3 * CHUNK + 5};
    for (int down = 1; down >= 0; --down)
        for (uint64_t ph : {0ull, 1ull, 7ull})
            for (int k = 0; k <= N_KEYS; ++k)
                for (int draw = 0; draw < 2; ++draw) {
                    std::vector<uint64_t> sizes, gaps;
                    for (int i = 0; i < 5; ++i) {
                        sizes.push_back(SIZES[rnd(6)]);
                        gaps.push_back(GAPS[rnd(9)]);
                    }
                    const bool mixed = k == N_KEYS;
                    run_table(layout(sizes, gaps, down != 0, CHUNK + 12345 * draw + ph, mixed ? 0 : k, mixed),
                              std::string(down ? "down " : "up   ") + (mixed ? "mixed" : KEYS[k].name) + " phase " + std::to_string(ph));
                }
    for (int down = 1; down >= 0; --down) // the 40-chunk segment between small ones, shifts from below a chunk to above
        run_table(layout({65537, BIG, 17, 131073, 15}, {4096, 17, 65537, 3, 3 * CHUNK + 5}, down != 0, CHUNK + 7, 0, true), down ? "down big mixed" : "up   big mixed");

    // (2) across entries
    for (int down = 1; down >= 0; --down) {
        // gaps below a chunk: the first destination chunk of entry i+1 covers the last source chunk of entry i
        run_table(layout({3 * CHUNK + 5, 2 * CHUNK + 100, 3 * CHUNK, 65537, 2 * CHUNK + 1}, {100, 17, 4096, 1, 65535}, down != 0, CHUNK + 1, 1, false),
                  down ? "down across gaps below a chunk" : "up   across gaps below a chunk");
        // 300 entries of 1..100 bytes with 1-byte gaps, then one of 5 chunks + 9: its first destination chunk meets many entries' sources
        std::vector<uint64_t> sizes, gaps;
        for (int i = 0; i < 300; ++i) {
            sizes.push_back(1 + rnd(100));
            gaps.push_back(1);
        }
        sizes.push_back(5 * CHUNK + 9);
        gaps.push_back(1);
        if (!down) { // opened: the large entry first, so that ITS sources lie under the small entries' destinations
            std::reverse(sizes.begin(), sizes.end());
        }
        run_table(layout(sizes, gaps, down != 0, CHUNK + 3, 0, false), down ? "down across 300 small entries" : "up   across 300 small entries");
        run_table(layout(sizes, gaps, down != 0, CHUNK + 3, 0, true), down ? "down across 300 small entries mixed" : "up   across 300 small entries mixed");
        // dst == src in the middle of a table: entry 2 sits at its source, the entries before and after it slide
        std::vector<Seg> mid;
        if (down) {
            mid = {{CHUNK, CHUNK + 500, 70000, 0}, {CHUNK + 70000, CHUNK + 80000, 65537, 1}, {4 * CHUNK + 9, 4 * CHUNK + 9, 2 * CHUNK + 3, 2},
                   {6 * CHUNK + 12, 6 * CHUNK + 4096, 131073, 3}, {9 * CHUNK, 9 * CHUNK + 100, 17, 4}};
        } else {
            mid = {{CHUNK + 500, CHUNK, 70000, 0}, {3 * CHUNK, 2 * CHUNK + 60000, 65537, 1}, {4 * CHUNK + 9, 4 * CHUNK + 9, 2 * CHUNK + 3, 2},
                   {6 * CHUNK + 4096, 6 * CHUNK + 12, 131073, 3}, {9 * CHUNK + 100, 9 * CHUNK, 17, 4}};
        }
        run_table(mid, down ? "down an entry in the middle stays" : "up   an entry in the middle stays");
        // empty entries anywhere, with pointers of any kind
        std::vector<Seg> holes = mid;
        holes.insert(holes.begin() + 2, Seg{0, ARENA - 1, 0, 0});
        holes.insert(holes.begin(), Seg{ARENA - 1, 0, 0, 0});
        holes.push_back(Seg{5, 5, 0, 0});
        run_table(holes, down ? "down with empty entries" : "up   with empty entries");
    }
    // one entry, each shape: what modgpu_rekey_move_device does for it
    for (uint64_t n : {1ull, 15ull, 17ull, 65535ull, 65537ull, 131073ull})
        for (uint64_t d : {1ull, 17ull, 65537ull})
            for (int down = 1; down >= 0; --down)
                run_table(layout({n}, {d}, down != 0, CHUNK + 7, (int)((n + d) % N_KEYS), false), down ? "down one entry" : "up   one entry");

    // (5) refusals on the device
    {
        const std::vector<Seg> good = layout({65537, 131073, 17, 2 * CHUNK + 5, 70000}, {4096, 17, 1, 65537, 3}, true, CHUNK + 7, 0, false);
        std::vector<modgpu_rekey_table_entry_t> t;
        uint64_t total = 0;
        for (const Seg &s : good) t.push_back(entry_of(s)), total += s.n;
        auto with = [&](auto change) {
            std::vector<modgpu_rekey_table_entry_t> u = t;
            change(u);
            return u;
        };
        refuse_table(with([](auto &u) { void *d = u[3].dst; u[3].dst = const_cast<void *>(u[3].src); u[3].src = d; }), total, 3, true, "an upward entry in a downward table");
        refuse_table(with([](auto &u) { std::swap(u[1], u[2]); }), total, 2, true, "two entries listed in falling order");
        refuse_table(with([](auto &u) { u[2].dst = static_cast<uint8_t *>(u[1].dst) + u[1].n - 1; }), total, 2, true, "overlapping destinations");
        refuse_table(with([](auto &u) { u[4].src = static_cast<const uint8_t *>(u[3].src) + u[3].n - 1; u[4].dst = static_cast<uint8_t *>(u[3].dst) + u[3].n; }), total, 4, true,
                     "overlapping sources");
        refuse_table(with([](auto &u) { u[1].flags = 1; }), total, 1, true, "nonzero flags");
        refuse_table(with([](auto &u) { u[3].reserved = 7; u[4].flags = 1; }), total, 3, true, "nonzero reserved, the lowest of two");
        refuse_table(with([](auto &u) { u[2].src = nullptr; }), total, 2, true, "a null source");
        refuse_table(with([](auto &u) { u[0].n = 1ull << 41; }), total, 0, true, "an entry of 1 TiB or more");
        for (const std::vector<uint64_t> &sizes : {std::vector<uint64_t>{BIG, 131073, 17}, std::vector<uint64_t>{17, 65537, BIG, 17}}) {
            std::vector<modgpu_rekey_table_entry_t> u;
            for (const Seg &s : layout(sizes, {4096, 17, 1, 65537}, true, CHUNK + 7, 0, false)) u.push_back(entry_of(s));
            const uint64_t past = first_past(u, 1000);
            refuse_table(u, 1000, past, false, past == 0 ? "total_bytes too small for the table" : "total_bytes too small from a later entry on");
        }
    }

    // host refusals, all before anything is queued
    {
        std::memcpy(g_base, g_orig.data(), ARENA);
        const std::vector<Seg> good = layout({65537, 131073}, {4096, 17}, true, CHUNK + 7, 0, false);
        for (size_t i = 0; i < good.size(); ++i) g_table[i] = entry_of(good[i]);
        const uint64_t total = 65537 + 131073, w = modgpu_rekey_move_table_workspace_bytes(2, total);
        const uint64_t before = launches();
        std::vector<uint64_t> host(w / 8 + 8);
        auto call = modgpu_rekey_move_table_device;
        refuse("null table", call(nullptr, 2, total, g_ws, w, -1, nullptr));
        refuse("null workspace", call(g_table, 2, total, nullptr, w, -1, nullptr));
        refuse("misaligned workspace", call(g_table, 2, total, g_ws + 4, w, -1, nullptr));
        refuse("misaligned table", call(reinterpret_cast<modgpu_rekey_table_entry_t *>(reinterpret_cast<uint8_t *>(g_table) + 4), 2, total, g_ws, w, -1, nullptr));
        refuse("short workspace", call(g_table, 2, total, g_ws, w - 1, -1, nullptr));
        refuse("too many entries", call(g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull, total, g_ws, ~0ull, -1, nullptr));
        refuse("total_bytes beyond 2^31 chunks", call(g_table, 2, ~0ull, g_ws, ~0ull, -1, nullptr));
        refuse("workspace that is not device memory", call(g_table, 2, total, host.data(), w, -1, nullptr));
        refuse("table that is not device memory", call(reinterpret_cast<modgpu_rekey_table_entry_t *>(host.data()), 2, total, g_ws, w, -1, nullptr));
        uint64_t a = 0, b = 0;
        refuse("status of a null workspace", modgpu_rekey_move_table_status(nullptr, -1, &a, &b));
        refuse("status without out pointers", modgpu_rekey_move_table_status(g_ws, -1, nullptr, &b));
        refuse("status of host memory", modgpu_rekey_move_table_status(host.data(), -1, &a, &b));
        refuse("validate a null table", modgpu_rekey_move_table_validate(nullptr, 3));
        ++g_cases;
        const bool quiet = launches() == before && std::memcmp(g_base, g_orig.data(), ARENA) == 0 && call(nullptr, 0, 0, nullptr, 0, -1, nullptr) == MODGPU_OK &&
                           modgpu_rekey_move_table_validate(nullptr, 0) == MODGPU_OK;
        if (!quiet) ++g_failed;
        std::printf("%s refusals queued nothing and wrote nothing; no entries does nothing\n", quiet ? "ok  " : "FAIL");
    }

    ++g_cases;
    bool plans = modgpu_shim_move_table_plan_errors() == 0;
    for (int k = 0; k < 5; ++k) plans = plans && modgpu_shim_move_table_launches(k) == modgpu_shim_move_table_launches(0) && modgpu_shim_move_table_launches(k) > 0;
    if (!plans) ++g_failed;
    std::printf("%s launch plans: %llu window errors, %llu calls of five launches\n", plans ? "ok  " : "FAIL", modgpu_shim_move_table_plan_errors(),
                modgpu_shim_move_table_launches(0));
    modgpu_shim_xfer_free(g_ws);
    modgpu_shim_xfer_free(g_table);
    modgpu_shim_xfer_free(raw);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
