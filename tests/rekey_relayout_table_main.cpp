// rekey_relayout_table_main.cpp -- modgpu_rekey_relayout_table_device on the CPU stand-in of the HIP runtime, as a program of its own
// (built by `make rekey-relayout-table-main` from the library's host sources with ASan + UBSan, run directly by
// tests/test_rekey_relayout_cpu.py).  Every case lays a table whose entries slide BOTH ways over one arena of stand-in device memory and
// compares EVERY byte of the arena's span with a model computed here: want = the arena as it was, then for each entry the source copied
// out of the ORIGINAL arena, both keystreams XORed in with modgpu_cycle_scalar_host, the result put in place.  The stand-in runs the two
// sweeps one after the other, walks each sweep's chunks in position order and stores each before it loads the next, so a wrong filter,
// direction, order or window gives wrong bytes, and it counts a plan error for a window that names a chunk not yet loaded or misses
// one.  Then the refusals of the device tier (the arena untouched, the status naming the lowest bad entry, the host validator
// agreeing) and those the host makes before anything is queued.  One line per case; exit status 0 = all of it held.
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
unsigned long long modgpu_shim_relayout_launches(int kind);
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
    bool compaction; // ot follows the shift: a byte that slides by d moves d in its stream
};
// the six key pairs of tests/test_gpu_rekey_move_table.py
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
    for (const Seg &s : segs)
        if (s.n) span = std::max(span, std::max(s.dst, s.src) + s.n), total += s.n;
    span = std::min<uint64_t>(ARENA, span + CHUNK);
    std::memcpy(g_base, g_orig.data(), span);
    std::memcpy(g_want.data(), g_orig.data(), span);
    bool ok = segs.size() <= MAX_ENTRIES;
    for (size_t i = 0; i < segs.size() && ok; ++i) {
        const modgpu_rekey_table_entry_t e = entry_of(segs[i]);
        g_table[i] = e;
        if (!e.n) continue;
        std::vector<uint8_t> moved(g_orig.begin() + (ptrdiff_t)segs[i].src, g_orig.begin() + (ptrdiff_t)(segs[i].src + segs[i].n));
        ok = ok && modgpu_cycle_scalar_host(moved.data(), e.n, e.key_from, e.off_from) == MODGPU_OK &&
             modgpu_cycle_scalar_host(moved.data(), e.n, e.key_to, e.off_to) == MODGPU_OK;
        std::memcpy(g_want.data() + segs[i].dst, moved.data(), e.n);
    }
    const int valid = modgpu_rekey_relayout_table_validate(g_table, segs.size());
    const uint64_t before = launches();
    const int rc = modgpu_rekey_relayout_table_device(g_table, segs.size(), total, g_ws, g_ws_bytes, -1, nullptr);
    ok = ok && valid == MODGPU_OK && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 10;
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

// A table from a run pattern -- a string of D (slides down), U (slides up), S (stays), one letter per entry: the sources laid from
// `start` upward with small gaps, each entry's shift drawn from SHIFTS with the sign of its letter, the gaps widened on whichever side
// the change of shift needs so that sources and destinations both stay disjoint and rising.  Sizes and shifts rotate from `turn`.
const uint64_t SIZES[] = {1, 15, 17, 4101, 65535, 65537, 131073};
const uint64_t SHIFTS[] = {1, 17, 4099, 65541, 7, 65536};
const uint64_t GAPS[] = {0, 1, 3, 16};
std::vector<Seg> pattern(const std::string &runs, uint64_t start, int turn, const std::vector<uint64_t> &sizes = {})
{
    std::vector<Seg> segs;
    uint64_t src = start;
    int64_t shift = 0, dst_end = 0;
    for (size_t i = 0; i < runs.size(); ++i) {
        const uint64_t n = sizes.empty() ? SIZES[(i + (size_t)turn) % 7] : sizes[i];
        const int64_t want = runs[i] == 'S' ? 0 : (runs[i] == 'U' ? 1 : -1) * (int64_t)SHIFTS[(i + 2 * (size_t)turn) % 6];
        src += GAPS[(i + (size_t)turn) % 4];
        if (i && (int64_t)src + want < dst_end) src = (uint64_t)(dst_end - want); // the destination would fall into the one before it
        shift = want;
        segs.push_back(Seg{(uint64_t)((int64_t)src + shift), src, n, (int)((i + (size_t)turn) % N_KEYS)});
        dst_end = (int64_t)src + shift + (int64_t)n;
        src += n;
    }
    return segs;
}

// `each` sliding alternately by +7 and -7
std::vector<Seg> alternating(uint64_t count, uint64_t each, uint64_t start)
{
    std::vector<Seg> segs;
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t src = start + i * (each + 16);
        segs.push_back(Seg{i % 2 ? src - 7 : src + 7, src, each, (int)(i % N_KEYS)});
    }
    return segs;
}

// the chunks the plan lays an entry on
uint64_t chunks_of(const modgpu_rekey_table_entry_t &e)
{
    const uint64_t d = reinterpret_cast<uintptr_t>(e.dst), head = std::min<uint64_t>(e.n, (16 - (d & 15)) & 15), words = (e.n - head) / 16;
    return words ? (((d + head) & (CHUNK - 1)) + words * 16 + CHUNK - 1) / CHUNK : 0;
}

// a table that the device must refuse whole: the arena untouched in either sweep, the status and the validator naming entry `want`
void refuse_table(std::vector<modgpu_rekey_table_entry_t> t, uint64_t total, uint64_t want, bool validator_sees_it, const char *what)
{
    std::memcpy(g_base, g_orig.data(), ARENA);
    std::copy(t.begin(), t.end(), g_table);
    const int valid = modgpu_rekey_relayout_table_validate(g_table, t.size());
    const bool named = std::string(modgpu_last_error()).find("entry " + std::to_string(want) + ":") != std::string::npos;
    const uint64_t before = launches();
    const int rc = modgpu_rekey_relayout_table_device(g_table, t.size(), total, g_ws, modgpu_rekey_move_table_workspace_bytes(t.size(), total), -1, nullptr);
    bool ok = rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK && launches() - before == 10;
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

// a host table the validator must refuse, naming entry `want`; the old validator's answer does not matter here
void refuse_valid(std::vector<modgpu_rekey_table_entry_t> t, uint64_t want, const char *what)
{
    const int rc = modgpu_rekey_relayout_table_validate(t.data(), t.size());
    const bool named = std::string(modgpu_last_error()).find("entry " + std::to_string(want) + ":") != std::string::npos;
    ++g_cases;
    const bool pass = rc == MODGPU_ERR_INVALID && named;
    if (!pass) ++g_failed;
    std::printf("%s validator refusal: %s rc=%d (%s)\n", pass ? "ok  " : "FAIL", what, rc, modgpu_last_error());
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

    // (1) the run patterns: sizes, shifts and key pairs in rotation, three destination phases
    const char *PATTERNS[] = {"DU", "UD", "DSU", "UDUD", "DDUUDD"};
    for (const char *runs : PATTERNS)
        for (uint64_t ph : {0ull, 1ull, 7ull})
            for (int turn = 0; turn < 7; ++turn)
                run_table(pattern(runs, 2 * CHUNK + 12345 * (uint64_t)turn + ph, turn), std::string("pattern ") + runs + " phase " + std::to_string(ph));
    // the 40-chunk segment once per direction, between entries of the other one
    run_table(pattern("DUD", 2 * CHUNK + 7, 0, {65537, BIG, 4101}), "pattern DUD big up");
    run_table(pattern("UDU", 2 * CHUNK + 7, 1, {131073, BIG, 17}), "pattern UDU big down");
    // one-way tables: the other sweep is idle
    for (uint64_t ph : {0ull, 1ull, 7ull}) {
        run_table(pattern("DDDSD", 2 * CHUNK + ph, 3), "pure down phase " + std::to_string(ph));
        run_table(pattern("UUSUU", 2 * CHUNK + ph, 4), "pure up phase " + std::to_string(ph));
        run_table(pattern("SSS", 2 * CHUNK + ph, 5), "all stationary phase " + std::to_string(ph));
    }

    // (2) small entries: 64 of 9 bytes and 64 of 1000 bytes, sliding alternately by +7 and -7
    for (uint64_t ph : {0ull, 1ull, 7ull}) {
        run_table(alternating(64, 9, CHUNK + ph), "alternating 64 x 9 phase " + std::to_string(ph));
        run_table(alternating(64, 1000, CHUNK + ph), "alternating 64 x 1000 phase " + std::to_string(ph));
    }
    run_table(alternating(300, 100, CHUNK - 3), "alternating 300 x 100 across a chunk boundary");

    // (3) empty entries between the runs, with pointers of any kind
    for (const char *runs : PATTERNS) {
        std::vector<Seg> segs = pattern(runs, 2 * CHUNK + 9, 2), holes;
        holes.push_back(Seg{ARENA - 1, 0, 0, 0});
        for (size_t i = 0; i < segs.size(); ++i) {
            if (i && runs[i] != runs[i - 1]) holes.push_back(Seg{i % 2 ? 0ull : 5ull, i % 2 ? ARENA - 1 : 5ull, 0, 0});
            holes.push_back(segs[i]);
        }
        holes.push_back(Seg{5, 7, 0, 0});
        run_table(holes, std::string("empty entries between the runs of ") + runs);
    }

    // (4) refusals on the device: nothing written by either sweep
    {
        const std::vector<Seg> good = pattern("DUDUD", 2 * CHUNK + 7, 0, {65537, 131073, 17, 2 * CHUNK + 5, 70000});
        std::vector<modgpu_rekey_table_entry_t> t;
        uint64_t total = 0;
        for (const Seg &s : good) t.push_back(entry_of(s)), total += s.n;
        auto with = [&](auto change) {
            std::vector<modgpu_rekey_table_entry_t> u = t;
            change(u);
            return u;
        };
        refuse_table(with([](auto &u) { u[1].dst = static_cast<uint8_t *>(u[2].dst) - u[1].n + 1; }), total, 2, true,
                     "an upward entry's destination runs into the next, downward, entry's");
        refuse_table(with([](auto &u) { std::swap(u[1], u[2]); }), total, 2, true, "falling order across a direction change");
        refuse_table(with([](auto &u) { std::swap(u[2], u[3]); }), total, 3, true, "falling order across the other direction change");
        refuse_table(with([](auto &u) { u[3].src = static_cast<const uint8_t *>(u[2].src) + u[2].n - 1; }), total, 3, true, "overlapping sources across a direction change");
        refuse_table(with([](auto &u) { u[1].flags = 1; }), total, 1, true, "nonzero flags on an entry sweep 0 filters");
        refuse_table(with([](auto &u) { u[2].flags = 1; }), total, 2, true, "nonzero flags on an entry sweep 1 filters");
        refuse_table(with([](auto &u) { u[3].reserved = 7; u[4].flags = 1; }), total, 3, true, "nonzero reserved, the lowest of two");
        refuse_table(with([](auto &u) { u[3].src = nullptr; }), total, 3, true, "a null source on an upward entry");
        refuse_table(with([](auto &u) { u[2].dst = nullptr; }), total, 2, true, "a null destination");
        refuse_table(with([](auto &u) { u[4].n = 1ull << 41; }), total, 4, true, "an entry of 1 TiB or more");
        // each sweep alone fits the workspace, the table does not: refused on the count over ALL entries
        for (const char *runs : {"DU", "UD", "DSUD"}) {
            std::vector<uint64_t> sizes(std::strlen(runs), 17);
            sizes[0] = BIG;
            sizes[1 + (runs[1] == 'S')] = BIG;
            std::vector<modgpu_rekey_table_entry_t> u;
            for (const Seg &s : pattern(runs, 2 * CHUNK + 7, 0, sizes)) u.push_back(entry_of(s));
            const uint64_t small = 45 * CHUNK, room = small / CHUNK + 2 * u.size();
            uint64_t down = 0, up = 0, sum = 0, past = UINT64_MAX;
            for (size_t i = 0; i < u.size(); ++i) {
                (u[i].dst > u[i].src ? up : down) += chunks_of(u[i]);
                if ((sum += chunks_of(u[i])) > room && past == UINT64_MAX) past = i;
            }
            if (down > room || up > room || past == UINT64_MAX) {
                ++g_cases, ++g_failed;
                std::printf("FAIL the case itself: %llu down, %llu up, room %llu\n", (unsigned long long)down, (unsigned long long)up, (unsigned long long)room);
                continue;
            }
            refuse_table(u, small, past, false, "total_bytes enough for each sweep alone, too small for the table");
        }
    }

    // (5) host refusals, all before anything is queued: every one the validator makes, then tier 1 of the call
    {
        std::memcpy(g_base, g_orig.data(), ARENA);
        const std::vector<Seg> good = pattern("DU", 2 * CHUNK + 7, 0, {65537, 131073});
        std::vector<modgpu_rekey_table_entry_t> t;
        for (size_t i = 0; i < good.size(); ++i) t.push_back(g_table[i] = entry_of(good[i]));
        const uint64_t total = 65537 + 131073, w = modgpu_rekey_move_table_workspace_bytes(2, total);
        const uint64_t before = launches();
        auto with = [&](auto change) {
            std::vector<modgpu_rekey_table_entry_t> u = t;
            change(u);
            return u;
        };
        refuse("validate a null table", modgpu_rekey_relayout_table_validate(nullptr, 3));
        refuse("validate more entries than a table has", modgpu_rekey_relayout_table_validate(g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull));
        refuse_valid(with([](auto &u) { u[1].flags = 1; }), 1, "nonzero flags");
        refuse_valid(with([](auto &u) { u[0].reserved = 1u << 31; }), 0, "nonzero reserved");
        refuse_valid(with([](auto &u) { u[1].src = nullptr; }), 1, "a null source");
        refuse_valid(with([](auto &u) { u[0].dst = nullptr; }), 0, "a null destination");
        refuse_valid(with([](auto &u) { u[1].n = 1ull << 40; }), 1, "an entry of 1 TiB or more");
        refuse_valid(with([](auto &u) { std::swap(u[0], u[1]); }), 1, "falling sources");
        refuse_valid(with([](auto &u) { u[1].src = static_cast<const uint8_t *>(u[0].src) + u[0].n - 1; }), 1, "overlapping sources");
        refuse_valid(with([](auto &u) { u[1].dst = static_cast<uint8_t *>(u[0].dst) + u[0].n - 1; }), 1, "overlapping destinations");
        refuse_valid(with([](auto &u) { u[1].dst = static_cast<uint8_t *>(u[0].dst) - 1; }), 1, "falling destinations");
        std::vector<uint64_t> host(w / 8 + 8);
        auto call = modgpu_rekey_relayout_table_device;
        refuse("null table", call(nullptr, 2, total, g_ws, w, -1, nullptr));
        refuse("null workspace", call(g_table, 2, total, nullptr, w, -1, nullptr));
        refuse("misaligned workspace", call(g_table, 2, total, g_ws + 4, w, -1, nullptr));
        refuse("misaligned table", call(reinterpret_cast<modgpu_rekey_table_entry_t *>(reinterpret_cast<uint8_t *>(g_table) + 4), 2, total, g_ws, w, -1, nullptr));
        refuse("short workspace", call(g_table, 2, total, g_ws, w - 1, -1, nullptr));
        refuse("too many entries", call(g_table, MODGPU_TABLE_MAX_ENTRIES + 1ull, total, g_ws, ~0ull, -1, nullptr));
        refuse("total_bytes beyond 2^31 chunks", call(g_table, 2, ~0ull, g_ws, ~0ull, -1, nullptr));
        refuse("workspace that is not device memory", call(g_table, 2, total, host.data(), w, -1, nullptr));
        refuse("table that is not device memory", call(reinterpret_cast<modgpu_rekey_table_entry_t *>(host.data()), 2, total, g_ws, w, -1, nullptr));
        ++g_cases;
        const bool quiet = launches() == before && std::memcmp(g_base, g_orig.data(), ARENA) == 0 && call(nullptr, 0, 0, nullptr, 0, -1, nullptr) == MODGPU_OK &&
                           modgpu_rekey_relayout_table_validate(nullptr, 0) == MODGPU_OK && modgpu_rekey_relayout_table_validate(t.data(), 2) == MODGPU_OK &&
                           modgpu_rekey_move_table_validate(t.data(), 2) == MODGPU_ERR_INVALID;
        if (!quiet) ++g_failed;
        std::printf("%s refusals queued nothing and wrote nothing; no entries does nothing; the move table validator still refuses a mixed table\n",
                    quiet ? "ok  " : "FAIL");
    }

    ++g_cases;
    // every call: one plan and one finish launch per sweep from the relayout stand-in, one window, move and place launch per sweep
    // from the move table stand-in, and none of the latter's own plan or finish launches
    const unsigned long long sweeps = modgpu_shim_relayout_launches(0);
    bool plans = modgpu_shim_move_table_plan_errors() == 0 && sweeps > 0 && sweeps % 2 == 0 && modgpu_shim_relayout_launches(1) == sweeps;
    for (int k = 0; k < 5; ++k) plans = plans && modgpu_shim_move_table_launches(k) == (k < 2 ? 0 : sweeps);
    if (!plans) ++g_failed;
    std::printf("%s launch plans: %llu window errors, %llu calls of ten launches\n", plans ? "ok  " : "FAIL", modgpu_shim_move_table_plan_errors(), sweeps / 2);
    modgpu_shim_xfer_free(g_ws);
    modgpu_shim_xfer_free(g_table);
    modgpu_shim_xfer_free(raw);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
