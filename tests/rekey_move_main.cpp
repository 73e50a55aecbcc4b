// rekey_move_main.cpp -- modgpu_rekey_move_device on the CPU stand-in of the HIP runtime, as a program of its own (built by
// `make rekey-move-main` from the library's host sources with ASan + UBSan, run directly by tests/test_rekey_move_cpu.py).
// Every case runs in one arena of stand-in device memory and compares EVERY byte of the arena's span with a model computed here: the
// source copied out, both keystreams XORed in with modgpu_cycle_scalar_host, the result put in place, everything else untouched.
// Then every refusal the host makes before anything is queued.  One line per case; exit status 0 = all of it held.
// The matrix is the GPU test's (tests/test_gpu_rekey_move.py), THINNED to keep a byte-by-byte sanitizer run short: every shift x
// direction x destination phase x size is run, but with the six key pairs taken in rotation rather than crossed in; every key pair is
// then run on a few geometries (shifts 1, 17, 65 537 at one phase, every size); and the largest size runs 2 or 3 of the 6 phases.
// The full cross product runs on the device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "modgpu.h"

extern "C" {
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
unsigned long long modgpu_shim_move_launches(int form);
unsigned long long modgpu_shim_move_plan_errors(void);
unsigned long long modgpu_shim_rekey_plan_errors(void);
}

namespace {
constexpr uint64_t CHUNK = 65536;
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
constexpr uint64_t BIG = 2 * 1024 * 1024 + 512 * 1024 + 77; // 40 chunks and a tail
int g_failed = 0, g_cases = 0;

struct Keys {
    const char *name;
    int32_t kf, kt;
    uint64_t of, ot; // ot is moved by -+d for the compaction pair
    bool compaction;
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
uint8_t *g_ws = nullptr;
uint64_t g_ws_bytes = 0;

uint64_t launches()
{
    modgpu_path_stats_t st;
    modgpu_path_stats(&st, 0);
    return st.gpu_launches;
}

// dst and src as offsets from the arena's base; span = bytes of the arena compared
void run_case(uint64_t dst, uint64_t src, uint64_t n, const Keys &k, uint64_t span, const char *what)
{
    const int64_t shift = (int64_t)src - (int64_t)dst;
    const uint64_t ot = k.compaction ? k.of - (uint64_t)shift : k.ot; // a byte that slides down by d drops d in its stream
    std::memcpy(g_base, g_orig.data(), span);
    std::memcpy(g_want.data(), g_orig.data(), span);
    std::vector<uint8_t> moved(g_orig.begin() + src, g_orig.begin() + src + n);
    int ok = modgpu_cycle_scalar_host(moved.data(), n, k.kf, k.of) == MODGPU_OK && modgpu_cycle_scalar_host(moved.data(), n, k.kt, ot) == MODGPU_OK;
    std::memcpy(g_want.data() + dst, moved.data(), n);
    const uint64_t before = launches(), body_before = modgpu_shim_move_launches(0) + modgpu_shim_move_launches(1);
    const int rc = modgpu_rekey_move_device(g_base + dst, g_base + src, n, k.kf, k.of, k.kt, ot, g_ws, g_ws_bytes, -1, nullptr);
    ok = ok && rc == MODGPU_OK && modgpu_sync(-1, nullptr) == MODGPU_OK;
    uint64_t stalled = 0;
    ok = ok && modgpu_move_status(g_ws, -1, &stalled) == MODGPU_OK && stalled == UINT64_MAX;
    const bool same = std::memcmp(g_base, g_want.data(), span) == 0;
    uint64_t first_bad = 0;
    if (!same)
        while (g_base[first_bad] == g_want[first_bad]) ++first_bad;
    // launches as documented, where the ranges partly overlap and both keystreams are real: pieces (1 if any) + body (1 if any)
    bool counted = true;
    const bool overlap = dst != src && (dst < src ? src < dst + n : dst < src + n);
    if (overlap) {
        uint64_t head = std::min<uint64_t>(n, (CHUNK - (dst & (CHUNK - 1))) & (CHUNK - 1)), body = (n - head) & ~15ull, tail = n - head - body;
        if (!body) head = n, tail = 0;
        const uint64_t bodies = modgpu_shim_move_launches(0) + modgpu_shim_move_launches(1) - body_before;
        counted = bodies == (body ? 1u : 0u);
        if (k.kf != 0 && k.kt != 0x7FFFFFFF && k.kt != 0) counted = counted && launches() - before == (head || tail ? 1u : 0u) + (body ? 1u : 0u);
    }
    ++g_cases;
    const bool pass = ok && same && counted;
    if (!pass) ++g_failed;
    std::printf("%s %s %s n=%llu dst=%llu shift=%lld rc=%d%s%s\n", pass ? "ok  " : "FAIL", what, k.name, (unsigned long long)n, (unsigned long long)dst,
                (long long)shift, rc, same ? "" : " BYTES", counted ? "" : " LAUNCHES");
    if (!same) std::printf("     first differing byte at arena offset %llu\n", (unsigned long long)first_bad);
    if (rc != MODGPU_OK) std::printf("     %s\n", modgpu_last_error());
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
    const uint64_t n_sizes[] = {1, 15, 17, 65535, 65537, 131071, 131073, BIG};
    const uint64_t max_span = 3 * CHUNK + BIG + BIG + 64;
    uint8_t *raw = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(max_span + CHUNK, 0));
    g_ws_bytes = modgpu_move_workspace_bytes(BIG);
    g_ws = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(g_ws_bytes, 0));
    if (!raw || !g_ws || !g_ws_bytes) return 2;
    g_base = raw + ((CHUNK - (reinterpret_cast<uintptr_t>(raw) & (CHUNK - 1))) & (CHUNK - 1));
    g_orig.resize(max_span);
    g_want.resize(max_span);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &b : g_orig) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }

    // workspace sizes: 0 at the ends of the range, non-decreasing inside
    {
        bool okw = modgpu_move_workspace_bytes(0) == 0 && modgpu_move_workspace_bytes(1ull << 40) == 0 && modgpu_move_workspace_bytes(~0ull) == 0;
        uint64_t prev = 0;
        for (uint64_t n = 1; n < (1ull << 40); n = n * 3 + 1) {
            const uint64_t w = modgpu_move_workspace_bytes(n);
            okw = okw && w >= prev && w > 0;
            prev = w;
        }
        okw = okw && modgpu_move_workspace_bytes((1ull << 40) - 1) >= prev;
        ++g_cases;
        if (!okw) ++g_failed;
        std::printf("%s workspace sizes\n", okw ? "ok  " : "FAIL");
    }

    int rot = 0;
    for (uint64_t n : n_sizes) {
        std::vector<uint64_t> shifts = {1, 3, 4, 15, 16, 17, 4096, 3 * CHUNK + 5, n - 1};
        for (uint64_t d = 65532; d <= 65540; ++d) shifts.push_back(d);
        bool disjoint_done = false;
        for (uint64_t d : shifts) {
            if (d == 0) continue;
            if (d >= n) { // disjoint ranges: the rekey call's route, once per size and direction
                if (disjoint_done) continue;
                disjoint_done = true;
            }
            for (int up = 0; up < 2; ++up)
                for (uint64_t at : {0ull, 12345ull})
                    for (uint64_t ph : {0ull, 1ull, 7ull}) {
                        if (n == BIG && !((at == 0 && ph == 0) || (at == 12345 && ph == 7) || (at == 0 && ph == 1 && d % 4 == 1))) continue; // (time)
                        const uint64_t lo = CHUNK + at + ph, hi = lo + d;
                        const uint64_t dst = up ? hi : lo, src = up ? lo : hi;
                        run_case(dst, src, n, KEYS[rot++ % N_KEYS], hi + n + CHUNK, up ? "up  " : "down");
                    }
        }
        // every pair of keys on a few geometries
        for (const Keys &k : KEYS)
            for (uint64_t d : {1ull, 17ull, 65537ull})
                for (int up = 0; up < 2; ++up) {
                    if (d >= n) continue;
                    const uint64_t lo = CHUNK + 12345 + 7, hi = lo + d;
                    run_case(up ? hi : lo, up ? lo : hi, n, k, hi + n + CHUNK, up ? "up  " : "down");
                }
        // exact alias
        run_case(CHUNK + 5, CHUNK + 5, n, KEYS[0], 2 * CHUNK + n, "same");
    }

    // refusals, all before anything is queued
    {
        uint8_t *d = g_base + CHUNK, *s = g_base + CHUNK + 100;
        const uint64_t n = 200000, w = modgpu_move_workspace_bytes(n);
        std::memcpy(g_base, g_orig.data(), 4 * CHUNK + n);
        const uint64_t before = launches();
        refuse("null destination", modgpu_rekey_move_device(nullptr, s, n, PS3, 0, PS4, 0, g_ws, g_ws_bytes, -1, nullptr));
        refuse("null source", modgpu_rekey_move_device(d, nullptr, n, PS3, 0, PS4, 0, g_ws, g_ws_bytes, -1, nullptr));
        refuse("null workspace", modgpu_rekey_move_device(d, s, n, PS3, 0, PS4, 0, nullptr, g_ws_bytes, -1, nullptr));
        refuse("misaligned workspace", modgpu_rekey_move_device(d, s, n, PS3, 0, PS4, 0, g_ws + 4, g_ws_bytes - 4, -1, nullptr));
        refuse("short workspace", modgpu_rekey_move_device(d, s, n, PS3, 0, PS4, 0, g_ws, w - 1, -1, nullptr));
        refuse("workspace meets the destination", modgpu_rekey_move_device(d, s, n, PS3, 0, PS4, 0, d + n - 8, w, -1, nullptr));
        refuse("workspace meets the source", modgpu_rekey_move_device(d, s, n, PS3, 0, PS4, 0, s + n - 4, w, -1, nullptr));
        refuse("workspace meets a disjoint call's source", modgpu_rekey_move_device(d, d + 2 * n, n, PS3, 0, PS4, 0, d + 2 * n - 8 - w + 16, w, -1, nullptr));
        std::vector<uint64_t> host_ws(w / 8 + 1);
        refuse("workspace that is not device memory", modgpu_rekey_move_device(d, s, n, PS3, 0, PS4, 0, host_ws.data(), w, -1, nullptr));
        refuse("2^24 chunks", modgpu_rekey_move_device(d, s, 1ull << 40, PS3, 0, PS4, 0, g_ws, ~0ull, -1, nullptr));
        refuse("2^24 chunks by the destination's phase", modgpu_rekey_move_device(d + 17, s, (1ull << 40) - 16, PS3, 0, PS4, 0, g_ws, ~0ull, -1, nullptr));
        uint64_t out = 0;
        refuse("status of a null workspace", modgpu_move_status(nullptr, -1, &out));
        refuse("status without an out pointer", modgpu_move_status(g_ws, -1, nullptr));
        refuse("status of host memory", modgpu_move_status(host_ws.data(), -1, &out));
        ++g_cases;
        const bool quiet = launches() == before && std::memcmp(g_base, g_orig.data(), 4 * CHUNK + n) == 0 &&
                           modgpu_rekey_move_device(nullptr, nullptr, 0, PS3, 0, PS4, 0, nullptr, 0, -1, nullptr) == MODGPU_OK;
        if (!quiet) ++g_failed;
        std::printf("%s refusals queued nothing and wrote nothing; n == 0 does nothing\n", quiet ? "ok  " : "FAIL");
    }

    ++g_cases;
    const bool plans = modgpu_shim_move_plan_errors() == 0 && modgpu_shim_rekey_plan_errors() == 0 && modgpu_shim_move_launches(0) > 0 && modgpu_shim_move_launches(1) > 0;
    if (!plans) ++g_failed;
    std::printf("%s launch plans: %llu move plan errors, %llu rekey plan errors, %llu plain and %llu funnel body launches\n", plans ? "ok  " : "FAIL",
                modgpu_shim_move_plan_errors(), modgpu_shim_rekey_plan_errors(), modgpu_shim_move_launches(0), modgpu_shim_move_launches(1));
    modgpu_shim_xfer_free(g_ws);
    modgpu_shim_xfer_free(raw);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
