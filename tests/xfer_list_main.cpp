// xfer_list_main.cpp -- the list transfers (modgpu_cycle_host_to_device_list, modgpu_cycle_device_to_host_list) on the CPU stand-in of the
// HIP runtime, as a program of its own (built by `make xfer-list-main` from the library's host sources, once with ASan + UBSan and once
// with TSan, runtimes linked statically; run directly by tests/test_xfer_list_cpu.py).  Every case lays its entries out in an arena of
// stand-in device memory and two arenas of host memory with guard bytes between them, runs the list up and down, and compares EVERY
// byte of all three arenas with a model computed here from lcg.h, byte by byte -- not from the device code or the stand-in's.  The lists
// of the GPU suite's long cases run here too, all but the 2 GiB entry -- every slot filled three times at chunks of one and two pieces,
// entries above 8 and 16 MiB, windows that begin and end inside an entry, 70 000 entries -- for the host half (fill_slot / drain_slot
// on reused slots, clipped windows, the big plan) and for the conditions those cases put on their inputs.  One `ok`
// line per case; nothing that depends on the run (addresses, times) is printed.  Exit status 0 = all of it held.
#include <algorithm>
#include <atomic>
#include <chrono>
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
unsigned long long modgpu_shim_xfer_list_launches(int upload);
unsigned long long modgpu_shim_xfer_list_plan_errors(void);
unsigned long long modgpu_shim_xfer_list_gave_up(void);
void modgpu_shim_wedge_next_xfer_list(int on);
void modgpu_shim_release_wedged_xfer_list(void);
}

namespace {
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
const int32_t KEYS[] = {PS4, PS3, 1, -1, INT32_MIN, 12345, 0x7FFFFFFF, 0}; // (the last two: the identity keystream)
constexpr uint64_t PERIOD = 0x7FFFFFFEull;
const uint64_t OFFSETS[] = {0, 5, (1ull << 32) + 5, PERIOD - 100, (1ull << 63) + 11, ~0ull - 2, 3 * PERIOD - 7};
constexpr uint64_t PIECE = 32768, GUARD = 24;
constexpr uint8_t DEV_FILL = 0xD5, HOST_FILL = 0x3C;

int g_failed = 0, g_cases = 0;
uint64_t g_chunk = 0; // the chunk of a call of the cases' size, as the library reports it (its host trace)

void report(const std::string &what, bool ok, const std::string &detail = "")
{
    ++g_cases;
    if (!ok) ++g_failed;
    std::printf("%s %s%s%s\n", ok ? "ok  " : "FAIL", what.c_str(), detail.empty() ? "" : " | ", detail.c_str());
    std::fflush(stdout);
}
uint64_t launches()
{
    modgpu_path_stats_t st;
    modgpu_path_stats(&st, 0);
    return st.gpu_launches;
}
uint64_t splitmix(uint64_t &x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
void model_xor(uint8_t *out, const uint8_t *in, uint64_t n, int32_t key, uint64_t off)
{
    const uint32_t r = lcg::key_residue(key);
    uint32_t s = r ? lcg::state_residue(r, off % PERIOD) : 0;
    for (uint64_t j = 0; j < n; ++j) {
        out[j] = r ? in[j] ^ (uint8_t)~s : in[j];
        if (r) s = lcg::mulmod(s, lcg::A);
    }
}

struct Spec { // one entry of a case: its bytes, key and offset, and the phases (mod 16) of its two sides
    uint64_t n;
    int32_t key;
    uint64_t off;
    uint32_t dev_phase, host_phase;
    bool null_ptrs = false; // (n == 0 only) both pointers NULL
};

// A case laid out: entry e's device side at dev + d_at[e], its plaintext at src + h_at[e], its download at back + h_at[e]
struct Layout {
    std::vector<Spec> specs;
    std::vector<uint64_t> d_at, h_at;
    uint64_t d_size = 0, h_size = 0;
    uint8_t *dev = nullptr;
    std::vector<uint8_t> src, back, want_dev;
    explicit Layout(std::vector<Spec> sp, int device = 0, uint64_t seed = 1) : specs(std::move(sp))
    {
        uint64_t d = 64, h = 64;
        for (const Spec &s : specs) {
            d = (d + GUARD + 15) / 16 * 16 + s.dev_phase;
            h = (h + GUARD + 15) / 16 * 16 + s.host_phase;
            d_at.push_back(d), h_at.push_back(h);
            d += s.n, h += s.n;
        }
        d_size = d + 64, h_size = h + 64;
        dev = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(d_size, device));
        std::memset(dev, DEV_FILL, d_size);
        src.assign(h_size, 0);
        for (auto &b : src) b = (uint8_t)splitmix(seed);
        back.assign(h_size, HOST_FILL);
        want_dev.assign(d_size, DEV_FILL);
        for (size_t e = 0; e < specs.size(); ++e) model_xor(&want_dev[d_at[e]], &src[h_at[e]], specs[e].n, specs[e].key, specs[e].off);
    }
    ~Layout() { if (dev) modgpu_shim_xfer_free(dev); }
    std::vector<modgpu_table_entry_t> table(bool upload)
    {
        std::vector<modgpu_table_entry_t> t;
        for (size_t e = 0; e < specs.size(); ++e) {
            const Spec &s = specs[e];
            void *d = s.null_ptrs ? nullptr : dev + d_at[e], *h = s.null_ptrs ? nullptr : (upload ? &src[h_at[e]] : &back[h_at[e]]);
            t.push_back(upload ? modgpu_table_entry_t{d, h, s.n, s.off, s.key, 0} : modgpu_table_entry_t{h, d, s.n, s.off, s.key, 0});
        }
        return t;
    }
    // what `back` must be after a download of the device image want_dev: the plaintext inside the entries, the fill around them
    std::vector<uint8_t> want_back() const
    {
        std::vector<uint8_t> w(h_size, HOST_FILL);
        for (size_t e = 0; e < specs.size(); ++e) std::memcpy(&w[h_at[e]], &src[h_at[e]], specs[e].n);
        return w;
    }
    uint64_t total() const
    {
        uint64_t t = 0;
        for (const Spec &s : specs) t += s.n;
        return t;
    }
};

// up, then down: every byte of the three arenas, the sources unchanged, one launch each way with the list variant
std::string round_trip(Layout &L, int device = 0, uint64_t expect_launches = 1)
{
    const std::vector<uint8_t> src_keep = L.src;
    const unsigned long long gave_up = modgpu_shim_xfer_list_gave_up(), perr = modgpu_shim_xfer_list_plan_errors(), up0 = modgpu_shim_xfer_list_launches(1), dn0 = modgpu_shim_xfer_list_launches(0);
    auto up = L.table(true);
    const auto up_keep = up;
    uint64_t l0 = launches();
    int rc = modgpu_cycle_host_to_device_list(up.data(), up.size(), device);
    if (rc != MODGPU_OK) return std::string("upload failed: ") + modgpu_last_error();
    const uint64_t want_l = L.total() ? expect_launches : 0;
    if (launches() - l0 != want_l || modgpu_shim_xfer_list_launches(1) - up0 != want_l) return "upload: launches " + std::to_string(launches() - l0);
    if (std::memcmp(L.dev, L.want_dev.data(), L.d_size) != 0) return "upload: the device image differs from the model";
    if (L.src != src_keep) return "upload: a source was written";
    if (!up.empty() && std::memcmp(up.data(), up_keep.data(), up.size() * sizeof up[0]) != 0) return "upload: the list was written";
    modgpu_launch_info_t li{};
    if (want_l && (modgpu_last_launch(&li) != MODGPU_OK || li.variant != 21 || !li.kernel || !std::strstr(li.kernel, "up funnel") ||
                   (expect_launches == 1 && li.bytes != L.total())))
        return "upload: last launch";
    auto dn = L.table(false);
    l0 = launches();
    rc = modgpu_cycle_device_to_host_list(dn.data(), dn.size(), device);
    if (rc != MODGPU_OK) return std::string("download failed: ") + modgpu_last_error();
    if (launches() - l0 != want_l || modgpu_shim_xfer_list_launches(0) - dn0 != want_l) return "download: launches " + std::to_string(launches() - l0);
    if (L.back != L.want_back()) return "download: the host image differs from the model";
    if (std::memcmp(L.dev, L.want_dev.data(), L.d_size) != 0) return "download: a source was written";
    if (want_l && (modgpu_last_launch(&li) != MODGPU_OK || li.variant != 21 || !li.kernel || !std::strstr(li.kernel, "down funnel"))) return "download: last launch";
    if (modgpu_shim_xfer_list_plan_errors() != perr) return "the stand-in refused a plan";
    if (modgpu_shim_xfer_list_gave_up() != gave_up) return "a stand-in launch gave up";
    return "";
}
void run_case(const std::string &what, std::vector<Spec> specs, uint64_t expect_launches = 1)
{
    Layout L(std::move(specs));
    const std::string err = round_trip(L, 0, expect_launches);
    report(what, err.empty(), err.empty() ? "entries=" + std::to_string(L.specs.size()) + " bytes=" + std::to_string(L.total()) : err);
}

// ---- the lists of the cases (tests/test_gpu_xfer_list.py builds the same ones) ---------------------------------------------------
std::vector<Spec> phases_and_sizes()
{
    const uint64_t sizes[] = {1, 15, 16, 17, 4095, 32767, 32768, 32769, 65536 + 17, 3 * 65536 + 77};
    std::vector<Spec> v;
    uint32_t k = 0;
    for (int rep = 0; rep < 5; ++rep)
        for (uint64_t n : sizes) {
            // the device phase walks 0..15 (k), the host phase against it by 0, 3, 5, 7, ...; the packed phase follows from the odd sizes
            v.push_back({n, KEYS[k % 8], OFFSETS[k % 7], k % 16, (k * 7 + (uint32_t)rep * 3) % 16});
            ++k;
        }
    return v;
}
std::vector<Spec> boundaries(uint64_t chunk)
{
    std::vector<Spec> v;
    uint64_t packed = 0;
    uint32_t k = 0;
    auto add = [&](uint64_t n) {
        v.push_back({n, KEYS[k % 6], OFFSETS[k % 7], (k * 5) % 16, (k * 3 + 1) % 16});
        packed += n, ++k;
    };
    auto end_at = [&](uint64_t p) { add(p - packed); }; // an entry that ends exactly at packed position p
    end_at(PIECE - 1), end_at(PIECE), end_at(2 * PIECE), end_at(3 * PIECE + 1); // boundaries one before, on, on, one behind a piece boundary
    const uint64_t c1 = (packed / chunk + 1) * chunk;
    end_at(c1 - 1), end_at(c1), end_at(c1 + chunk), end_at(c1 + 2 * chunk + 1); // the same around chunk boundaries
    add(3 * chunk + 4097);                                                      // one entry that spans more than three chunks
    const uint64_t p0 = (packed / PIECE + 1) * PIECE;
    end_at(p0 - 15000); // a run of 10 000 entries of 1..7 bytes (40 000 bytes) that crosses the piece boundary p0, and the next
    for (uint32_t i = 0; i < 10000; ++i) v.push_back({1 + i % 7, KEYS[i % 6], OFFSETS[i % 7] + i, i % 16, (i * 11) % 16}), packed += 1 + i % 7;
    add(777);
    return v;
}
std::vector<Spec> with_empties()
{
    std::vector<Spec> v;
    const Spec nul{0, PS4, 0, 0, 0, true}, empty{0, PS3, 9, 3, 5, false};
    v.push_back(nul), v.push_back(empty), v.push_back(nul);
    v.push_back({70000, PS4, 17, 1, 2});
    v.push_back(nul), v.push_back(nul), v.push_back(empty);
    v.push_back({5, PS3, (1ull << 40) + 3, 15, 0});
    v.push_back(nul);
    v.push_back({PIECE + 3, 1, 0, 7, 9});
    v.push_back(empty), v.push_back(nul);
    return v;
}

// ---- the lists of the GPU suite's cases past one round of the slots, 8 MiB and 65 535 records (the same ones, but the 2 GiB entry) --
constexpr uint64_t PIPES_MOST = 8, SLOT_ROUNDS = 3; // the pipelines a call can have (MODGPU_HOST_PIPES' default), two slots each
uint64_t total_of(const std::vector<Spec> &v)
{
    uint64_t t = 0;
    for (const Spec &s : v) t += s.n;
    return t;
}
// `specs` behind as many copies of phases_and_sizes() as it takes for ceil(total / chunk) >= 3 x 2 x 8, the copies padded to a whole
// number of chunks: every packed position of `specs` keeps its place in its piece and its chunk, in a slot that has been used before
std::vector<Spec> refilled(const std::vector<Spec> &specs, uint64_t chunk)
{
    std::vector<Spec> head;
    while (total_of(specs) + total_of(head) < SLOT_ROUNDS * 2 * PIPES_MOST * chunk)
        for (const Spec &s : phases_and_sizes()) head.push_back(s);
    const uint64_t pad = (chunk - total_of(head) % chunk) % chunk;
    if (pad) head.push_back({pad, KEYS[1], OFFSETS[2], 9, 4});
    head.insert(head.end(), specs.begin(), specs.end());
    return head;
}
std::vector<Spec> long_entries() // ~32 MiB, entries above 8 and above 16 MiB: the kernel's second jump table at the indices 1 and 2
{
    return {{13, KEYS[1], 5, 3, 7},
            {(8ull << 20) + 3 * PIECE + 77, KEYS[0], ~0ull - 2, 5, 11},
            {4097, KEYS[2], (1ull << 32) + 5, 0, 9},
            {(16ull << 20) + PIECE + 1, KEYS[1], PERIOD - 100, 12, 1},
            {(8ull << 20) + 5, 0x7FFFFFFF, 3, 7, 14}};
}
std::vector<Spec> seventy_thousand() // 70 000 entries of 1..7 bytes, one of 40 000 bytes in the middle, empty and NULL entries scattered in
{
    std::vector<Spec> v;
    for (uint32_t i = 0; i < 70000; ++i) {
        if (i == 35000) v.push_back({40000, KEYS[1], OFFSETS[2], 5, 11});
        if (i % 9973 == 17) v.push_back((i / 9973) % 2 ? Spec{0, PS4, 0, 0, 0, true} : Spec{0, PS3, 9, 3, 5, false});
        v.push_back({1 + i % 7, KEYS[i % 6], OFFSETS[i % 7] + i, i % 16, (i * 11) % 16});
    }
    return v;
}
// per non-empty entry, the largest `steps` -- whole 32 KiB steps from a record's first byte to a segment's -- the kernel computes for it:
// pieces are cut from each window's first byte, a window's first record begins where the window does, a segment begins at a record's
// first byte or on a piece boundary
std::vector<uint64_t> most_steps(const std::vector<Spec> &specs, uint64_t most = 0)
{
    std::vector<uint64_t> out;
    const uint64_t total = total_of(specs);
    uint64_t es = 0;
    for (const Spec &s : specs) {
        if (!s.n) continue;
        uint64_t top = 0;
        for (uint64_t at = most ? es - es % most : 0; at < es + s.n; at += most) {
            const uint64_t first = std::max(es, at), end = std::min(es + s.n, most ? at + most : total);
            const uint64_t last_piece = at + (end - 1 - at) / PIECE * PIECE;
            if (last_piece > first) top = std::max(top, (last_piece - first) / PIECE);
            if (!most) break;
        }
        out.push_back(top);
        es += s.n;
    }
    return out;
}
struct SlotsEvent { // a window's `slots` event of the host trace
    uint64_t pipes, chunk;
};
// round_trip with the host trace on: the `slots` event of every window, both ways
std::string traced_round_trip(Layout &L, uint64_t expect_launches, std::vector<SlotsEvent> &slots)
{
    modgpu_host_trace(1);
    const std::string err = round_trip(L, 0, expect_launches);
    modgpu_host_trace(0);
    std::vector<modgpu_host_trace_event_t> ev((size_t)std::max(modgpu_host_trace_read(nullptr, 0), 1));
    const int n = std::min<int>(modgpu_host_trace_read(ev.data(), (int)ev.size()), (int)ev.size());
    slots.clear();
    for (int i = 0; i < n; ++i)
        if (ev[i].kind == MODGPU_TRACE_SLOTS) slots.push_back({ev[i].chunk, ev[i].bytes});
    return err;
}
// every window's chunk is `chunk` (0: whatever the library chose) and fills every slot of its pipelines at least three times
std::string three_rounds(const std::vector<SlotsEvent> &slots, uint64_t total, uint64_t chunk)
{
    if (slots.size() != 2) return "slots events: " + std::to_string(slots.size());
    for (const SlotsEvent &s : slots) {
        if (chunk && s.chunk != chunk) return "chunk " + std::to_string(s.chunk) + ", not " + std::to_string(chunk);
        if (s.pipes < 2 || (total + s.chunk - 1) / s.chunk < SLOT_ROUNDS * 2 * s.pipes)
            return "slots are not filled three times: " + std::to_string((total + s.chunk - 1) / s.chunk) + " chunks on " + std::to_string(s.pipes) + " pipelines";
    }
    return "";
}

void every_slot_refilled()
{
    // a call of 8 MiB or less takes chunks of HALF the feed chunk, at least a piece: 32 and 64 KiB give one piece, 128 KiB two
    const uint64_t knobs[][2] = {{32u << 10, 32u << 10}, {64u << 10, 32u << 10}, {128u << 10, 64u << 10}};
    for (const auto &k : knobs) {
        modgpu_debug_set_host_tunable(MODGPU_TUNABLE_FEED_CHUNK_BYTES, k[0]);
        for (int which = 0; which < 2; ++which) {
            Layout L(refilled(which ? boundaries(k[1]) : phases_and_sizes(), k[1]));
            std::vector<SlotsEvent> slots;
            std::string err = traced_round_trip(L, 1, slots);
            if (err.empty()) err = three_rounds(slots, L.total(), k[1]);
            if (err.empty() && L.total() > (8ull << 20)) err = "the list is above 8 MiB";
            report("every slot refilled: feed chunk " + std::to_string(k[0]) + ", chunks of " + std::to_string(k[1]) + ", " + (which ? "boundaries" : "phases and sizes"),
                   err.empty(), err.empty() ? "bytes=" + std::to_string(L.total()) : err);
        }
    }
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_FEED_CHUNK_BYTES, 256u << 10);
}

void entries_longer_than_8_mib()
{
    Layout L(long_entries());
    const std::vector<uint64_t> steps = most_steps(L.specs);
    std::vector<SlotsEvent> slots;
    std::string err = steps[1] >> 8 == 1 && (steps[1] & 255) < 255 && steps[3] >> 8 == 2 ? "" : "the entries do not reach the second jump table's indices 1 and 2";
    if (err.empty()) err = traced_round_trip(L, 1, slots);
    if (err.empty()) err = three_rounds(slots, L.total(), 0);
    report("entries longer than 8 MiB", err.empty(), err.empty() ? "bytes=" + std::to_string(L.total()) : err);
}

bool error_names(uint64_t entry, const char *what)
{
    const std::string e = modgpu_last_error();
    return e.find("entry " + std::to_string(entry) + ":") == 0 && e.find(what) != std::string::npos;
}

void refusals()
{
    Layout L({{1000, PS4, 0, 1, 2}, {2000, PS3, 5, 3, 4}, {0, PS4, 0, 0, 0, true}, {3000, 1, 7, 5, 6}, {4000, PS4, 9, 7, 8}});
    const std::vector<uint8_t> src_keep = L.src, back_keep = L.back;
    std::vector<uint8_t> dev_keep(L.dev, L.dev + L.d_size);
    const uint64_t l0 = launches();
    const unsigned long long s0 = modgpu_shim_xfer_list_launches(0) + modgpu_shim_xfer_list_launches(1);
    for (int upload = 1; upload >= 0; --upload) {
        const std::string dir = upload ? "up" : "down";
        auto call = [&](std::vector<modgpu_table_entry_t> &t, uint64_t n) {
            return upload ? modgpu_cycle_host_to_device_list(t.data(), n, 0) : modgpu_cycle_device_to_host_list(t.data(), n, 0);
        };
        auto t = L.table(upload);
        int rc = upload ? modgpu_cycle_host_to_device_list(nullptr, 3, 0) : modgpu_cycle_device_to_host_list(nullptr, 3, 0);
        report("refusal " + dir + ": null list", rc == MODGPU_ERR_INVALID && std::strstr(modgpu_last_error(), "NULL list"));
        rc = call(t, (uint64_t)MODGPU_TABLE_MAX_ENTRIES + 1);
        report("refusal " + dir + ": too many entries", rc == MODGPU_ERR_INVALID && std::strstr(modgpu_last_error(), "more than 4194304 entries"));
        t = L.table(upload), t[3].dst = nullptr;
        report("refusal " + dir + ": null dst", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(3, "NULL pointer"));
        t = L.table(upload), t[1].src = nullptr, t[4].src = nullptr;
        report("refusal " + dir + ": null src, the lowest of two", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(1, "NULL pointer"));
        t = L.table(upload), t[2].flags = 1; // (an empty entry's flags count too)
        report("refusal " + dir + ": flags", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(2, "nonzero flags"));
        t = L.table(upload), t[4].n = 1ull << 39;
        report("refusal " + dir + ": 2^39 bytes", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(4, "2^39 bytes"));
        t = L.table(upload), (upload ? t[3].dst : const_cast<void *&>(t[3].src)) = L.back.data() + 64; // host memory as the device side
        report("refusal " + dir + ": host memory as the device side", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(3, "not device memory"));
        t = L.table(upload), t[4].n = L.d_size; // runs off the end of its allocation
        report("refusal " + dir + ": device range past its allocation", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(4, "not device memory"));
        t = L.table(upload), t[4].flags = 2, (upload ? t[1].dst : const_cast<void *&>(t[1].src)) = L.src.data();
        report("refusal " + dir + ": a device side below a flagged entry", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(1, "not device memory"));
        t = L.table(upload), t[0].flags = 2, (upload ? t[1].dst : const_cast<void *&>(t[1].src)) = L.src.data();
        report("refusal " + dir + ": a flagged entry below a device side", call(t, t.size()) == MODGPU_ERR_INVALID && error_names(0, "nonzero flags"));
        t = L.table(upload);
        rc = upload ? modgpu_cycle_host_to_device_list(t.data(), t.size(), 63) : modgpu_cycle_device_to_host_list(t.data(), t.size(), 63);
        report("refusal " + dir + ": a device that does not exist", rc != MODGPU_OK);
    }
    const bool quiet = launches() == l0 && modgpu_shim_xfer_list_launches(0) + modgpu_shim_xfer_list_launches(1) == s0 && L.src == src_keep && L.back == back_keep &&
                       std::memcmp(L.dev, dev_keep.data(), L.d_size) == 0;
    report("refusals queued nothing and wrote nothing", quiet);
    // ... and the next call is clean
    L.back = back_keep;
    std::memset(L.dev, DEV_FILL, L.d_size);
    const std::string err = round_trip(L);
    report("a good list after the refusals", err.empty(), err);
}

void same_bytes_as_the_loop()
{
    Layout A(phases_and_sizes(), 0, 7), B(phases_and_sizes(), 0, 7);
    auto ta = A.table(true), tb = B.table(true);
    int rc = modgpu_cycle_host_to_device_list(ta.data(), ta.size(), 0);
    for (size_t e = 0; e < tb.size() && rc == MODGPU_OK; ++e)
        rc = modgpu_cycle_host_to_device(tb[e].dst, static_cast<const uint8_t *>(tb[e].src), tb[e].n, tb[e].key, tb[e].stream_off, 0);
    bool ok = rc == MODGPU_OK && A.d_size == B.d_size && std::memcmp(A.dev, B.dev, A.d_size) == 0;
    ta = A.table(false), tb = B.table(false);
    rc = modgpu_cycle_device_to_host_list(ta.data(), ta.size(), 0);
    for (size_t e = 0; e < tb.size() && rc == MODGPU_OK; ++e)
        rc = modgpu_cycle_device_to_host(static_cast<uint8_t *>(tb[e].dst), tb[e].src, tb[e].n, tb[e].key, tb[e].stream_off, 0);
    ok = ok && rc == MODGPU_OK && A.back == B.back;
    report("same bytes as the single calls one by one, both ways", ok);
}

void shared_sources()
{
    // one host range to three destinations under three keys; then one device range to two host destinations
    const uint64_t n = 2 * PIECE + 301;
    Layout L({{n, PS4, 3, 1, 5}, {n, PS3, (1ull << 33), 9, 5}, {n, 0, 0, 14, 5}});
    auto up = L.table(true);
    up[1].src = up[0].src, up[2].src = up[0].src;
    for (size_t e = 0; e < 3; ++e) model_xor(&L.want_dev[L.d_at[e]], &L.src[L.h_at[0]], n, L.specs[e].key, L.specs[e].off);
    bool ok = modgpu_cycle_host_to_device_list(up.data(), 3, 0) == MODGPU_OK && std::memcmp(L.dev, L.want_dev.data(), L.d_size) == 0;
    auto dn = L.table(false);
    dn.resize(2);
    dn[1].src = dn[0].src, dn[1].key = dn[0].key, dn[1].stream_off = dn[0].stream_off;
    std::vector<uint8_t> want(L.h_size, HOST_FILL);
    for (size_t e = 0; e < 2; ++e) std::memcpy(&want[L.h_at[e]], &L.src[L.h_at[0]], n);
    ok = ok && modgpu_cycle_device_to_host_list(dn.data(), 2, 0) == MODGPU_OK && L.back == want;
    report("shared sources, both ways", ok);
}

void injected_failures()
{
    for (int upload = 1; upload >= 0; --upload)
        for (int64_t piece : {(int64_t)0, (int64_t)MODGPU_INJECT_PIECE_MIDDLE, (int64_t)MODGPU_INJECT_PIECE_LAST})
            for (int stage : {MODGPU_STAGE_FILL, MODGPU_STAGE_LAUNCH, MODGPU_STAGE_SYNC}) {
                Layout L(phases_and_sizes(), 0, 11);
                if (!upload) std::memcpy(L.dev, L.want_dev.data(), L.d_size);
                const std::vector<uint8_t> src_keep = L.src;
                auto t = L.table(upload);
                modgpu_debug_inject_failure_at(piece, stage);
                const int rc = upload ? modgpu_cycle_host_to_device_list(t.data(), t.size(), 0) : modgpu_cycle_device_to_host_list(t.data(), t.size(), 0);
                const bool fired = modgpu_debug_injection_armed() == 0;
                modgpu_debug_inject_failure_at(0, -1);
                bool ok = rc == MODGPU_ERR_HIP && fired && L.src == src_keep && (upload || std::memcmp(L.dev, L.want_dev.data(), L.d_size) == 0);
                std::memset(L.dev, DEV_FILL, L.d_size);
                std::fill(L.back.begin(), L.back.end(), HOST_FILL);
                const std::string err = round_trip(L); // the next call is clean
                ok = ok && err.empty();
                report(std::string("injected failure ") + (upload ? "up" : "down") + " piece " + std::to_string(piece) + " stage " + std::to_string(stage), ok, err);
            }
}

void two_threads()
{
    std::atomic<int> bad{0};
    auto work = [&](uint64_t seed) {
        for (int k = 0; k < 3; ++k) {
            Layout L(k == 1 ? with_empties() : phases_and_sizes(), 0, seed + (uint64_t)k);
            auto up = L.table(true);
            auto dn = L.table(false);
            if (modgpu_cycle_host_to_device_list(up.data(), up.size(), 0) != MODGPU_OK || std::memcmp(L.dev, L.want_dev.data(), L.d_size) != 0) ++bad;
            if (modgpu_cycle_device_to_host_list(dn.data(), dn.size(), 0) != MODGPU_OK || L.back != L.want_back()) ++bad;
        }
    };
    std::thread a(work, 100), b(work, 200);
    a.join(), b.join();
    report("two threads at once on separate buffers", bad.load() == 0);
}

void cut_above_the_limit()
{
    // the one-launch limit lowered to 300 000 bytes: the ~2 MiB of the phases list go in 7 launches, windows cut inside entries
    Layout probe(phases_and_sizes());
    const uint64_t most = 300000, want = (probe.total() + most - 1) / most;
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, most);
    run_case("cut above the one-launch limit: " + std::to_string(want) + " launches", phases_and_sizes(), want);
    run_case("cut above the one-launch limit, boundaries list", boundaries(g_chunk), (Layout(boundaries(g_chunk)).total() + most - 1) / most);
    // ... at three pieces: every window edge is a piece edge
    const uint64_t edge = 3 * PIECE;
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, edge);
    run_case("cut at three pieces, phases and sizes", phases_and_sizes(), (probe.total() + edge - 1) / edge);
    run_case("cut at three pieces, boundaries list", boundaries(g_chunk), (Layout(boundaries(g_chunk)).total() + edge - 1) / edge);
    // ... and the 32 MiB list at 5 MiB + 12345: windows that begin and end inside one entry, a clipped record's base from off + into
    {
        const uint64_t inside = (5ull << 20) + 12345;
        Layout L(long_entries());
        uint64_t es = 0;
        bool lies_inside = false;
        for (const Spec &s : L.specs) {
            for (uint64_t w = 0; w + inside < L.total(); w += inside) lies_inside = lies_inside || (es < w && w + inside < es + s.n);
            es += s.n;
        }
        modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, inside);
        std::string err = lies_inside ? round_trip(L, 0, (L.total() + inside - 1) / inside) : "no window lies inside one entry";
        report("cut inside long entries: " + std::to_string((L.total() + inside - 1) / inside) + " launches", err.empty(), err);
    } // (the same list in one launch: entries_longer_than_8_mib)
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, 0);
    run_case("one launch again with the limit back", phases_and_sizes());
}

void many_entries()
{
    Layout L(seventy_thousand());
    uint64_t records = 0, nulls = 0, empties = 0;
    for (const Spec &s : L.specs) records += s.n ? 1 : 0, nulls += s.null_ptrs ? 1 : 0, empties += !s.n && !s.null_ptrs ? 1 : 0;
    std::string err = records > 65535 && nulls >= 3 && empties >= 3 ? "" : "the list has no more than 65 535 records";
    if (err.empty()) err = round_trip(L);
    report("seventy thousand entries", err.empty(), err.empty() ? "records=" + std::to_string(records) + " bytes=" + std::to_string(L.total()) : err);
}

void wedged_kernel()
{
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_FEED_PATIENCE_MS, 100);
    Layout *L = new Layout(phases_and_sizes(), 0, 13); // (never freed: the lost call's memory stays out of circulation)
    const std::vector<uint8_t> src_keep = L->src;
    auto t = L->table(true);
    modgpu_shim_wedge_next_xfer_list(1);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = modgpu_cycle_host_to_device_list(t.data(), t.size(), 0);
    const double took = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const bool again = modgpu_cycle_host_to_device_list(t.data(), t.size(), 0) == MODGPU_ERR_HIP; // the device's routes stay abandoned
    modgpu_shim_release_wedged_xfer_list();
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_FEED_PATIENCE_MS, 10000);
    report("a wedged kernel: MODGPU_ERR_HIP within the host deadline, sources intact", rc == MODGPU_ERR_HIP && took < 4 * 0.1 + 1 + 20 && L->src == src_keep && again);
}
} // namespace

int main()
{
    // the chunk of a ~2 MiB call, as the library's host trace reports it
    {
        Layout L(phases_and_sizes());
        auto t = L.table(true);
        modgpu_host_trace(1);
        const int rc = modgpu_cycle_host_to_device_list(t.data(), t.size(), 0);
        modgpu_host_trace(0);
        std::vector<modgpu_host_trace_event_t> ev(4096);
        const int n = std::min<int>(modgpu_host_trace_read(ev.data(), (int)ev.size()), (int)ev.size());
        for (int i = 0; i < n; ++i)
            if (ev[i].kind == MODGPU_TRACE_SLOTS) g_chunk = ev[i].bytes;
        report("the chunk size from the host trace", rc == MODGPU_OK && g_chunk >= PIECE && g_chunk % PIECE == 0 && L.total() / g_chunk >= 12,
               "chunk=" + std::to_string(g_chunk) + " total=" + std::to_string(L.total()));
        if (!g_chunk) g_chunk = 4 * PIECE;
    }
    run_case("phases and sizes", phases_and_sizes());
    run_case("boundaries", boundaries(g_chunk));
    run_case("empty entries", with_empties());
    run_case("only empty entries", {{0, PS4, 0, 0, 0, true}, {0, PS3, 1, 2, 3, false}, {0, PS4, 0, 0, 0, true}});
    run_case("no entries", {});
    run_case("one byte", {{1, PS4, PERIOD - 1, 15, 15}});
    same_bytes_as_the_loop();
    shared_sources();
    refusals();
    injected_failures();
    two_threads();
    cut_above_the_limit();
    every_slot_refilled();
    entries_longer_than_8_mib();
    many_entries();
    wedged_kernel();
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
