// xfer_list_digest_main.cpp -- the digesting list transfers (modgpu_cycle_host_to_device_list_digest, modgpu_cycle_device_to_host_list_digest)
// on the CPU stand-in of the HIP runtime, as a program of its own (built by `make xfer-list-digest-main` from the library's host sources,
// once with ASan + UBSan and once with TSan, runtimes linked statically; run directly by tests/test_xfer_list_digest_cpu.py).  Every case
// lays its entries out as tests/xfer_list_main.cpp does -- an arena of stand-in device memory and two of host memory, guard bytes between
// the entries --, runs the list up and down under both sides, and compares EVERY record (n and the reserved word included) with the
// Adler-32 of a model computed here from lcg.h byte by byte, and every byte of the three arenas.  The lists are the GPU cases'
// (tests/test_gpu_xfer_list_digest.py).  Then every refusal, a call repeated on the same records, a failure injected at a middle chunk
// and the cut into windows with a clipped entry.  One `ok` line per case; nothing that depends on the run is printed.
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
unsigned long long modgpu_shim_xfer_list_digest_launches(int upload);
unsigned long long modgpu_shim_xfer_list_digest_plan_errors(void);
unsigned long long modgpu_shim_xfer_list_digest_gave_up(void);
unsigned long long modgpu_shim_xfer_list_launches(int upload);
}

namespace {
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB;
const int32_t KEYS[] = {PS4, PS3, 1, -1, INT32_MIN, 12345, 0x7FFFFFFF, 0}; // (the last two: the identity keystream)
constexpr uint64_t PERIOD = 0x7FFFFFFEull;
const uint64_t OFFSETS[] = {0, 5, (1ull << 32) + 5, PERIOD - 100, (1ull << 63) + 11, ~0ull - 2, 3 * PERIOD - 7};
constexpr uint64_t PIECE = 32768, GUARD = 24, ADLER = 65521;
constexpr uint8_t DEV_FILL = 0xD5, HOST_FILL = 0x3C, REC_FILL = 0xA7;

int g_failed = 0, g_cases = 0;
uint64_t g_chunk = 0;

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
uint32_t adler32(const uint8_t *p, uint64_t n) // as zlib defines it, byte by byte
{
    uint32_t a = 1, b = 0;
    for (uint64_t j = 0; j < n; ++j) {
        a = (a + p[j]) % ADLER;
        b = (b + a) % ADLER;
    }
    return b << 16 | a;
}

struct Spec {
    uint64_t n;
    int32_t key;
    uint64_t off;
    uint32_t dev_phase, host_phase;
    bool null_ptrs = false;
    int fill = -1; // >= 0: every source byte is this
};

struct Layout {
    std::vector<Spec> specs;
    std::vector<uint64_t> d_at, h_at;
    uint64_t d_size = 0, h_size = 0;
    uint8_t *dev = nullptr;
    modgpu_digest_result_t *records = nullptr; // stand-in device memory: one per entry and a guard record at either end
    std::vector<uint8_t> src, back, want_dev;
    explicit Layout(std::vector<Spec> sp, uint64_t seed = 1) : specs(std::move(sp))
    {
        uint64_t d = 64, h = 64;
        for (const Spec &s : specs) {
            d = (d + GUARD + 15) / 16 * 16 + s.dev_phase;
            h = (h + GUARD + 15) / 16 * 16 + s.host_phase;
            d_at.push_back(d), h_at.push_back(h);
            d += s.n, h += s.n;
        }
        d_size = d + 64, h_size = h + 64;
        dev = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(d_size, 0));
        std::memset(dev, DEV_FILL, d_size);
        records = static_cast<modgpu_digest_result_t *>(modgpu_shim_xfer_alloc((specs.size() + 2) * sizeof *records, 0));
        std::memset(records, REC_FILL, (specs.size() + 2) * sizeof *records);
        src.assign(h_size, 0);
        for (auto &b : src) b = (uint8_t)splitmix(seed);
        for (size_t e = 0; e < specs.size(); ++e)
            if (specs[e].fill >= 0) std::memset(&src[h_at[e]], specs[e].fill, specs[e].n);
        back.assign(h_size, HOST_FILL);
        want_dev.assign(d_size, DEV_FILL);
        for (size_t e = 0; e < specs.size(); ++e) model_xor(&want_dev[d_at[e]], &src[h_at[e]], specs[e].n, specs[e].key, specs[e].off);
    }
    ~Layout()
    {
        if (dev) modgpu_shim_xfer_free(dev);
        if (records) modgpu_shim_xfer_free(records);
    }
    Layout(const Layout &) = delete;
    modgpu_digest_result_t *recs() { return records + 1; }
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
    // the records against the model: `plain` = the records are of the plaintext (src), else of the ciphertext (want_dev)
    std::string records_wrong(bool plain)
    {
        const std::vector<uint8_t> guard(sizeof *records, REC_FILL);
        if (std::memcmp(records, guard.data(), guard.size()) != 0 || std::memcmp(records + 1 + specs.size(), guard.data(), guard.size()) != 0) return "a record outside the list was written";
        for (size_t e = 0; e < specs.size(); ++e) {
            const modgpu_digest_result_t &r = recs()[e];
            if (r.n != specs[e].n || r.reserved != 0) return "record " + std::to_string(e) + ": n or the reserved word";
            if (specs[e].n == 0 && (r.s1 != 0 || r.s2 != 0)) return "record " + std::to_string(e) + ": an empty entry's sums";
            const uint32_t want = adler32(plain ? &src[h_at[e]] : &want_dev[d_at[e]], specs[e].n);
            if (modgpu_digest_adler32(&r) != want) return "record " + std::to_string(e) + ": Adler-32 differs from the model";
        }
        return "";
    }
};

// up, then down, under `side`: every record, every byte of the three arenas, the sources unchanged, the launches with the digest variant
std::string round_trip(Layout &L, uint32_t side, uint64_t expect_launches = 1)
{
    const std::vector<uint8_t> src_keep = L.src;
    const unsigned long long gave_up = modgpu_shim_xfer_list_digest_gave_up(), perr = modgpu_shim_xfer_list_digest_plan_errors(), up0 = modgpu_shim_xfer_list_digest_launches(1),
                             dn0 = modgpu_shim_xfer_list_digest_launches(0), plain0 = modgpu_shim_xfer_list_launches(0) + modgpu_shim_xfer_list_launches(1);
    auto up = L.table(true);
    uint64_t l0 = launches();
    int rc = modgpu_cycle_host_to_device_list_digest(up.data(), up.size(), side, L.recs(), 0);
    if (rc != MODGPU_OK) return std::string("upload failed: ") + modgpu_last_error();
    const uint64_t want_l = L.total() ? expect_launches : 0;
    if (launches() - l0 != want_l || modgpu_shim_xfer_list_digest_launches(1) - up0 != want_l) return "upload: launches " + std::to_string(launches() - l0);
    if (std::memcmp(L.dev, L.want_dev.data(), L.d_size) != 0) return "upload: the device image differs from the model";
    if (L.src != src_keep) return "upload: a source was written";
    std::string err = L.specs.empty() ? "" : L.records_wrong(side == MODGPU_DIGEST_INPUT); // (an upload reads the plaintext and stores the ciphertext)
    if (!err.empty()) return "upload: " + err;
    modgpu_launch_info_t li{};
    if (want_l && (modgpu_last_launch(&li) != MODGPU_OK || li.variant != 22 || !li.kernel || !std::strstr(li.kernel, "up funnel") || (expect_launches == 1 && li.bytes != L.total())))
        return "upload: last launch";
    if (!L.specs.empty()) std::memset(L.records, REC_FILL, (L.specs.size() + 2) * sizeof *L.records);
    auto dn = L.table(false);
    l0 = launches();
    rc = modgpu_cycle_device_to_host_list_digest(dn.data(), dn.size(), side, L.recs(), 0);
    if (rc != MODGPU_OK) return std::string("download failed: ") + modgpu_last_error();
    if (launches() - l0 != want_l || modgpu_shim_xfer_list_digest_launches(0) - dn0 != want_l) return "download: launches " + std::to_string(launches() - l0);
    if (L.back != L.want_back()) return "download: the host image differs from the model";
    if (std::memcmp(L.dev, L.want_dev.data(), L.d_size) != 0) return "download: a source was written";
    err = L.specs.empty() ? "" : L.records_wrong(side == MODGPU_DIGEST_OUTPUT); // (a download reads the ciphertext and stores the plaintext)
    if (!err.empty()) return "download: " + err;
    if (want_l && (modgpu_last_launch(&li) != MODGPU_OK || li.variant != 22 || !li.kernel || !std::strstr(li.kernel, "down funnel"))) return "download: last launch";
    if (modgpu_shim_xfer_list_digest_plan_errors() != perr) return "the stand-in refused a plan";
    if (modgpu_shim_xfer_list_digest_gave_up() != gave_up) return "a stand-in launch gave up";
    if (modgpu_shim_xfer_list_launches(0) + modgpu_shim_xfer_list_launches(1) != plain0) return "a plain list launch was made";
    return "";
}
void run_case(const std::string &what, const std::vector<Spec> &specs, uint64_t expect_launches = 1)
{
    for (uint32_t side : {MODGPU_DIGEST_OUTPUT, MODGPU_DIGEST_INPUT}) {
        Layout L(specs);
        const std::string err = round_trip(L, side, expect_launches);
        report(what + (side ? ", side input" : ", side output"), err.empty(), err.empty() ? "entries=" + std::to_string(L.specs.size()) + " bytes=" + std::to_string(L.total()) : err);
    }
}

// ---- the lists of the cases (tests/test_gpu_xfer_list_digest.py builds the same ones, the first three as tests/test_gpu_xfer_list.py) ----
std::vector<Spec> phases_and_sizes()
{
    const uint64_t sizes[] = {1, 15, 16, 17, 4095, 32767, 32768, 32769, 65536 + 17, 3 * 65536 + 77};
    std::vector<Spec> v;
    uint32_t k = 0;
    for (int rep = 0; rep < 5; ++rep)
        for (uint64_t n : sizes) {
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
    auto end_at = [&](uint64_t p) { add(p - packed); };
    end_at(PIECE - 1), end_at(PIECE), end_at(2 * PIECE), end_at(3 * PIECE + 1);
    const uint64_t c1 = (packed / chunk + 1) * chunk;
    end_at(c1 - 1), end_at(c1), end_at(c1 + chunk), end_at(c1 + 2 * chunk + 1);
    add(3 * chunk + 4097);
    const uint64_t p0 = (packed / PIECE + 1) * PIECE;
    end_at(p0 - 15000);
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
std::vector<Spec> long_entries()
{
    return {{13, KEYS[1], 5, 3, 7},
            {(8ull << 20) + 3 * PIECE + 77, KEYS[0], ~0ull - 2, 5, 11},
            {4097, KEYS[2], (1ull << 32) + 5, 0, 9},
            {(16ull << 20) + PIECE + 1, KEYS[1], PERIOD - 100, 12, 1},
            {(8ull << 20) + 5, 0x7FFFFFFF, 3, 7, 14}};
}
std::vector<Spec> all_ones() { return {{4 * PIECE + 77, PS4, 5, 3, 9, false, 0xFF}}; } // the largest sums a lane, a wave and a record can meet
std::vector<Spec> wraps_twice() { return {{2 * ADLER + 5, PS3, 7, 11, 2}}; }           // the position passes 65521 twice
std::vector<Spec> tiny_entries()
{
    std::vector<Spec> v;
    for (uint32_t i = 0; i < 10000; ++i) v.push_back({1 + i % 7, KEYS[i % 6], OFFSETS[i % 7] + i, i % 16, (i * 11) % 16});
    return v;
}

void refusals()
{
    Layout L({{1000, PS4, 0, 1, 2}, {2000, PS3, 5, 3, 4}, {0, PS4, 0, 0, 0, true}, {3000, 1, 7, 5, 6}, {4000, PS4, 9, 7, 8}});
    const std::vector<uint8_t> src_keep = L.src, back_keep = L.back;
    std::vector<uint8_t> dev_keep(L.dev, L.dev + L.d_size), rec_keep((uint8_t *)L.records, (uint8_t *)(L.records + L.specs.size() + 2));
    std::vector<modgpu_digest_result_t> host_records(L.specs.size());
    const uint64_t l0 = launches();
    const unsigned long long s0 = modgpu_shim_xfer_list_digest_launches(0) + modgpu_shim_xfer_list_digest_launches(1);
    for (int upload = 1; upload >= 0; --upload) {
        const std::string dir = upload ? "up" : "down";
        auto call = [&](const modgpu_table_entry_t *t, uint64_t n, uint32_t side, modgpu_digest_result_t *r, int device = 0) {
            return upload ? modgpu_cycle_host_to_device_list_digest(t, n, side, r, device) : modgpu_cycle_device_to_host_list_digest(t, n, side, r, device);
        };
        auto refused = [&](const char *text) { return std::strstr(modgpu_last_error(), text) != nullptr; };
        auto names = [&](uint64_t entry, const char *what) {
            const std::string e = modgpu_last_error();
            return e.find("entry " + std::to_string(entry) + ":") == 0 && e.find(what) != std::string::npos;
        };
        auto t = L.table(upload);
        report("refusal " + dir + ": null list", call(nullptr, 3, 0, L.recs()) == MODGPU_ERR_INVALID && refused("NULL list"));
        report("refusal " + dir + ": too many entries", call(t.data(), (uint64_t)MODGPU_TABLE_MAX_ENTRIES + 1, 0, L.recs()) == MODGPU_ERR_INVALID && refused("more than 4194304 entries"));
        report("refusal " + dir + ": null records", call(t.data(), t.size(), 0, nullptr) == MODGPU_ERR_INVALID && refused("NULL records"));
        report("refusal " + dir + ": misaligned records",
               call(t.data(), t.size(), 0, reinterpret_cast<modgpu_digest_result_t *>(reinterpret_cast<uint8_t *>(L.recs()) + 4)) == MODGPU_ERR_INVALID && refused("not 8-byte aligned"));
        report("refusal " + dir + ": a third side", call(t.data(), t.size(), 2, L.recs()) == MODGPU_ERR_INVALID && refused("a side other than"));
        report("refusal " + dir + ": host memory as records", call(t.data(), t.size(), 1, host_records.data()) == MODGPU_ERR_INVALID && refused("records are not device memory"));
        report("refusal " + dir + ": records past their allocation", call(t.data(), t.size(), 0, L.recs() + 2) == MODGPU_ERR_INVALID && refused("records are not device memory"));
        // records inside entry 3's device range (the arena is large enough to hold them there: 5 x 32 bytes at an 8-byte aligned address)
        modgpu_digest_result_t *inside = reinterpret_cast<modgpu_digest_result_t *>(L.dev + (L.d_at[3] + 7) / 8 * 8);
        report("refusal " + dir + ": records inside an entry's device range", call(t.data(), t.size(), 0, inside) == MODGPU_ERR_INVALID && names(3, "meets the records"));
        t = L.table(upload), t[3].dst = nullptr;
        report("refusal " + dir + ": null dst", call(t.data(), t.size(), 0, L.recs()) == MODGPU_ERR_INVALID && names(3, "NULL pointer"));
        t = L.table(upload), t[2].flags = 1;
        report("refusal " + dir + ": flags", call(t.data(), t.size(), 1, L.recs()) == MODGPU_ERR_INVALID && names(2, "nonzero flags"));
        t = L.table(upload), t[4].n = 1ull << 39;
        report("refusal " + dir + ": 2^39 bytes", call(t.data(), t.size(), 0, L.recs()) == MODGPU_ERR_INVALID && names(4, "2^39 bytes"));
        t = L.table(upload), (upload ? t[3].dst : const_cast<void *&>(t[3].src)) = L.back.data() + 64;
        report("refusal " + dir + ": host memory as the device side", call(t.data(), t.size(), 0, L.recs()) == MODGPU_ERR_INVALID && names(3, "not device memory"));
        t = L.table(upload);
        report("refusal " + dir + ": a device that does not exist", call(t.data(), t.size(), 0, L.recs(), 63) != MODGPU_OK);
        report("no entries " + dir + ": nothing touched", call(nullptr, 0, 7, nullptr) == MODGPU_OK);
    }
    const bool quiet = launches() == l0 && modgpu_shim_xfer_list_digest_launches(0) + modgpu_shim_xfer_list_digest_launches(1) == s0 && L.src == src_keep && L.back == back_keep &&
                       std::memcmp(L.dev, dev_keep.data(), L.d_size) == 0 && std::memcmp(L.records, rec_keep.data(), rec_keep.size()) == 0;
    report("refusals queued nothing and wrote nothing", quiet);
    const std::string err = round_trip(L, MODGPU_DIGEST_INPUT);
    report("a good list after the refusals", err.empty(), err);
}

void only_empty_entries()
{
    Layout L({{0, PS4, 0, 0, 0, true}, {0, PS3, 1, 2, 3, false}, {0, PS4, 0, 0, 0, true}});
    const std::string err = round_trip(L, MODGPU_DIGEST_OUTPUT, 0); // (no launch; the records are written all the same)
    report("only empty entries: records written, nothing launched", err.empty(), err);
}

void twice_on_the_same_records()
{
    Layout L(phases_and_sizes(), 5);
    auto up = L.table(true);
    bool ok = modgpu_cycle_host_to_device_list_digest(up.data(), up.size(), MODGPU_DIGEST_OUTPUT, L.recs(), 0) == MODGPU_OK;
    std::vector<modgpu_digest_result_t> first(L.recs(), L.recs() + L.specs.size());
    for (auto &r : first) r.s1 %= ADLER, r.s2 %= ADLER;
    ok = ok && modgpu_cycle_host_to_device_list_digest(up.data(), up.size(), MODGPU_DIGEST_OUTPUT, L.recs(), 0) == MODGPU_OK && L.records_wrong(false).empty();
    for (size_t e = 0; e < first.size() && ok; ++e) {
        const modgpu_digest_result_t &r = L.recs()[e];
        ok = r.s1 % ADLER == first[e].s1 && r.s2 % ADLER == first[e].s2 && r.n == first[e].n && r.reserved == 0;
    }
    report("the call twice on the same records: the same records", ok);
}

void injected_failure_in_the_middle()
{
    for (int upload = 1; upload >= 0; --upload) {
        Layout L(phases_and_sizes(), 11);
        if (!upload) std::memcpy(L.dev, L.want_dev.data(), L.d_size);
        const std::vector<uint8_t> src_keep = L.src;
        auto t = L.table(upload);
        modgpu_debug_inject_failure_at(MODGPU_INJECT_PIECE_MIDDLE, MODGPU_STAGE_SYNC);
        const int rc = upload ? modgpu_cycle_host_to_device_list_digest(t.data(), t.size(), 0, L.recs(), 0) : modgpu_cycle_device_to_host_list_digest(t.data(), t.size(), 0, L.recs(), 0);
        const bool fired = modgpu_debug_injection_armed() == 0;
        modgpu_debug_inject_failure_at(0, -1);
        bool ok = rc == MODGPU_ERR_HIP && fired && L.src == src_keep && (upload || std::memcmp(L.dev, L.want_dev.data(), L.d_size) == 0);
        std::memset(L.dev, DEV_FILL, L.d_size);
        std::fill(L.back.begin(), L.back.end(), HOST_FILL);
        const std::string err = round_trip(L, MODGPU_DIGEST_OUTPUT); // the next call is clean, on the records the failed one left
        report(std::string("injected failure at a middle chunk, ") + (upload ? "up" : "down"), ok && err.empty(), err);
    }
}

void cut_into_windows()
{
    for (uint64_t most : {(uint64_t)300000, 3 * PIECE}) {
        const std::vector<Spec> specs = phases_and_sizes();
        uint64_t total = 0, es = 0;
        bool clipped = false;
        for (const Spec &s : specs) total += s.n;
        for (const Spec &s : specs) {
            for (uint64_t w = most; w < total; w += most) clipped = clipped || (es < w && w < es + s.n);
            es += s.n;
        }
        modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, most);
        if (!clipped) report("cut into windows of " + std::to_string(most), false, "no entry is clipped by a window");
        else run_case("cut into windows of " + std::to_string(most) + ": " + std::to_string((total + most - 1) / most) + " launches, a clipped entry", specs, (total + most - 1) / most);
    }
    {
        const uint64_t inside = (5ull << 20) + 12345; // windows that begin and end inside one entry: skip_mod of a long way in
        Layout L(long_entries());
        modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, inside);
        const std::string err = round_trip(L, MODGPU_DIGEST_INPUT, (L.total() + inside - 1) / inside);
        report("cut inside long entries", err.empty(), err);
    }
    modgpu_debug_set_host_tunable(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, 0);
    run_case("one launch again with the limit back", with_empties());
}
} // namespace

int main()
{
    {
        Layout L(phases_and_sizes());
        auto t = L.table(true);
        modgpu_host_trace(1);
        const int rc = modgpu_cycle_host_to_device_list_digest(t.data(), t.size(), MODGPU_DIGEST_OUTPUT, L.recs(), 0);
        modgpu_host_trace(0);
        std::vector<modgpu_host_trace_event_t> ev(4096);
        const int n = std::min<int>(modgpu_host_trace_read(ev.data(), (int)ev.size()), (int)ev.size());
        for (int i = 0; i < n; ++i)
            if (ev[i].kind == MODGPU_TRACE_SLOTS) g_chunk = ev[i].bytes;
        report("the chunk size from the host trace", rc == MODGPU_OK && g_chunk >= PIECE && g_chunk % PIECE == 0, "chunk=" + std::to_string(g_chunk));
        if (!g_chunk) g_chunk = 4 * PIECE;
    }
    run_case("phases and sizes", phases_and_sizes());
    run_case("boundaries", boundaries(g_chunk));
    run_case("every source byte 0xFF", all_ones());
    run_case("the position wraps twice", wraps_twice());
    run_case("ten thousand tiny entries", tiny_entries());
    run_case("empty entries", with_empties());
    run_case("entries longer than 8 MiB", long_entries());
    run_case("no entries", {});
    only_empty_entries();
    refusals();
    twice_on_the_same_records();
    injected_failure_in_the_middle();
    cut_into_windows();
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
