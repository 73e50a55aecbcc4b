// host_calls_main.cpp -- the single host-buffer calls (modgpu_cycle_host, modgpu_cycle_auto_host, modgpu_cycle_file*) and the single
// transfers (modgpu_cycle_host_to_device & co.) on the CPU stand-in of the HIP runtime, as a program of its own (built by
// `make host-calls-main` from the library's host sources, once with ASan + UBSan and once with TSan, runtimes linked statically; run
// directly by tests/test_host_calls_cpu.py).  Every shape of call and every route of modulate_amd/csrc/host_stream.cpp at the smallest
// size that still takes it, injected failures at every stage, the staging set of another NUMA node, and one list call and one list
// digest call cut into two windows.  Every byte of the destination and of the guard bytes around it is compared with a model computed
// here from lcg.h, byte by byte.  Each line also prints what the call's plan led to: return code and error text, what the call added
// to modgpu_path_stats, the calling thread's last launch, the host trace's events per kind, the slots event's pipelines and chunk, the
// chunks filled / marked ready / launched / drained, and the calls that took another node's staging set.  Nothing that depends on the
// run is printed -- no thread ids, times or addresses, no order of events between pipelines; where pipelines race for what a line
// would say (a failure among several of them) the line says less -- so one commit's output can be compared with another's byte for byte.
// Exit status 0 = all of it held.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "lcg.h"
#include "modgpu.h"
#include "modgpu_testing.h"

extern "C" { // the stand-in's own: "device" memory the transfer calls accept, and a launch the "runtime" refuses
void *modgpu_shim_xfer_alloc(unsigned long long n, int device);
void modgpu_shim_xfer_free(void *p);
void modgpu_shim_fail_next_feed_launch(int on);
void modgpu_shim_fail_next_xfer_launch(int on);
}

namespace {
constexpr int32_t PS3 = (int32_t)0xC64EED30, PS4 = (int32_t)0x90CFC0AB, IDENTITY = 0x7FFFFFFF;
constexpr uint64_t PERIOD = 0x7FFFFFFEull;
constexpr uint64_t PIECE = 32768, GUARD = 64;
constexpr uint64_t ZEROCOPY = 4096;        // the one-slot limit the cases run with (below a piece)
constexpr uint64_t MIB = 1ull << 20;
constexpr uint8_t HOST_FILL = 0x3C, DEV_FILL = 0xD5;

int g_failed = 0, g_cases = 0;
uint64_t g_pipes = 0, g_many = 0; // MODGPU_HOST_PIPES as latched; 2 x pipes x chunk + 17 at the feed chunk of one piece
std::string g_dir;                // the temporary directory of the file cases

void report(const std::string &what, bool ok, const std::string &detail = "")
{
    ++g_cases;
    if (!ok) ++g_failed;
    std::printf("%s %s%s%s\n", ok ? "ok  " : "FAIL", what.c_str(), detail.empty() ? "" : " | ", detail.c_str());
    std::fflush(stdout);
}
uint64_t splitmix(uint64_t &x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
std::vector<uint8_t> plaintext(uint64_t n, uint64_t seed)
{
    std::vector<uint8_t> v(n);
    for (auto &b : v) b = (uint8_t)splitmix(seed);
    return v;
}
// the model: out[j] = in[j] ^ ks(key)[off + j], the position taken in the integers and reduced mod the period
std::vector<uint8_t> model(const std::vector<uint8_t> &in, int32_t key, uint64_t off)
{
    std::vector<uint8_t> out(in);
    const uint32_t r = lcg::key_residue(key);
    if (!r) return out;
    uint32_t s = lcg::state_residue(r, off % PERIOD);
    for (auto &b : out) b ^= (uint8_t)~s, s = lcg::mulmod(s, lcg::A);
    return out;
}

// n bytes between two guards: pageable, page-locked (modgpu_host_alloc) or the stand-in's device memory
enum Kind { PAGEABLE, LOCKED, DEVICE };
struct Buf {
    Kind kind;
    uint64_t n, phase;
    uint8_t *base = nullptr, fill;
    Buf(Kind k, uint64_t n_, uint64_t phase_ = 0) : kind(k), n(n_), phase(phase_), fill(k == DEVICE ? DEV_FILL : HOST_FILL)
    {
        const uint64_t all = n + phase + 2 * GUARD;
        if (kind == PAGEABLE) base = static_cast<uint8_t *>(std::malloc(all));
        else if (kind == DEVICE) base = static_cast<uint8_t *>(modgpu_shim_xfer_alloc(all, 0));
        else if (modgpu_host_alloc(reinterpret_cast<void **>(&base), all) != MODGPU_OK) base = nullptr;
        if (!base) std::abort();
        std::memset(base, fill, all);
    }
    Buf(const Buf &) = delete;
    ~Buf()
    {
        if (kind == PAGEABLE) std::free(base);
        else if (kind == DEVICE) modgpu_shim_xfer_free(base);
        else (void)modgpu_host_free(base);
    }
    uint8_t *p() const { return base + GUARD + phase; }
    void set(const std::vector<uint8_t> &v) { if (n) std::memcpy(p(), v.data(), n); }
    bool is(const std::vector<uint8_t> &v) const { return v.size() == n && (n == 0 || std::memcmp(p(), v.data(), n) == 0); }
    bool untouched() const { return is(std::vector<uint8_t>(n, fill)); }
    bool guards() const
    {
        for (uint64_t i = 0; i < GUARD + phase; ++i)
            if (base[i] != fill) return false;
        for (uint64_t i = 0; i < GUARD; ++i)
            if (p()[n + i] != fill) return false;
        return true;
    }
};

std::string path_of(const char *name) { return g_dir + "/" + name; }
bool write_file(const std::string &path, const std::vector<uint8_t> &head, const std::vector<uint8_t> &body)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = (head.empty() || std::fwrite(head.data(), 1, head.size(), f) == head.size()) && (body.empty() || std::fwrite(body.data(), 1, body.size(), f) == body.size());
    return std::fclose(f) == 0 && ok;
}
std::vector<uint8_t> read_file(const std::string &path)
{
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    uint8_t buf[65536];
    for (size_t r; (r = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + r);
    std::fclose(f);
    return v;
}

// ---- what a call did, as the library itself reports it -------------------------------------------------------------------------------
const char *const KINDS[15] = {"begin", "slots", "posted", "pipe_start", "fill_begin", "fill_end", "launched", "sync_begin", "sync_end", "drain_end",
                               "pipe_end", "end", "failed", "rescued", "ready"};
// (chunk, bytes) pairs, sorted, runs of consecutive chunks of one size as first-last:bytes
std::string runs_of(std::vector<std::pair<uint64_t, uint64_t>> v)
{
    std::sort(v.begin(), v.end());
    std::string s;
    for (size_t i = 0; i < v.size();) {
        size_t j = i + 1;
        while (j < v.size() && v[j].second == v[i].second && v[j].first == v[j - 1].first + 1) ++j;
        s += (s.empty() ? "" : ",") + std::to_string(v[i].first) + (j - i > 1 ? "-" + std::to_string(v[j - 1].first) : "") + ":" + std::to_string(v[i].second);
        i = j;
    }
    return s.empty() ? "-" : s;
}
struct Watch { // from its construction to text(): one case's calls
    modgpu_path_stats_t st0;
    uint64_t pool0[6];
    uint64_t node_sets = 0, pipes = 0, chunk = 0; // (after text(): the calls that took another node's set; the last slots event)
    Watch()
    {
        modgpu_path_stats(&st0, 0);
        modgpu_host_pool_stats(pool0);
        modgpu_host_trace(1);
    }
    // `racing`: several pipelines met a failure -- how far each got before it saw the others stop is the run's business; the line keeps
    // to what the call decided before they started and how it ended
    std::string text(int rc, bool racing = false)
    {
        modgpu_host_trace(0);
        std::vector<modgpu_host_trace_event_t> ev((size_t)std::max(modgpu_host_trace_read(nullptr, 0), 1));
        const int n_ev = std::min<int>(modgpu_host_trace_read(ev.data(), (int)ev.size()), (int)ev.size());
        modgpu_path_stats_t st;
        uint64_t pool[6];
        modgpu_path_stats(&st, 0);
        modgpu_host_pool_stats(pool);
        node_sets = pool[5] - pool0[5];
        uint64_t count[15] = {};
        std::vector<std::pair<uint64_t, uint64_t>> fill, ready, launched, drain;
        std::string slots;
        bool launch_of_the_call = false;
        for (int i = 0; i < n_ev; ++i) {
            const modgpu_host_trace_event_t &e = ev[(size_t)i];
            if (e.kind < 0 || e.kind >= 15) continue;
            ++count[e.kind];
            if (e.kind == MODGPU_TRACE_SLOTS) {
                pipes = e.chunk, chunk = e.bytes;
                slots += (slots.empty() ? "" : ",") + std::to_string(e.chunk) + "x" + std::to_string(e.bytes);
            }
            if (e.kind == MODGPU_TRACE_FILL_END) fill.push_back({e.chunk, e.bytes});
            if (e.kind == MODGPU_TRACE_READY) ready.push_back({e.chunk, e.bytes});
            if (e.kind == MODGPU_TRACE_LAUNCHED) launched.push_back({e.chunk, e.bytes}), launch_of_the_call = launch_of_the_call || e.pipe < 0;
            if (e.kind == MODGPU_TRACE_DRAIN_END) drain.push_back({e.chunk, e.bytes});
        }
        char buf[1024];
        std::snprintf(buf, sizeof buf, "rc=%d err=\"%s\"", rc, rc != MODGPU_OK || std::strncmp(modgpu_last_error(), "finished on the host", 20) == 0 ? modgpu_last_error() : "");
        std::string s = buf;
        s += " slots=" + (slots.empty() ? std::string("-") : slots);
        if (racing) {
            std::snprintf(buf, sizeof buf, " begin=%llu end=%llu posted=%llu", (unsigned long long)count[0], (unsigned long long)count[11], (unsigned long long)count[2]);
            return s + buf;
        }
        std::snprintf(buf, sizeof buf, " calls=%llu bytes=%llu direct=%llu staged=%llu scalar=%llu rescues=%llu rescued=%llu launches=%llu",
                      (unsigned long long)(st.gpu_calls - st0.gpu_calls), (unsigned long long)(st.gpu_bytes - st0.gpu_bytes),
                      (unsigned long long)(st.direct_bytes - st0.direct_bytes), (unsigned long long)(st.staged_bytes - st0.staged_bytes),
                      (unsigned long long)(st.scalar_bytes - st0.scalar_bytes), (unsigned long long)(st.midcall_rescues - st0.midcall_rescues),
                      (unsigned long long)(st.midcall_rescued_bytes - st0.midcall_rescued_bytes), (unsigned long long)(st.gpu_launches - st0.gpu_launches));
        s += buf;
        // the calling thread's last launch: the call's own where it has one launch, or one pipeline (which this thread then ran itself)
        modgpu_launch_info_t li{};
        if ((launch_of_the_call || pipes <= 1) && st.gpu_launches != st0.gpu_launches && modgpu_last_launch(&li) == MODGPU_OK && li.kernel) {
            // (the grid of the host-fed and transfer kernels follows from the size alone; an in-place launch's also from where the
            //  allocator put the buffer it works on, which is the run's business)
            std::snprintf(buf, sizeof buf, " last=[%s v=%d bytes=%llu", li.kernel, li.variant, (unsigned long long)li.bytes);
            s += buf + (li.variant >= 4 ? " grid=" + std::to_string(li.grid) : std::string()) + "]";
        }
        s += " ev=" + std::string(n_ev ? "" : "-");
        for (int k = 0; k < 15; ++k)
            if (count[k]) s += (s.back() == '=' ? "" : ",") + std::string(KINDS[k]) + ":" + std::to_string(count[k]);
        s += " fill=" + runs_of(fill) + " ready=" + runs_of(ready) + " launched=" + runs_of(launched) + " drain=" + runs_of(drain);
        s += " node_sets=" + std::to_string(node_sets);
        return s;
    }
};

void set(int which, uint64_t value) { modgpu_debug_set_host_tunable(which, value); }

// ---- stream_impl: memory in place -------------------------------------------------------------------------------------------------
// modgpu_cycle_host (or _auto_host) on n bytes of `kind` memory: every byte and the guards against the model
enum Api { CYCLE, AUTO };
void in_place(const std::string &what, Kind kind, uint64_t n, int32_t key = PS4, uint64_t off = 5, Api api = CYCLE, int want_rc = MODGPU_OK, bool racing = false)
{
    const std::vector<uint8_t> pt = plaintext(n, n + 1);
    Buf b(kind, n);
    b.set(pt);
    Watch w;
    const int rc = api == AUTO ? modgpu_cycle_auto_host(b.p(), n, key, off, 0) : modgpu_cycle_host(b.p(), n, key, off, 0);
    const std::string t = w.text(rc, racing);
    // (a call that failed with nobody to finish it leaves the pieces that had arrived cycled and the others as they were: only the guards)
    const bool ok = rc == want_rc && b.guards() && (rc != MODGPU_OK || b.is(model(pt, key, off)));
    report(what, ok, t);
}

// ---- stream_impl: the file shapes -------------------------------------------------------------------------------------------------
enum Shape { FILE_TO_MEM, MEM_TO_FILE, FILE_TO_FILE };
void file_call(const std::string &what, Shape shape, Kind kind, uint64_t n, int32_t key = PS3, uint64_t off = (1ull << 32) + 5)
{
    const std::vector<uint8_t> pt = plaintext(n, n + 2), head(7, 0xEE);
    const std::string in = path_of("in.bin"), out = path_of("out.bin");
    bool ok = true;
    std::string t;
    if (shape == FILE_TO_MEM) { // the bytes behind a 7-byte head of the file
        ok = write_file(in, head, pt);
        Buf b(kind, n);
        Watch w;
        const int rc = modgpu_cycle_file_to_host(in.c_str(), head.size(), b.p(), n, key, off, 0);
        t = w.text(rc);
        ok = ok && rc == MODGPU_OK && b.guards() && b.is(model(pt, key, off));
    } else if (shape == MEM_TO_FILE) {
        Buf b(kind, n);
        b.set(pt);
        Watch w;
        const int rc = modgpu_cycle_host_to_file(b.p(), n, out.c_str(), key, off, 0);
        t = w.text(rc);
        ok = rc == MODGPU_OK && b.guards() && b.is(pt) && read_file(out) == model(pt, key, off);
    } else {
        ok = write_file(in, {}, pt);
        Watch w;
        const int rc = modgpu_cycle_file(in.c_str(), out.c_str(), key, off, 0);
        t = w.text(rc);
        ok = ok && rc == MODGPU_OK && read_file(in) == pt && read_file(out) == model(pt, key, off);
    }
    report(what, ok, t);
}

// ---- xfer_impl ------------------------------------------------------------------------------------------------------------------------
// one transfer, `host` memory (or, host == DEVICE: a file) on the host side, the device buffer at `phase` mod 16.  A call that fails
// leaves its source intact.
void transfer(const std::string &what, bool up, Kind host, uint64_t n, uint64_t phase = 3, int32_t key = PS4, uint64_t off = PERIOD - 100, int want_rc = MODGPU_OK,
              bool racing = false)
{
    const std::vector<uint8_t> pt = plaintext(n, n + 3), want = model(pt, key, off);
    const bool file = host == DEVICE;
    Buf d(DEVICE, n, phase), h(file ? PAGEABLE : host, file ? 0 : n, file ? 0 : 5);
    const std::string path = path_of(up ? "up.bin" : "down.bin");
    bool ok = true;
    if (up && file) ok = write_file(path, std::vector<uint8_t>(7, 0xEE), pt);
    else if (up) h.set(pt);
    else d.set(pt);
    Watch w;
    const int rc = up ? (file ? modgpu_cycle_file_to_device(path.c_str(), 7, d.p(), n, key, off, 0) : modgpu_cycle_host_to_device(d.p(), h.p(), n, key, off, 0))
                      : (file ? modgpu_cycle_device_to_file(d.p(), n, path.c_str(), key, off, 0) : modgpu_cycle_device_to_host(h.p(), d.p(), n, key, off, 0));
    const std::string t = w.text(rc, racing);
    ok = ok && rc == want_rc && d.guards() && h.guards();
    if (up) ok = ok && (file || h.is(pt)) && (rc != MODGPU_OK || d.is(want));
    else ok = ok && d.is(pt) && (rc != MODGPU_OK || (file ? read_file(path) == want : h.is(want)));
    report(what, ok, t);
}

// ---- failures -------------------------------------------------------------------------------------------------------------------------
const char *const STAGES[5] = {"fill", "launch", "sync", "drain", "after-drain"};
std::string piece_name(int64_t p) { return p == MODGPU_INJECT_PIECE_MIDDLE ? "middle" : p == MODGPU_INJECT_PIECE_LAST ? "last" : std::to_string(p); }
// One pipeline (all other pipeline slots of the set are held), seven pieces: which pieces had arrived when the failure came, and so
// what the host loop is left with, is the same in every run.
void failures_at_every_stage()
{
    const uint64_t n = 6 * PIECE + 17;
    const int held = modgpu_debug_hold_slots(0, 30);
    report("all pipeline slots but two held", held == 30, "held=" + std::to_string(held));
    for (int64_t piece : {(int64_t)0, (int64_t)MODGPU_INJECT_PIECE_MIDDLE, (int64_t)MODGPU_INJECT_PIECE_LAST})
        for (int stage = MODGPU_STAGE_FILL; stage <= MODGPU_STAGE_AFTER_DRAIN; ++stage) {
            const std::string at = std::string(" piece ") + piece_name(piece) + " stage " + STAGES[stage];
            { // feed, with the host loop behind it: rescued, the bytes right
                const std::vector<uint8_t> pt = plaintext(n, 40 + (uint64_t)stage);
                Buf b(PAGEABLE, n);
                b.set(pt);
                Watch w;
                modgpu_debug_inject_failure_at(piece, stage);
                const int rc = modgpu_cycle_auto_host(b.p(), n, PS4, 9, 0);
                const bool fired = modgpu_debug_injection_armed() == 0;
                modgpu_debug_inject_failure_at(0, -1);
                const std::string t = w.text(rc);
                report("injected failure on feed," + at, rc == MODGPU_OK && fired && b.guards() && b.is(model(pt, PS4, 9)) &&
                                                            std::strncmp(modgpu_last_error(), "finished on the host loop after:", 32) == 0, t);
            }
            for (int up = 1; up >= 0; --up) { // xfer: the error stands, the source is intact (an upload has nothing to drain: those stages do not fire)
                if (up && (stage == MODGPU_STAGE_DRAIN)) continue;
                modgpu_debug_inject_failure_at(piece, stage);
                transfer(std::string("injected failure on xfer ") + (up ? "up," : "down,") + at, up != 0, PAGEABLE, n, 1, PS3, 77, MODGPU_ERR_HIP);
                const bool fired = modgpu_debug_injection_armed() == 0;
                modgpu_debug_inject_failure_at(0, -1);
                if (!fired) report(std::string("injected failure on xfer ") + (up ? "up," : "down,") + at + ": fired", false);
            }
        }
    report("the held slots given back", modgpu_debug_hold_slots(0, 0) == 0);
}

void launch_errors()
{
    // one pipeline: nothing has begun when the launch is refused -- the error is the call's, and _auto_ does the whole buffer on the host
    modgpu_shim_fail_next_feed_launch(1);
    in_place("a refused launch, one pipeline: the error stands", PAGEABLE, PIECE, PS4, 5, CYCLE, MODGPU_ERR_HIP);
    modgpu_shim_fail_next_feed_launch(1);
    in_place("a refused launch, one pipeline, the host loop behind it", PAGEABLE, PIECE, PS4, 5, AUTO);
    // several pipelines, one of which fails by itself as well: the launch's text wins over the pipeline's
    modgpu_shim_fail_next_feed_launch(1);
    modgpu_debug_inject_failure_at(1, MODGPU_STAGE_FILL);
    in_place("a refused launch with several pipelines: the launch's text wins over a pipeline's", PAGEABLE, g_many, PS4, 5, CYCLE, MODGPU_ERR_HIP, true);
    modgpu_debug_inject_failure_at(0, -1);
    report("... and its text", std::strstr(modgpu_last_error(), "cycle kernel launch (host-fed)") != nullptr);
    modgpu_shim_fail_next_feed_launch(1);
    in_place("a refused launch with several pipelines, the host loop behind it", PAGEABLE, g_many, PS4, 5, AUTO, MODGPU_OK, true);
    for (int up = 1; up >= 0; --up) {
        modgpu_shim_fail_next_xfer_launch(1);
        transfer(std::string("a refused transfer launch, one pipeline, ") + (up ? "up" : "down"), up != 0, PAGEABLE, PIECE, 3, PS4, 5, MODGPU_ERR_HIP);
        modgpu_shim_fail_next_xfer_launch(1);
        modgpu_debug_inject_failure_at(1, MODGPU_STAGE_FILL);
        transfer(std::string("a refused transfer launch with several pipelines, ") + (up ? "up" : "down"), up != 0, PAGEABLE, g_many, 3, PS4, 5, MODGPU_ERR_HIP, true);
        modgpu_debug_inject_failure_at(0, -1);
        report("... and its text", std::strstr(modgpu_last_error(), "cycle kernel launch (transfer)") != nullptr);
        modgpu_shim_fail_next_xfer_launch(1);
        transfer(std::string("a refused transfer launch on page-locked memory, ") + (up ? "up" : "down"), up != 0, LOCKED, PIECE, 3, PS4, 5, MODGPU_ERR_HIP);
    }
}

// ---- the list transfers: three entries in two windows, the second entry clipped ----------------------------------------------------------
void list_calls(const std::string &what, bool digest, uint64_t most, bool other_node = false)
{
    const uint64_t sizes[3] = {40000, 70000, 30000}, offs[3] = {0, (1ull << 40) + 3, PERIOD - 7};
    const int32_t keys[3] = {PS4, PS3, IDENTITY};
    std::vector<std::vector<uint8_t>> pt;
    std::vector<Buf *> dev, src, back;
    for (int e = 0; e < 3; ++e) {
        pt.push_back(plaintext(sizes[e], 90 + (uint64_t)e));
        dev.push_back(new Buf(DEVICE, sizes[e], (uint64_t)(e * 5 + 1)));
        src.push_back(new Buf(PAGEABLE, sizes[e], (uint64_t)(e * 3)));
        back.push_back(new Buf(PAGEABLE, sizes[e], (uint64_t)(e * 7 + 2)));
        src.back()->set(pt.back());
    }
    Buf records(DEVICE, 3 * sizeof(modgpu_digest_result_t));
    modgpu_digest_result_t *const rec = reinterpret_cast<modgpu_digest_result_t *>(records.p());
    std::vector<modgpu_table_entry_t> up, down;
    for (int e = 0; e < 3; ++e) {
        up.push_back({dev[(size_t)e]->p(), src[(size_t)e]->p(), sizes[e], offs[e], keys[e], 0});
        down.push_back({back[(size_t)e]->p(), dev[(size_t)e]->p(), sizes[e], offs[e], keys[e], 0});
    }
    set(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, most);
    auto sums = [&] {
        std::string s;
        for (int e = 0; e < 3; ++e) s += " rec" + std::to_string(e) + "=" + std::to_string(rec[e].s1 % 65521) + "/" + std::to_string(rec[e].s2 % 65521) + "/" + std::to_string(rec[e].n);
        return s;
    };
    for (int dir = 1; dir >= 0; --dir) {
        Watch w;
        const int rc = digest ? (dir ? modgpu_cycle_host_to_device_list_digest(up.data(), 3, MODGPU_DIGEST_INPUT, rec, 0)
                                     : modgpu_cycle_device_to_host_list_digest(down.data(), 3, MODGPU_DIGEST_OUTPUT, rec, 0))
                              : (dir ? modgpu_cycle_host_to_device_list(up.data(), 3, 0) : modgpu_cycle_device_to_host_list(down.data(), 3, 0));
        std::string t = w.text(rc);
        bool ok = rc == MODGPU_OK && records.guards();
        for (size_t e = 0; e < 3; ++e) {
            ok = ok && dev[e]->guards() && src[e]->guards() && back[e]->guards() && src[e]->is(pt[e]) && dev[e]->is(model(pt[e], keys[e], offs[e]));
            if (!dir) ok = ok && back[e]->is(pt[e]);
            if (digest) ok = ok && rec[e].n == sizes[e] && rec[e].reserved == 0;
        }
        if (digest) t += sums();
        if (other_node && w.node_sets != 1) t = "skipped: one node";
        report(what + (dir ? ", up" : ", down"), ok, t);
        if (other_node) break;
    }
    set(MODGPU_TUNABLE_XFER_LIST_MOST_BYTES, 0);
    for (auto *v : {&dev, &src, &back})
        for (Buf *b : *v) delete b;
}

// ---- the staging set of another node: the library is told its GPU hangs off node 1, so that node 0's pages are "elsewhere" -----------------
void another_nodes_set()
{
    modgpu_debug_set_gpu_node(1);
    { // (a machine whose kernel does not say which node a page is on places nothing: all three lines then say so, on every commit alike)
        const std::vector<uint8_t> pt = plaintext(g_many, 7);
        Buf b(PAGEABLE, g_many);
        b.set(pt);
        Watch w;
        const int rc = modgpu_cycle_host(b.p(), g_many, PS4, 5, 0);
        const std::string t = w.text(rc);
        report("the staging set of another node, host buffer", rc == MODGPU_OK && b.guards() && b.is(model(pt, PS4, 5)), w.node_sets == 1 ? t : "skipped: one node");
    }
    {
        const std::vector<uint8_t> pt = plaintext(g_many, 8);
        Buf h(PAGEABLE, g_many), d(DEVICE, g_many, 1);
        h.set(pt);
        Watch w;
        const int rc = modgpu_cycle_host_to_device(d.p(), h.p(), g_many, PS4, 5, 0);
        const std::string t = w.text(rc);
        report("the staging set of another node, transfer", rc == MODGPU_OK && d.guards() && d.is(model(pt, PS4, 5)), w.node_sets == 1 ? t : "skipped: one node");
    }
    list_calls("the staging set of another node, list of two windows", false, 3 * PIECE, true);
    modgpu_debug_set_gpu_node(-2);
    in_place("the GPU's own set again", PAGEABLE, g_many);
}
} // namespace

int main()
{
    ::setenv("MODGPU_MIN_GPU_BYTES", "0", 1); // modgpu_cycle_auto_host: every size of these cases goes to the kernel (read at its first call)
    const char *tmp = std::getenv("TMPDIR");
    std::string dir = std::string(tmp && *tmp ? tmp : "/tmp") + "/host_calls_XXXXXX";
    if (!::mkdtemp(dir.data())) {
        std::perror("mkdtemp");
        return 2;
    }
    g_dir = dir;
    uint64_t tun[4];
    modgpu_host_tunables(tun);
    g_pipes = tun[0];
    set(MODGPU_TUNABLE_ZEROCOPY_BYTES, ZEROCOPY);
    set(MODGPU_TUNABLE_FEED_CHUNK_BYTES, PIECE);
    g_many = 2 * g_pipes * PIECE + 17;
    { // the feed chunk of the cases, as the library's host trace reports it
        const std::vector<uint8_t> pt = plaintext(g_many, 1);
        Buf b(PAGEABLE, g_many);
        b.set(pt);
        Watch w;
        const int rc = modgpu_cycle_host(b.p(), g_many, PS4, 0, 0);
        const std::string t = w.text(rc);
        report("the chunk size from the host trace", rc == MODGPU_OK && w.chunk == PIECE && w.pipes == g_pipes && b.is(model(pt, PS4, 0)), t);
    }
    // -- stream_impl, each shape of call
    in_place("page-locked in place", LOCKED, 64 * 1024 + 5);
    in_place("one slot, at the limit", PAGEABLE, ZEROCOPY);
    in_place("one slot, one below the limit", PAGEABLE, ZEROCOPY - 1);
    in_place("one slot, page-locked source is cycled in place all the same", LOCKED, ZEROCOPY);
    in_place("feed, one piece", PAGEABLE, PIECE);
    in_place("feed, 2 x pipes x chunk + 17", PAGEABLE, g_many);
    set(MODGPU_TUNABLE_FEED, 0);
    set(MODGPU_TUNABLE_RAMP_BYTES, 64 * 1024);
    in_place("slot_kernel, one piece", PAGEABLE, PIECE);
    in_place("slot_kernel, five chunks behind a ramp", PAGEABLE, 4 * MIB + 17);
    set(MODGPU_TUNABLE_RAMP_BYTES, 512 * 1024);
    set(MODGPU_TUNABLE_FEED, 1);
    modgpu_debug_set_staged_mode(1);
    in_place("dma, pageable on both sides", PAGEABLE, 2 * MIB + 5);
    file_call("dma, page-locked source to a file", MEM_TO_FILE, LOCKED, 2 * MIB + 5);
    file_call("dma, a file to a page-locked destination", FILE_TO_MEM, LOCKED, 2 * MIB + 5);
    modgpu_debug_set_staged_mode(0);
    modgpu_debug_set_pinned_mode(1);
    in_place("dma, page-locked in place on the ring", LOCKED, 3 * MIB + 5);
    modgpu_debug_set_pinned_mode(0);
    file_call("file to pageable", FILE_TO_MEM, PAGEABLE, g_many);
    file_call("file to page-locked, through the slots", FILE_TO_MEM, LOCKED, g_many);
    set(MODGPU_TUNABLE_FILE_FEED, 0);
    file_call("file to page-locked, in_dst", FILE_TO_MEM, LOCKED, g_many);
    file_call("file to pageable, a launch per chunk", FILE_TO_MEM, PAGEABLE, g_many);
    set(MODGPU_TUNABLE_FILE_FEED, 1);
    file_call("pageable to file", MEM_TO_FILE, PAGEABLE, g_many);
    file_call("file to file", FILE_TO_FILE, PAGEABLE, g_many);
    in_place("identity key in place: nothing to do", PAGEABLE, g_many, IDENTITY);
    file_call("identity key out of place, file to pageable", FILE_TO_MEM, PAGEABLE, g_many, 0);
    file_call("identity key out of place, page-locked to file", MEM_TO_FILE, LOCKED, g_many, IDENTITY);
    in_place("stream_off at 2^64 - 3", PAGEABLE, g_many, PS3, ~0ull - 2);
    in_place("stream_off at 2^64 - 3, page-locked", LOCKED, 64 * 1024 + 5, PS3, ~0ull - 2);
    in_place("n = 0", PAGEABLE, 0);
    // -- xfer_impl
    for (int up = 1; up >= 0; --up) {
        const std::string d = up ? "up" : "down";
        transfer("transfer " + d + ", pageable, one piece", up != 0, PAGEABLE, PIECE);
        for (uint64_t phase : {0, 1, 15}) transfer("transfer " + d + ", pageable, 2 x pipes x chunk + 17, device phase " + std::to_string(phase), up != 0, PAGEABLE, g_many, phase);
        transfer("transfer " + d + ", page-locked, one piece", up != 0, LOCKED, PIECE);
        transfer("transfer " + d + ", page-locked, 2 x pipes x chunk + 17", up != 0, LOCKED, g_many, 4);
        transfer("transfer " + d + ", a file on the host side", up != 0, DEVICE, g_many, 15);
        transfer("transfer " + d + ", identity key", up != 0, PAGEABLE, g_many, 1, IDENTITY);
        transfer("transfer " + d + ", identity key, page-locked", up != 0, LOCKED, g_many, 1, 0);
        modgpu_debug_set_xfer_form(1);
        transfer("transfer " + d + ", DMA form, pageable", up != 0, PAGEABLE, 2 * MIB + 5);
        transfer("transfer " + d + ", DMA form, page-locked", up != 0, LOCKED, 2 * MIB + 5);
        modgpu_debug_set_xfer_form(0);
    }
    { // a device pointer that is host memory: refused, nothing queued, nothing written
        const std::vector<uint8_t> pt = plaintext(g_many, 5);
        Buf h(PAGEABLE, g_many), not_dev(PAGEABLE, g_many);
        h.set(pt);
        Watch w;
        const int rc = modgpu_cycle_host_to_device(not_dev.p(), h.p(), g_many, PS4, 0, 0);
        const std::string t = w.text(rc);
        Watch w2;
        const int rc2 = modgpu_cycle_device_to_host(h.p(), not_dev.p(), g_many, PS4, 0, 0);
        report("a device pointer that is host memory, up", rc == MODGPU_ERR_INVALID && not_dev.untouched() && not_dev.guards() && h.is(pt), t);
        report("a device pointer that is host memory, down", rc2 == MODGPU_ERR_INVALID && not_dev.untouched() && h.is(pt) && h.guards(), w2.text(rc2));
    }
    // -- failures
    failures_at_every_stage();
    launch_errors();
    modgpu_debug_forbid_worker_threads(1);
    in_place("no worker threads to be had: not the feed route", PAGEABLE, g_many);
    transfer("no worker threads to be had: a transfer of one pipeline", true, PAGEABLE, g_many);
    modgpu_debug_forbid_worker_threads(0);
    modgpu_debug_inject_failures(3);
    in_place("injected failure before anything is touched, host buffer", PAGEABLE, g_many, PS4, 5, CYCLE, MODGPU_ERR_HIP);
    transfer("injected failure before anything is touched, transfer", true, PAGEABLE, g_many, 3, PS4, 5, MODGPU_ERR_HIP);
    {
        Buf d(DEVICE, 100), h(PAGEABLE, 100);
        const modgpu_table_entry_t e{d.p(), h.p(), 100, 0, PS4, 0};
        Watch w;
        const int rc = modgpu_cycle_host_to_device_list(&e, 1, 0);
        report("injected failure before anything is touched, list", rc == MODGPU_ERR_HIP && d.untouched(), w.text(rc));
    }
    modgpu_debug_inject_failures(0);
    in_place("a good call after the failures", PAGEABLE, g_many);
    // -- the three users of the staging-set choice
    another_nodes_set();
    // -- send_window
    list_calls("list of three entries in two windows, the second clipped", false, 3 * PIECE);
    list_calls("list digest of three entries in two windows, the second clipped", true, 3 * PIECE);
    ::unlink(path_of("in.bin").c_str()), ::unlink(path_of("out.bin").c_str()), ::unlink(path_of("up.bin").c_str()), ::unlink(path_of("down.bin").c_str());
    ::rmdir(g_dir.c_str());
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
