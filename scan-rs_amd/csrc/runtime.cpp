// The process runtime: the calling thread's error text, SCANRS_TRACE and the stage ring, the landing places of device-to-host
// copies, the bounded waits and their timeout report, the device-lost state, and the registry of live handles.
#include <algorithm>
#include <cstdlib>

#include "common.hpp"

namespace scanrs {

// ---- errors ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
void fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    throw Failure{code};
}

uint32_t next_map_op_id() {
    static std::atomic<uint32_t> next{1};
    return next.fetch_add(1, std::memory_order_relaxed);
}

// SCANRS_TRACE=1: phase timings (with the synchronisations they need); SCANRS_TRACE=2: stage markers only — one line per host
// step of the solvers, nothing synchronised: where a call that does not return is standing.
static int trace_level() {
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("SCANRS_TRACE");
        v = !e ? 0 : (e[0] == '2' ? 2 : 1);
    }
    return v;
}
bool trace_on() { return trace_level() == 1; }

// the calling thread's last stage marks (what a timed-out wait reports)
namespace {
struct StageRing {
    static constexpr int N = 16;
    struct Rec {
        char what[40];
        long a, b;
        std::chrono::steady_clock::time_point t;
    } rec[N];
    unsigned n = 0;
};
thread_local StageRing tl_stages;
thread_local const Storage *tl_handle = nullptr;
thread_local const Storage *tl_dying = nullptr; // scanrs_mat_free: the storage whose members are being destroyed on this thread (its streams are drained)

std::atomic<double> g_sync_timeout_s{120.0};
} // namespace
// set by a bounded wait that gave up (timeout_report); cleared only when the whole device has been seen idle again (device_recovered)
std::atomic<bool> g_device_lost{false};
bool device_lost() { return g_device_lost.load(std::memory_order_acquire); }
// the handles of this process (registry_add, where a handle is created): "is every stream the library owns idle?" walks them
static std::mutex g_storages_mu;
static std::set<const Storage *> g_storages;
static std::atomic<int> g_storages_dying{0}; // handles inside their destructor: out of the set (nobody may walk their members), their streams possibly still draining
// every stream every handle queues work on (main, the two auxiliary ones, the overflow gather's, the helper thread's) has run dry
bool all_library_streams_idle() {
    std::lock_guard<std::mutex> lk(g_storages_mu);
    bool idle = g_storages_dying.load(std::memory_order_acquire) == 0;
    for (const Storage *st : g_storages)
        for_each_stream(*st, [&](const char *, hipStream_t q) {
            if (idle && hipStreamQuery(q) != hipSuccess) {
                (void)hipGetLastError();
                idle = false;
            }
        });
    return idle;
}
void registry_add(const Storage *st) {
    std::lock_guard<std::mutex> lk(g_storages_mu);
    g_storages.insert(st);
}
// Out of the set of handles FIRST (another thread's all_library_streams_idle walked a storage whose streams were
// already destroyed); while the destructor drains the streams the process counts as busy.
RegistryLeave::RegistryLeave(const Storage *st) {
    std::lock_guard<std::mutex> lk(g_storages_mu);
    g_storages.erase(st);
    g_storages_dying.fetch_add(1, std::memory_order_acq_rel);
}
RegistryLeave::~RegistryLeave() { g_storages_dying.fetch_sub(1, std::memory_order_acq_rel); }
void registry_set_side(Storage &st, Storage::SideBuild *sb) {
    std::lock_guard<std::mutex> lk(g_storages_mu);
    st.side = sb;
}

void stage_mark(const char *what, long a, long b) {
    StageRing::Rec &r = tl_stages.rec[tl_stages.n++ % StageRing::N];
    strncpy(r.what, what, sizeof(r.what) - 1);
    r.what[sizeof(r.what) - 1] = 0;
    r.a = a;
    r.b = b;
    r.t = std::chrono::steady_clock::now();
    if (trace_level() != 2) return;
    fprintf(stderr, "[scanrs stage] %.3f %s %ld %ld\n", std::chrono::duration<double, std::milli>(r.t.time_since_epoch()).count(), what, a, b);
    fflush(stderr);
}
double sync_timeout_s() { return g_sync_timeout_s.load(std::memory_order_relaxed); }
void set_sync_timeout_s(double s) { g_sync_timeout_s.store(s, std::memory_order_relaxed); }
void *landing_slot(size_t bytes) {
    static char *ring = nullptr;
    static std::atomic<size_t> head{0};
    static std::once_flag once;
    constexpr size_t RING = 1u << 20;
    std::call_once(once, [] {
        void *p = nullptr;
        if (hipHostMalloc(&p, RING, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = malloc(RING); // pageable, but still a place that no stack frame owns
        }
        ring = static_cast<char *>(p);
    });
    const size_t need = (bytes + 7) & ~(size_t)7;
    if (!ring || need > 4096) fail(SCANRS_ERR_DEVICE, "no landing slot of %zu bytes", bytes);
    size_t at = head.fetch_add(need, std::memory_order_relaxed) % RING;
    if (at + need > RING) at = head.fetch_add(need, std::memory_order_relaxed) % RING; // (a slot never straddles the end: the next one does not either)
    if (at + need > RING) at = 0;
    return ring + at;
}
namespace {
// Pinned staging areas of 8 MB for the array copies (histograms, factor verdicts, axis sums, small panels). A copy takes one for
// itself for as long as it waits and hands it back afterwards: the pool's mutex is held only to take and to give (one
// area under one mutex held across the wait made every handle and shard thread queue behind the stream with the longest backlog).
// An area whose wait timed out is NOT given back - the abandoned copy may still land in it. Never unmapped.
struct LandingPool {
    std::mutex mu;
    std::vector<char *> idle;
    static constexpr size_t BYTES = 8u << 20;
};
LandingPool &landing_pool() {
    static LandingPool *a = new LandingPool(); // never destroyed
    return *a;
}
struct LandingLease {
    char *p = nullptr;
    bool keep = true; // cleared when the lease ends in order: a timed-out wait unwinds past `done()` and the area stays out of the pool
    LandingLease() {
        LandingPool &g = landing_pool();
        {
            std::lock_guard<std::mutex> lk(g.mu);
            if (!g.idle.empty()) {
                p = g.idle.back();
                g.idle.pop_back();
            }
        }
        if (!p) {
            void *q = nullptr;
            if (hipHostMalloc(&q, LandingPool::BYTES, hipHostMallocPortable) != hipSuccess) {
                (void)hipGetLastError();
                q = malloc(LandingPool::BYTES);
            }
            p = static_cast<char *>(q);
        }
    }
    void done() { keep = false; }
    ~LandingLease() {
        if (!p || keep) return;
        LandingPool &g = landing_pool();
        std::lock_guard<std::mutex> lk(g.mu);
        g.idle.push_back(p);
    }
};
} // namespace
void d2h_landed_2d(void *dst, const void *dsrc, size_t src_pitch, size_t row_bytes, size_t rows, hipStream_t s, const char *func, const char *file, int line) {
    if (!rows || !row_bytes) return;
    LandingLease a;
    if (!a.p) fail(SCANRS_ERR_DEVICE, "no host staging area for device-to-host copies");
    if (row_bytes > LandingPool::BYTES) fail(SCANRS_ERR_ARGUMENT, "a row of %zu bytes does not fit the host staging area", row_bytes);
    const size_t rows_per = std::max<size_t>(1, LandingPool::BYTES / row_bytes);
    for (size_t r0 = 0; r0 < rows; r0 += rows_per) {
        const size_t nr = std::min(rows_per, rows - r0);
        const char *src = static_cast<const char *>(dsrc) + r0 * src_pitch;
        if (src_pitch == row_bytes)
            SCANRS_HIP(hipMemcpyAsync(a.p, src, nr * row_bytes, hipMemcpyDeviceToHost, s));
        else
            SCANRS_HIP(hipMemcpy2DAsync(a.p, row_bytes, src, src_pitch, row_bytes, nr, hipMemcpyDeviceToHost, s));
        wait_stream(s, func, file, line);
        memcpy(static_cast<char *>(dst) + r0 * row_bytes, a.p, nr * row_bytes);
    }
    a.done();
}
void d2h_landed(void *dst, const void *dsrc, size_t bytes, hipStream_t s, const char *func, const char *file, int line) {
    if (!bytes) return;
    const size_t piece = std::min<size_t>(bytes, 1u << 20);
    const size_t whole = bytes / piece;
    d2h_landed_2d(dst, dsrc, piece, piece, whole, s, func, file, line);
    if (bytes > whole * piece)
        d2h_landed_2d(static_cast<char *>(dst) + whole * piece, static_cast<const char *>(dsrc) + whole * piece, bytes - whole * piece, bytes - whole * piece, 1, s, func, file, line);
}
static const char DEVICE_LOST_TEXT[] = "a device wait of this process timed out earlier (sync_timeout_s) and the device has not been seen idle since: the library "
                                       "does not queue new work or reuse memory that kernels may still be using";
CurrentHandle::CurrentHandle(const Storage *st, bool waits_only) : prev(tl_handle) {
    if (!waits_only && device_lost() && !device_recovered()) fail(SCANRS_ERR_DEVICE, "%s (scanrs_mat_sync waits for a handle's streams)", DEVICE_LOST_TEXT);
    tl_handle = st;
}
CurrentHandle::~CurrentHandle() { tl_handle = prev; }
const Storage *current_handle() { return tl_handle; }
DyingHandle::DyingHandle(const Storage *st) { tl_dying = st; }
DyingHandle::~DyingHandle() { tl_dying = nullptr; }
const Storage *dying_handle() { return tl_dying; }

// Poll `query` (hipSuccess: done, hipErrorNotReady: not yet, anything else: a device error) until the deadline. Spins for the
// first 200 us, then sleeps 20 us per round (about 70 us with the kernel's timer slack), 200 us per round once a second has passed.
// (Until round 6 the long rounds began after 5 ms: svd_bk's waits for the coefficients' verdict, the projection and the Gram matrix last
// 15-35 ms with the device idle until the host reacts — half a round of 250 us lost at each.)
template <typename Q>
static hipError_t poll_until(Q &&query, double timeout_s, double *waited_s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el > timeout_s) {
            if (waited_s) *waited_s = el;
            return hipErrorNotReady;
        }
        if (el < 200e-6)
            std::this_thread::yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(el < 1.0 ? 20 : 200));
    }
}
// "auto scanrs_mat_sync(scanrs_mat *)::(anonymous class)::operator()() const" -> "scanrs_mat_sync": most waits sit inside the lambda
// an entry point hands to guard(), whose own __func__ is "operator()"
static std::string short_func(const char *pretty) {
    std::string s(pretty ? pretty : "?");
    for (const char *cut : {"::(anonymous class)", "::<lambda", "::(lambda"}) {
        const size_t at = s.find(cut);
        if (at != std::string::npos) s.resize(at);
    }
    const size_t paren = s.find('(');
    if (paren != std::string::npos) s.resize(paren);
    const size_t sp = s.rfind(' ');
    if (sp != std::string::npos) s = s.substr(sp + 1);
    return s.empty() ? std::string("?") : s;
}
static const char *base_name(const char *file) {
    const char *b = strrchr(file, '/');
    return b ? b + 1 : file;
}
// message + stderr dump of a wait that ran into its deadline; `waited_stream` is starred among the handle's streams (may be null)
static void timeout_report(const char *kind, const char *pretty_func, const char *file, int line, double waited, hipStream_t waited_stream) {
    const std::string fn = short_func(pretty_func);
    const char *func = fn.c_str();
    char where[160] = "";
    if (tl_handle) { // which of the handle's streams still have work (hipStreamQuery never blocks)
        size_t off = 0;
        for_each_stream(*tl_handle, [&](const char *name, hipStream_t s) {
            if (off >= sizeof(where) || !strcmp(name, "helper")) return; // (the message text is pinned by the bounded-wait tests and by callers that parse it: the four streams it has always named)
            const hipError_t q = hipStreamQuery(s);
            off += (size_t)snprintf(where + off, sizeof(where) - off, "%s%s%s=%s", off ? ", " : "", s == waited_stream ? "*" : "", name,
                                    q == hipSuccess ? "idle" : q == hipErrorNotReady ? "busy" : hipGetErrorString(q));
        });
        (void)hipGetLastError();
    }
    char stages[200] = "";
    {
        size_t off = 0;
        const unsigned n = tl_stages.n, first = n > 4 ? n - 4 : 0;
        const auto now = std::chrono::steady_clock::now();
        for (unsigned i = first; i < n && off < sizeof(stages); i++) {
            const StageRing::Rec &r = tl_stages.rec[i % StageRing::N];
            off += (size_t)snprintf(stages + off, sizeof(stages) - off, "%s%s(%ld) -%.1fs", off ? " > " : "", r.what, r.a,
                                    std::chrono::duration<double>(now - r.t).count());
        }
    }
    fprintf(stderr, "[scanrs] device wait timed out: %s in %s (%s:%d) after %.1f s; streams: %s; last stages: %s\n", kind, func, base_name(file), line,
            waited, where[0] ? where : "n/a", stages[0] ? stages : "none");
    { // the whole ring on stderr
        const unsigned n = tl_stages.n, first = n > StageRing::N ? n - StageRing::N : 0;
        const auto now = std::chrono::steady_clock::now();
        for (unsigned i = first; i < n; i++) {
            const StageRing::Rec &r = tl_stages.rec[i % StageRing::N];
            fprintf(stderr, "[scanrs]   stage %-36s %ld %ld  %.3f s ago\n", r.what, r.a, r.b, std::chrono::duration<double>(now - r.t).count());
        }
        fflush(stderr);
    }
    // From here on the library must assume that kernels and copies of this process are still running: nothing they may touch is
    // reused or freed (device_free_flush leaks), and every later entry point fails fast until device_recovered() has seen the device idle.
    g_device_lost.store(true, std::memory_order_release);
    fail(SCANRS_ERR_DEVICE, "device wait timed out after %.1f s (sync_timeout_s): %s in %s (%s:%d); streams: %s; last stages: %s", waited, kind, func,
         base_name(file), line, where[0] ? where : "n/a", stages[0] ? stages : "none");
}
void wait_stream(hipStream_t s, const char *func, const char *file, int line) {
    double waited = 0.0;
    const hipError_t e = poll_until([&] { return hipStreamQuery(s); }, sync_timeout_s(), &waited);
    if (e == hipSuccess) return;
    if (e == hipErrorNotReady) timeout_report("stream synchronisation", func, file, line, waited, s);
    fail(SCANRS_ERR_DEVICE, "stream synchronisation failed: %s in %s (%s:%d)", hipGetErrorString(e), short_func(func).c_str(), base_name(file), line);
}
void wait_event(hipEvent_t ev, const char *func, const char *file, int line) {
    double waited = 0.0;
    const hipError_t e = poll_until([&] { return hipEventQuery(ev); }, sync_timeout_s(), &waited);
    if (e == hipSuccess) return;
    if (e == hipErrorNotReady) timeout_report("event wait", func, file, line, waited, nullptr);
    fail(SCANRS_ERR_DEVICE, "event wait failed: %s in %s (%s:%d)", hipGetErrorString(e), short_func(func).c_str(), base_name(file), line);
}
void wait_device(const char *func, const char *file, int line) {
    // the null stream of a process is ordered behind every blocking stream: querying it covers "everything queued so far"
    wait_stream(nullptr, func, file, line);
}
template <typename Q>
static bool poll_quiet(Q &&query) noexcept {
    const hipError_t e = poll_until(query, sync_timeout_s(), nullptr);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}
bool wait_stream_quiet(hipStream_t s) noexcept { return poll_quiet([&] { return hipStreamQuery(s); }); }
bool wait_event_quiet(hipEvent_t ev) noexcept { return poll_quiet([&] { return hipEventQuery(ev); }); }
// (the other shard threads of a single-process multi-GPU run rarely all pause at the instant of ONE question: polled, bounded)
bool wait_all_idle_quiet() noexcept {
    return poll_quiet([&] {
        const hipError_t q = hipStreamQuery(nullptr);
        if (q != hipSuccess) return q;
        return all_library_streams_idle() ? hipSuccess : hipErrorNotReady;
    });
}
bool device_ok() {
    static int cached = -1;
    if (cached < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            cached = 0;
        } else {
            hipDeviceProp_t p;
            int dev = 0;
            (void)hipGetDevice(&dev);
            cached = (hipGetDeviceProperties(&p, dev) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ? 1 : 0;
        }
    }
    return cached == 1;
}
// After a timed-out wait: is the device idle again? Non-blocking questions only (hipDeviceSynchronize would be an unbounded wait): the
// null stream is ordered behind every blocking stream, and the library's own streams - the overflow gather's and the helper
// thread's are non-blocking, the legacy stream says nothing about them - are asked one by one through the handles of
// this process. Clears the flag when all of them report idle twice in a row 10 ms apart.
bool device_recovered() {
    if (!device_lost()) return true;
    for (int i = 0; i < 2; i++) {
        if (hipStreamQuery(nullptr) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (!all_library_streams_idle()) return false;
        std::this_thread::sleep_for(std::chrono::milliseconds(10));
    }
    g_device_lost.store(false, std::memory_order_release);
    return true;
}
void need_device() {
    if (!device_ok())
        fail(SCANRS_ERR_DEVICE, "no gfx950 (MI355X) device is usable from this process; scanrs_amd has no CPU fallback");
    if (!device_recovered()) fail(SCANRS_ERR_DEVICE, "%s", DEVICE_LOST_TEXT);
}

} // namespace scanrs

using namespace scanrs;
extern "C" {
const char *scanrs_last_error(void) { return g_err; }
// The bounded wait on an event that is never signalled: the library's own poll loop (poll_until + the timeout report) over a
// query that always answers "not ready" — no HIP call is made, so it runs without a device. Returns SCANRS_ERR_DEVICE after
// `timeout_s` with the message a real stuck wait would leave in scanrs_last_error().
int scanrs_debug_wait_never(double timeout_s) {
    return guard([&] {
        if (!(timeout_s > 0.0)) fail(SCANRS_ERR_ARGUMENT, "timeout must be positive");
        stage_mark("debug: injected wait", 1, 0);
        double waited = 0.0;
        const hipError_t e = poll_until([] { return hipErrorNotReady; }, timeout_s, &waited);
        if (e == hipErrorNotReady) timeout_report("event wait (injected: never signalled)", "scanrs_debug_wait_never", __FILE__, __LINE__, waited, nullptr);
    });
}
} // extern "C"
