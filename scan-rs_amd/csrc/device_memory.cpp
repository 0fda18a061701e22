// Device memory: allocation with retry, deferred frees behind per-stream release events, the block cache and the reserves
// (common.hpp, "device memory"); the pinned host staging buffers kept across handles.
#include <algorithm>

#include "common.hpp"

namespace scanrs {

namespace {
struct Block {
    void *p;
    size_t size; // what hipMalloc was asked for
    int dev;
};
struct Reserve { // one large allocation made ahead of time (scanrs_reserve_device_memory) that later requests are carved from
    char *base;
    size_t size;
    int dev;
    std::map<size_t, size_t> holes; // offset -> length of every unused stretch, neighbours merged: released blocks are reusable at any size
    size_t unused() const {
        size_t n = 0;
        for (auto &h : holes) n += h.second;
        return n;
    }
    bool owns(const void *p) const { return (const char *)p >= base && (const char *)p < base + size; }
    // best fit (the smallest hole that holds it: the big holes stay whole for the big requests); nullptr when none does
    void *take(size_t want) {
        auto best = holes.end();
        for (auto it = holes.begin(); it != holes.end(); ++it)
            if (it->second >= want && (best == holes.end() || it->second < best->second)) best = it;
        if (best == holes.end()) return nullptr;
        const size_t off = best->first, len = best->second;
        holes.erase(best);
        if (len > want) holes.emplace(off + want, len - want);
        return base + off;
    }
    void give(void *p, size_t len) {
        size_t off = (size_t)((char *)p - base);
        auto next = holes.lower_bound(off);
        if (next != holes.begin()) {
            auto prev = std::prev(next);
            if (prev->first + prev->second == off) {
                off = prev->first;
                len += prev->second;
                holes.erase(prev);
            }
        }
        if (next != holes.end() && off + len == next->first) {
            len += next->second;
            holes.erase(next);
        }
        holes.emplace(off, len);
    }
};
struct DeadBlock {
    void *p;
    const Storage *owner; // the handle that was current on the releasing thread (nullptr: none)
    hipEvent_t ev[5];     // recorded at the release on every stream of the owner: work queued before the release is done when they are
    int n_ev;
    int ev_dev;           // the device those events belong to (an event records only on streams of the device it was created on)
};
struct DeviceMemory {
    std::mutex mu;
    std::vector<DeadBlock> dead;                        // released by their owners, waiting for their release events
    std::map<int, std::vector<hipEvent_t>> release_events; // spare events by device (created once, reused; ADVICE r5: one pool for all devices handed a shard thread another device's event)
    size_t ownerless = 0;                               // entries of `dead` without an owner: they wait for a moment at which every library stream is idle
    std::map<void *, std::pair<size_t, int>> live;      // every block handed out: pointer -> (size, device)
    std::vector<Reserve> reserves;                      // blocks carved from a reserve go back into it (Reserve::give), never to the driver one by one
    std::multimap<std::pair<int, size_t>, void *> idle; // cached blocks by (device, size)
    size_t idle_bytes = 0;
    double cache_fraction = 0.5; // of the device's memory; 0: no cache (every released block goes back to the driver)
};
DeviceMemory &devmem() {
    static DeviceMemory *g = new DeviceMemory(); // never destroyed: handles freed by static destructors of the host program still find it
    return *g;
}
std::atomic<uint64_t> g_alloc_us{0}, g_alloc_calls{0};
constexpr size_t CACHE_MIN = 1u << 20; // smaller blocks go straight back
size_t round_block(size_t bytes) { return bytes >= CACHE_MIN ? (bytes + (2u << 20) - 1) & ~((size_t)(2u << 20) - 1) : bytes; }
} // namespace
// A released block may be handed out again once everything that was queued BEFORE the release, on any stream of the releasing handle
// (main, the two auxiliary ones, the overflow gather's, the helper thread's), has run: one event per such stream, recorded here. Work
// queued later cannot name the block. (hipFree used to give this guarantee by waiting for the whole device; ADVICE r4: a process-wide
// list flushed by whoever saw its own main stream idle did not.)
void device_free_later(void *p, size_t) {
    if (!p) return;
    DeadBlock db{p, current_handle(), {nullptr, nullptr, nullptr, nullptr, nullptr}, 0, 0};
    DeviceMemory &g = devmem();
    (void)hipGetDevice(&db.ev_dev); // (the handle's streams live on the device that is current on the thread that works for it)
    if (!db.owner && dying_handle()) {
        db.owner = dying_handle(); // a member of a handle that is being destroyed: its destructor has drained every stream that could name the block
    } else if (const Storage *st = db.owner) {
        for_each_stream(*st, [&](const char *, hipStream_t q) {
            hipEvent_t e = nullptr;
            {
                std::lock_guard<std::mutex> lk(g.mu);
                auto &pool = g.release_events[db.ev_dev];
                if (!pool.empty()) {
                    e = pool.back();
                    pool.pop_back();
                }
            }
            if ((!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) || hipEventRecord(e, q) != hipSuccess) {
                (void)hipGetLastError();
                if (e) (void)hipEventDestroy(e);
                db.owner = nullptr; // no proof of completion for this one: it waits for a device-wide idle point
                return;
            }
            db.ev[db.n_ev++] = e;
        });
    }
    std::lock_guard<std::mutex> lk(g.mu);
    if (!db.owner) g.ownerless++;
    g.dead.push_back(db);
}
// Released blocks of 1 MB and more are kept for the next allocation of about their size instead of going back to the driver:
// VRAM that was just freed is scrubbed in the background and an allocation that lands on it waits for the scrubber — seconds for
// the tens of GB a handle holds (the second and third handle of one process took 2.4 / 4.1 s for their first PCA instead of 0.4).
// At most `device_cache_fraction` (default one half) of the device's memory is kept; scanrs_release_cached_memory() and a failed
// allocation empty the cache.
// Moves released blocks to the cache (or back to the driver): those whose release events have completed (device_free_later); with
// `owner_gone` also every block of that (destroyed) handle; with `everything` (the caller has just seen the whole device idle) all.
static void device_free_flush_impl(const Storage *owner, bool owner_gone, bool everything, bool cache_only = false) noexcept {
    DeviceMemory &g = devmem();
    if (device_lost()) return; // kernels of a timed-out call may still use them: leaked on purpose
    std::vector<Block> to_free;
    // Blocks released while no handle was current carry no events (every reset_map + normalize cycle stranded the old map
    // arrays until an out-of-memory retry wiped the cache). They may go once every stream of the library has been seen idle: work
    // queued before their release is done then, work queued later cannot name them. (Asked outside the lock: the handles' own mutex.)
    bool ownerless_done = everything;
    if (!ownerless_done && !cache_only) {
        bool any = false;
        {
            std::lock_guard<std::mutex> lk(g.mu);
            any = g.ownerless > 0;
        }
        if (any) {
            ownerless_done = hipStreamQuery(nullptr) == hipSuccess && all_library_streams_idle();
            if (!ownerless_done) (void)hipGetLastError();
        }
    }
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (g.dead.empty()) return;
        size_t cap = 0;
        if (g.cache_fraction > 0.0) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess) cap = (size_t)((double)tot * g.cache_fraction);
        }
        std::vector<DeadBlock> keep;
        for (DeadBlock &db : g.dead) {
            // done with: its release events have all completed / its owner is gone (streams drained by the destructor) / the caller has
            // just seen the whole device idle. A block released outside any handle waits for the last case.
            bool done = everything || (owner_gone && db.owner == owner) || (ownerless_done && db.owner == nullptr);
            if (!done && db.owner != nullptr) {
                done = true;
                for (int i = 0; i < db.n_ev && done; i++) {
                    const hipError_t e = hipEventQuery(db.ev[i]);
                    if (e != hipSuccess) {
                        (void)hipGetLastError();
                        done = false;
                    }
                }
            }
            if (!done) {
                keep.push_back(db);
                continue;
            }
            void *p = db.p;
            auto it = g.live.find(p);
            if (!db.owner && g.ownerless) g.ownerless--;
            if (it == g.live.end()) { // not ours (cannot happen)
                for (int i = 0; i < db.n_ev; i++) g.release_events[db.ev_dev].push_back(db.ev[i]);
                continue;
            }
            const Block b{p, it->second.first, it->second.second};
            Reserve *home = nullptr;
            for (Reserve &r : g.reserves)
                if (r.owns(p)) home = &r;
            size_t idle_dev = 0; // what the cache holds for THIS block's device (the limit is a share of one device's memory)
            for (auto ii = g.idle.lower_bound(std::make_pair(b.dev, (size_t)0)); ii != g.idle.end() && ii->first.first == b.dev; ++ii) idle_dev += ii->first.second;
            const bool to_cache = home || (b.size >= CACHE_MIN && idle_dev + b.size <= cap);
            if (!to_cache && cache_only) { // in the middle of a call: hipFree would wait for the whole device, the block stays on the list
                if (!db.owner) g.ownerless++;
                keep.push_back(db);
                continue;
            }
            for (int i = 0; i < db.n_ev; i++) g.release_events[db.ev_dev].push_back(db.ev[i]);
            g.live.erase(it);
            if (home) {
                home->give(p, b.size);
            } else if (to_cache) {
                g.idle.emplace(std::make_pair(b.dev, b.size), p);
                g.idle_bytes += b.size;
            } else {
                to_free.push_back(b);
            }
        }
        g.dead.swap(keep);
    }
    if (to_free.empty()) return;
    const auto t0 = std::chrono::steady_clock::now();
    size_t bytes = 0;
    for (auto &b : to_free) {
        (void)hipFree(b.p);
        bytes += b.size;
    }
    if (trace_on())
        fprintf(stderr, "[scanrs trace] released %zu buffers, %.2f GB, in %.2f ms\n", to_free.size(), (double)bytes / 1e9,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}
void device_free_flush() noexcept { device_free_flush_impl(current_handle(), false, false); }
// the handle at `owner` has been destroyed (its streams were drained by its destructor): its blocks can go
void device_free_flush_owner_gone(const void *owner) noexcept { device_free_flush_impl(static_cast<const Storage *>(owner), true, false); }
void device_cache_release() noexcept {
    // every owner's blocks: only behind a wait for the whole device (bounded like every other wait; if it does not come, nothing is released)
    if (device_lost() || !wait_all_idle_quiet()) return;
    device_free_flush_impl(nullptr, false, true);
    DeviceMemory &g = devmem();
    std::vector<void *> take;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        for (auto it = g.idle.begin(); it != g.idle.end();) {
            take.push_back(it->second);
            g.idle_bytes -= it->first.second;
            it = g.idle.erase(it);
        }
        for (auto it = g.reserves.begin(); it != g.reserves.end();) { // a reserve nothing is handed out from any more goes back whole
            if (it->unused() == it->size) {
                take.push_back(it->base);
                it = g.reserves.erase(it);
            } else {
                ++it;
            }
        }
    }
    for (void *p : take) (void)hipFree(p);
}
void device_reserve(size_t bytes) {
    if (!bytes) return;
    DeviceMemory &g = devmem();
    int dev = 0;
    (void)hipGetDevice(&dev);
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(SCANRS_ERR_DEVICE, "reserving %.2f GB of device memory failed: %s", (double)bytes / 1e9, hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lk(g.mu);
    Reserve r{(char *)p, bytes, dev, {}};
    r.holes.emplace(0, bytes);
    g.reserves.push_back(std::move(r));
}
void device_cache_set_fraction(double f) {
    DeviceMemory &g = devmem();
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.cache_fraction = f;
    }
    if (f <= 0.0) device_cache_release();
}
size_t device_cache_bytes() { // cached blocks of the CURRENT device (a single-process multi-GPU program has one cache per device in the same map)
    DeviceMemory &g = devmem();
    device_free_flush_impl(nullptr, false, false, true); // released blocks whose events have completed count
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g.mu);
    size_t n = 0;
    for (auto it = g.idle.lower_bound(std::make_pair(dev, (size_t)0)); it != g.idle.end() && it->first.first == dev; ++it) n += it->first.second;
    return n;
}
// what scanrs_reserve_device_memory set aside on this device and nobody has been handed yet
size_t device_reserve_unused_bytes() {
    DeviceMemory &g = devmem();
    device_free_flush_impl(nullptr, false, false, true);
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g.mu);
    size_t n = 0;
    for (const Reserve &r : g.reserves)
        if (r.dev == dev) n += r.unused();
    return n;
}
// SCANRS_TRACE: what the library holds on the device, block by block (>= 256 MB), and what its reserves have left
void device_memory_report(const char *why) {
    DeviceMemory &g = devmem();
    std::lock_guard<std::mutex> lk(g.mu);
    std::vector<size_t> big;
    size_t live = 0, dead = 0;
    for (auto &kv : g.live) {
        live += kv.second.first;
        if (kv.second.first >= (256u << 20)) big.push_back(kv.second.first);
    }
    for (auto &db : g.dead) {
        auto it = g.live.find(db.p);
        if (it != g.live.end()) dead += it->second.first;
    }
    std::sort(big.begin(), big.end(), std::greater<size_t>());
    fprintf(stderr, "[scanrs trace] device memory (%s): %.2f GB in %zu blocks (%.2f GB of them released, waiting for their events), %.2f GB cached; blocks of 256 MB and more:", why,
            (double)live / 1e9, g.live.size(), (double)dead / 1e9, (double)g.idle_bytes / 1e9);
    for (size_t b : big) fprintf(stderr, " %.2f", (double)b / 1e9);
    fprintf(stderr, "\n");
    for (const Reserve &r : g.reserves) {
        fprintf(stderr, "[scanrs trace]   reserve of %.2f GB on device %d, unused %.2f GB in %zu stretches:", (double)r.size / 1e9, r.dev, (double)r.unused() / 1e9, r.holes.size());
        for (auto &h : r.holes) fprintf(stderr, " %.2f", (double)h.second / 1e9);
        fprintf(stderr, "\n");
    }
}
size_t device_live_bytes() {
    DeviceMemory &g = devmem();
    std::lock_guard<std::mutex> lk(g.mu);
    size_t n = 0;
    for (auto &kv : g.live) n += kv.second.first;
    return n;
}
void *device_alloc(size_t bytes) {
    DeviceMemory &g = devmem();
    const size_t want = round_block(bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (want >= CACHE_MIN) { // a cached block of this size, or up to 1/8 larger
        bool any_dead;
        {
            std::lock_guard<std::mutex> lk(g.mu);
            any_dead = !g.dead.empty();
        }
        if (any_dead) device_free_flush_impl(nullptr, false, false, true); // blocks whose release events have completed join the cache first
        std::lock_guard<std::mutex> lk(g.mu);
        auto it = g.idle.lower_bound(std::make_pair(dev, want));
        if (it != g.idle.end() && it->first.first == dev && it->first.second <= want + want / 8) {
            void *p = it->second;
            g.live[p] = std::make_pair(it->first.second, dev);
            g.idle_bytes -= it->first.second;
            g.idle.erase(it);
            return p;
        }
    }
    if (want >= CACHE_MIN) { // carve from a reserve made ahead of time
        std::lock_guard<std::mutex> lk(g.mu);
        for (Reserve &r : g.reserves) {
            if (r.dev != dev) continue;
            if (void *p = r.take(want)) {
                g.live[p] = std::make_pair(want, dev);
                return p;
            }
        }
    }
    if (want >= (1u << 30) && trace_on()) device_memory_report("no cached block and no reserve holds the request, asking the driver");
    void *p = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&p, want);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) { // cached blocks and buffers waiting for their release may be all that stands in the way
        (void)hipGetLastError();
        device_cache_release();
        e = hipMalloc(&p, want);
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    g_alloc_us.fetch_add((uint64_t)us, std::memory_order_relaxed);
    g_alloc_calls.fetch_add(1, std::memory_order_relaxed);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(SCANRS_ERR_DEVICE, "hipMalloc of %.3f GB failed: %s", (double)want / 1e9, hipGetErrorString(e));
    }
    if (us > 2000.0 && trace_on()) fprintf(stderr, "[scanrs trace]   hipMalloc of %.2f GB took %.1f ms\n", (double)want / 1e9, us / 1e3);
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.live[p] = std::make_pair(want, dev);
    }
    return p;
}
uint64_t device_alloc_us() { return g_alloc_us.load(std::memory_order_relaxed); }
uint64_t device_alloc_calls() { return g_alloc_calls.load(std::memory_order_relaxed); }

// ---- pinned host staging buffers, kept across handles ------------------------------------------------------------------------
// A handle stages its seeded start panel (26 MB) and the delivery of V (ring of 8 x 8 MB) through pinned memory; pinning 64 MB costs
// 5-8 ms, once per handle until round 4. Buffers go back to a small pool when their handle dies, and scanrs_init() pins the first
// one ahead of the first call (portable: usable from every device of a single-process multi-GPU program).
namespace {
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> idle;
    size_t idle_bytes = 0;
};
PinnedPool &pinned_pool() {
    static PinnedPool *p = new PinnedPool(); // never destroyed: handles may outlive static destruction order
    return *p;
}
} // namespace
void *pinned_take(size_t bytes, size_t *got) {
    PinnedPool &g = pinned_pool();
    {
        std::lock_guard<std::mutex> lk(g.mu);
        int best = -1;
        for (int i = 0; i < (int)g.idle.size(); i++)
            if (g.idle[i].second >= bytes && (best < 0 || g.idle[i].second < g.idle[best].second)) best = i;
        if (best >= 0) {
            void *p = g.idle[best].first;
            *got = g.idle[best].second;
            g.idle_bytes -= *got;
            g.idle.erase(g.idle.begin() + best);
            return p;
        }
    }
    void *p = nullptr;
    SCANRS_HIP(hipHostMalloc(&p, bytes, hipHostMallocPortable));
    *got = bytes;
    return p;
}
void pinned_give(void *p, size_t bytes) noexcept {
    if (!p) return;
    PinnedPool &g = pinned_pool();
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (g.idle.size() < 4 && g.idle_bytes + bytes <= ((size_t)1 << 30)) {
            g.idle.emplace_back(p, bytes);
            g.idle_bytes += bytes;
            return;
        }
    }
    (void)hipHostFree(p);
}

// scanrs_debug_arena_selftest: random take / give rounds on a Reserve over addresses nobody dereferences, the books checked after each
void reserve_selftest(uint32_t rounds, uint64_t seed) {
    constexpr size_t UNIT = 2u << 20;
    Reserve r{reinterpret_cast<char *>((uintptr_t)1 << 40), 512 * UNIT, 0, {}};
    r.holes.emplace(0, r.size);
    std::map<char *, size_t> live; // base -> length
    uint64_t z = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() {
        z ^= z << 13;
        z ^= z >> 7;
        z ^= z << 17;
        return z;
    };
    auto check = [&]() {
        size_t held = 0;
        char *prev_end = r.base;
        for (auto &b : live) {
            if (b.first < prev_end || b.first + b.second > r.base + r.size) fail(SCANRS_ERR_NUMERICAL, "arena selftest: a live block overlaps its neighbour or leaves the range");
            prev_end = b.first + b.second;
            held += b.second;
        }
        if (held + r.unused() != r.size) fail(SCANRS_ERR_NUMERICAL, "arena selftest: %zu bytes held + %zu unused != %zu", held, r.unused(), r.size);
        size_t end_prev = (size_t)-1;
        for (auto &h : r.holes) {
            if (h.second == 0 || h.first == end_prev) fail(SCANRS_ERR_NUMERICAL, "arena selftest: an empty hole, or two holes that should have merged");
            end_prev = h.first + h.second;
            for (auto &b : live) // no hole inside a live block
                if (r.base + h.first < b.first + b.second && b.first < r.base + h.first + h.second) fail(SCANRS_ERR_NUMERICAL, "arena selftest: a hole overlaps a live block");
        }
    };
    for (uint32_t i = 0; i < rounds; i++) {
        if (live.empty() || (rnd() % 3u) != 0u) {
            const size_t want = (1 + rnd() % 40) * UNIT;
            if (void *p = r.take(want)) {
                live[static_cast<char *>(p)] = want;
            } else { // no hole holds it: then no hole may be that large
                for (auto &h : r.holes)
                    if (h.second >= want) fail(SCANRS_ERR_NUMERICAL, "arena selftest: a request was refused although a hole holds it");
            }
        } else {
            auto it = live.begin();
            std::advance(it, (long)(rnd() % live.size()));
            r.give(it->first, it->second);
            live.erase(it);
        }
        check();
    }
    while (!live.empty()) {
        r.give(live.begin()->first, live.begin()->second);
        live.erase(live.begin());
        check();
    }
    if (r.holes.size() != 1 || r.holes.begin()->first != 0 || r.holes.begin()->second != r.size) fail(SCANRS_ERR_NUMERICAL, "arena selftest: the arena is not whole at the end");
}

} // namespace scanrs
