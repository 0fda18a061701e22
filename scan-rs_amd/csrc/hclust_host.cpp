// Host logic of hclust (hclust/src/lib.rs): the driver of the device chain (hclust.hip), its host twin, kodama's naming of the
// finished merges (shared with linkage.rs' relabel in cluster_host.cpp), and what the reference does with a dendrogram: leaves
// (:150-206), merge_clusters_below_distance_threshold (:210-227), fcluster (:231-239), relabel_vector (:122-125).
#include "common.hpp"
#include "hclust_lw.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

struct scanrs_hclust {
    uint64_t n = 0;
    std::vector<uint32_t> c1, c2, size;
    std::vector<double> diss;
    // chain steps, launches, batches waited for, bytes of the matrix, us of the distance pass, us of the chain, merges
    uint64_t info[7] = {0, 0, 0, 0, 0, 0, 0};
};

namespace scanrs {
namespace {

constexpr uint64_t HOST_TWIN_MAX_N = 20000; // the twin's matrix lives in host memory: tests and small inputs

const char *method_name(int method) {
    static const char *names[] = {"Single", "Complete", "Average", "Weighted", "Ward", "Centroid", "Median"};
    return method >= 0 && method <= 6 ? names[method] : "?";
}

void check_method(int method) {
    if (method < HC_SINGLE || method > HC_MEDIAN) fail(SCANRS_ERR_ARGUMENT, "unknown linkage method %d", method);
    if (method == HC_CENTROID || method == HC_MEDIAN)
        fail(SCANRS_ERR_ARGUMENT, "linkage method %s is not provided: it is not reducible, and the nearest-neighbour chain does not compute it",
             method_name(method));
}

void check_n(uint64_t n) {
    if (n < 2) fail(SCANRS_ERR_SHAPE, "Need at least two elements to do hierarchical clustering");
    if (n > 0x7FFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "at most 2^31 - 1 observations");
}

// the merges in discovery order -> kodama's dendrogram: stable sort by height, the cluster of sorted step i named n + i,
// cluster1 < cluster2, size = observations; Ward's heights were squared until here
void finish(scanrs_hclust &h, uint64_t n, int method, const uint32_t *ma, const uint32_t *mb, const double *mh) {
    std::vector<double> z((n - 1) * 4), zo((n - 1) * 4);
    for (uint64_t i = 0; i + 1 < n; i++) {
        z[i * 4] = (double)ma[i];
        z[i * 4 + 1] = (double)mb[i];
        z[i * 4 + 2] = mh[i];
        z[i * 4 + 3] = 0.0;
    }
    cluster_sort_relabel(z.data(), n, zo.data());
    h.n = n;
    h.c1.resize(n - 1);
    h.c2.resize(n - 1);
    h.size.resize(n - 1);
    h.diss.resize(n - 1);
    for (uint64_t i = 0; i + 1 < n; i++) {
        h.c1[i] = (uint32_t)zo[i * 4];
        h.c2[i] = (uint32_t)zo[i * 4 + 1];
        h.diss[i] = method == HC_WARD ? std::sqrt(zo[i * 4 + 2]) : zo[i * 4 + 2];
        h.size[i] = (uint32_t)zo[i * 4 + 3];
    }
}

// Finite coordinates do not make finite dissimilarities: a squared difference overflows beyond about 1.3e154, and a Lance-Williams
// update multiplies by cluster sizes. Neither side lets such a value into the chain (a row without a finite entry yields no candidate).
[[noreturn]] void refuse_distance(uint64_t i, uint64_t j) {
    fail(SCANRS_ERR_ARGUMENT, "the distance between observations %llu and %llu is not finite: the squared differences of their coordinates overflow",
         (unsigned long long)i, (unsigned long long)j);
}
[[noreturn]] void refuse_update(int error, uint64_t merges, int method) {
    if (error == 1)
        fail(SCANRS_ERR_NUMERICAL, "a dissimilarity overflowed in the Lance-Williams update of merge %llu (%s linkage): the distances are too large for it",
             (unsigned long long)merges, method_name(method));
    fail(SCANRS_ERR_NUMERICAL, "the nearest-neighbour chain found no finite dissimilarity after %llu merges", (unsigned long long)merges);
}

// ---- the host twin: the device chain's steps, one for one, in plain C++ ---------------------------------------------------------------
void twin_linkage(const double *obs, uint64_t n, uint32_t d, int method, scanrs_hclust &h) {
    if (n > HOST_TWIN_MAX_N) fail(SCANRS_ERR_ARGUMENT, "the host twin serves tests and small inputs: at most %llu observations", (unsigned long long)HOST_TWIN_MAX_N);
    for (uint64_t e = 0; e < n * d; e++)
        if (!std::isfinite(obs[e]))
            fail(SCANRS_ERR_ARGUMENT, "element %llu (row %llu, column %llu) is not finite", (unsigned long long)e, (unsigned long long)(e / d),
                 (unsigned long long)(e % d));
    std::vector<double> dist(n * n);
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t j = i; j < n; j++) {
            const double s = hclust_sqdist(obs + i * d, obs + j * d, d);
            const double v = method == HC_WARD ? s : std::sqrt(s);
            dist[i * n + j] = v;
            dist[j * n + i] = v;
            if (!std::isfinite(v)) refuse_distance(i, j); // (pairs in row-major order: the first one, as the device's minimum)
        }
    std::vector<uint32_t> chain(n), size(n, 1), ma(n - 1), mb(n - 1);
    std::vector<double> mh(n - 1);
    uint64_t len = 0, merges = 0, steps = 0;
    while (merges + 1 < n) {
        if (steps >= 3 * n) fail(SCANRS_ERR_NUMERICAL, "the nearest-neighbour chain took %llu steps for %llu observations", (unsigned long long)steps, (unsigned long long)n);
        steps++;
        uint32_t a;
        if (len == 0) {
            a = 0;
            while (size[a] == 0) a++;
            len = 1;
        } else {
            a = chain[len - 1];
        }
        const double *row = &dist[(uint64_t)a * n];
        double v = INFINITY;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t j = 0; j < n; j++) {
            if (j == a || size[j] == 0) continue;
            if (hclust_better(row[j], j, v, c)) {
                v = row[j];
                c = j;
            }
        }
        if (c == 0xFFFFFFFFu || !std::isfinite(v)) refuse_update(2, merges, method);
        const uint32_t prev = len > 1 ? chain[len - 2] : 0xFFFFFFFFu;
        if (len > 1 && !(v < row[prev])) c = prev;
        if (len > 1 && c == prev) {
            const uint32_t lo = std::min(a, c), hi = std::max(a, c);
            const uint32_t sl = size[lo], sh = size[hi];
            ma[merges] = lo;
            mb[merges] = hi;
            mh[merges] = row[prev];
            size[lo] = 0;
            size[hi] = sl + sh;
            len -= 2;
            merges++;
            const double dab = dist[(uint64_t)lo * n + hi];
            for (uint32_t k = 0; k < n; k++) {
                if (k == lo || k == hi || size[k] == 0) continue;
                const double nv = hclust_lw(method, dist[(uint64_t)lo * n + k], dist[(uint64_t)hi * n + k], dab, (double)sl, (double)sh, (double)size[k]);
                dist[(uint64_t)hi * n + k] = nv;
                dist[(uint64_t)k * n + hi] = nv;
                if (!std::isfinite(nv)) refuse_update(1, merges, method);
            }
        } else {
            if (len == 1) chain[0] = a;
            chain[len++] = c;
        }
    }
    finish(h, n, method, ma.data(), mb.data(), mh.data());
    h.info[0] = steps;
    h.info[6] = merges;
}

// ---- the device chain -------------------------------------------------------------------------------------------------------------
struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    Events() {
        for (auto &x : e) {
            const hipError_t err = hipEventCreate(&x);
            if (err != hipSuccess) { // (a constructor that throws runs no destructor: the events made so far go here)
                x = nullptr;
                destroy();
                fail(SCANRS_ERR_DEVICE, "hipEventCreate failed: %s", hipGetErrorString(err));
            }
        }
    }
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { destroy(); }
    void destroy() noexcept {
        for (auto &x : e) {
            if (x) (void)hipEventDestroy(x);
            x = nullptr;
        }
    }
};

// the n x n matrix beside what the library has set aside: what the driver reports free, the cached blocks (a failed allocation
// empties the cache) and the unused part of the reserves
void check_matrix_fits(uint64_t n, uint64_t bytes) {
    size_t fr = 0, tot = 0;
    SCANRS_HIP(hipMemGetInfo(&fr, &tot));
    const uint64_t have = (uint64_t)fr + device_cache_bytes() + device_reserve_unused_bytes();
    if (bytes > have)
        fail(SCANRS_ERR_DEVICE, "the distance matrix of n = %llu observations needs %llu bytes of device memory, %llu are available",
             (unsigned long long)n, (unsigned long long)bytes, (unsigned long long)have);
}

// d_x: the array as given (device memory). Fills d_dist; returns after the pass is queued (nothing waited for)
void queue_pdist(hipStream_t s, const double *d_x, uint64_t n, uint32_t d, uint64_t ld, int by_cols, int squared, DevBuf<double> &d_obs,
                 DevBuf<unsigned long long> &d_bad, double *d_dist) {
    d_obs.alloc(std::max<uint64_t>(1, n * d));
    d_bad.alloc(2); // [0] the first element that is not finite, [1] the first pair whose distance is not
    launch_hclust_pack(s, d_x, n, d, ld, by_cols, d_obs.p, d_bad.p);
    launch_hclust_pdist(s, d_obs.p, n, d, squared, d_dist, d_bad.p + 1);
}

void refuse_not_finite(unsigned long long bad, uint64_t cols) {
    if (bad != ~0ull)
        fail(SCANRS_ERR_ARGUMENT, "element %llu (row %llu, column %llu) is not finite", bad, bad / cols, bad % cols);
}

void device_linkage(const double *d_x, uint64_t rows, uint64_t cols, uint64_t ld, int direction, int method, const scanrs_snoop *snoop,
                    scanrs_hclust &h) {
    const uint64_t n = direction ? cols : rows, d64 = direction ? rows : cols;
    const uint32_t d = (uint32_t)d64, n32 = (uint32_t)n;
    if (n > (1ull << 30)) fail(SCANRS_ERR_DEVICE, "the distance matrix of n = %llu observations needs more than 2^63 bytes of device memory", (unsigned long long)n);
    const uint64_t bytes = n * n * 8;
    const hipStream_t s = nullptr;
    check_matrix_fits(n, bytes);
    DevBuf<double> d_dist;
    try {
        d_dist.alloc(n * n);
    } catch (const Failure &) {
        fail(SCANRS_ERR_DEVICE, "the distance matrix of n = %llu observations needs %llu bytes of device memory, and the allocation failed",
             (unsigned long long)n, (unsigned long long)bytes);
    }
    DevBuf<double> d_obs, d_mh(n - 1);
    DevBuf<unsigned long long> d_bad, d_ctr(4);
    DevBuf<uint32_t> d_chain(n), d_size(n), d_rec(8), d_ma(n - 1), d_mb(n - 1), d_msize(n - 1);
    Events ev;
    SCANRS_HIP(hipEventRecord(ev.e[0], s));
    queue_pdist(s, d_x, n, d, ld, direction, method == HC_WARD, d_obs, d_bad, d_dist.p);
    SCANRS_HIP(hipEventRecord(ev.e[1], s));
    {
        unsigned long long bad[2] = {0, 0};
        SCANRS_D2H(bad, d_bad.p, sizeof(bad), s);
        refuse_not_finite(bad[0], cols);
        if (bad[1] != ~0ull) refuse_distance(bad[1] / n, bad[1] % n);
    }
    {
        const std::vector<uint32_t> ones(n, 1);
        h2d(d_size.p, ones.data(), n, s);
        SCANRS_HIP(hipMemsetAsync(d_ctr.p, 0, 4 * 8, s));
        SCANRS_HIP(hipMemsetAsync(d_rec.p, 0, 8 * 4, s));
        SCANRS_SYNC(s); // (`ones` is pageable host memory)
    }
    // Steps are queued blindly; between batches the host reads the four counters and nothing else. At most 3n steps are ever queued:
    // a chain of n observations ends within 3 (n - 1) of them, and steps behind the last merge return at once.
    uint64_t queued = 0, merges = 0, steps = 0, batches = 0;
    const uint64_t bound = 3 * n;
    while (merges + 1 < n) {
        if (queued >= bound)
            fail(SCANRS_ERR_NUMERICAL, "the nearest-neighbour chain made %llu of %llu merges in %llu steps", (unsigned long long)merges,
                 (unsigned long long)(n - 1), (unsigned long long)queued);
        const uint64_t batch = std::min<uint64_t>(bound - queued, std::min<uint64_t>(2048, std::max<uint64_t>(32, n - 1 - merges)));
        for (uint64_t i = 0; i < batch; i++)
            launch_hclust_step(s, d_dist.p, n32, method, d_chain.p, d_size.p, d_ctr.p, d_rec.p, d_ma.p, d_mb.p, d_mh.p, d_msize.p);
        SCANRS_HIP(hipGetLastError());
        queued += batch;
        unsigned long long ctr[4] = {0, 0, 0, 0};
        SCANRS_D2H(ctr, d_ctr.p, sizeof(ctr), s);
        batches++;
        merges = ctr[1];
        steps = ctr[2];
        if (ctr[3]) refuse_update((int)ctr[3], merges, method); // (the stream is idle: the steps behind the error returned at once)
        snoop_poll(snoop, (double)merges / (double)(n - 1));
    }
    SCANRS_HIP(hipEventRecord(ev.e[2], s));
    std::vector<uint32_t> ma(n - 1), mb(n - 1);
    std::vector<double> mh(n - 1);
    SCANRS_D2H(ma.data(), d_ma.p, (n - 1) * 4, s);
    SCANRS_D2H(mb.data(), d_mb.p, (n - 1) * 4, s);
    SCANRS_D2H(mh.data(), d_mh.p, (n - 1) * 8, s);
    SCANRS_SYNC_EVENT(ev.e[2]);
    float ms_p = 0.f, ms_c = 0.f;
    SCANRS_HIP(hipEventElapsedTime(&ms_p, ev.e[0], ev.e[1]));
    SCANRS_HIP(hipEventElapsedTime(&ms_c, ev.e[1], ev.e[2]));
    finish(h, n, method, ma.data(), mb.data(), mh.data());
    h.info[0] = steps;
    h.info[1] = 2 * queued + 2;
    h.info[2] = batches;
    h.info[3] = bytes;
    h.info[4] = (uint64_t)std::llround((double)ms_p * 1000.0);
    h.info[5] = (uint64_t)std::llround((double)ms_c * 1000.0);
    h.info[6] = merges;
}

void create_common(const double *x, bool on_device, uint64_t rows, uint64_t cols, uint64_t ld, int direction, int method, const scanrs_snoop *snoop,
                   scanrs_hclust **out) {
    if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
    *out = nullptr;
    if (direction != SCANRS_CLUSTER_ROWS && direction != SCANRS_CLUSTER_COLUMNS) fail(SCANRS_ERR_ARGUMENT, "unknown cluster direction %d", direction);
    check_method(method);
    const uint64_t n = direction ? cols : rows, d = direction ? rows : cols;
    check_n(n);
    if (d > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "at most 2^32 - 1 dimensions");
    if (ld < cols) fail(SCANRS_ERR_ARGUMENT, "ld must be at least cols");
    if (!x && rows && cols) fail(SCANRS_ERR_ARGUMENT, "null argument");
    need_device();
    CurrentHandle cur(nullptr); // (refuses while an earlier timed-out wait has not been cleared)
    snoop_check(snoop);         // a flag that is already set: nothing is queued
    std::unique_ptr<scanrs_hclust> h(new scanrs_hclust());
    // where the call ends, by any way out: what it released joins the cache or goes back to the driver (the buffers below and
    // device_linkage's are gone before this runs; after a timed-out wait the flush keeps everything, as it must)
    struct FlushAtEnd {
        ~FlushAtEnd() { device_free_flush(); }
    } flush_at_end;
    DevBuf<double> d_x;
    const double *src = x;
    if (!on_device) {
        const uint64_t count = rows ? (rows - 1) * ld + cols : 0;
        d_x.alloc(std::max<uint64_t>(1, count));
        if (count) {
            SCANRS_HIP(hipMemcpyAsync(d_x.p, x, count * 8, hipMemcpyHostToDevice, nullptr));
            SCANRS_SYNC(nullptr); // (the caller's array may be pageable)
        }
        src = d_x.p;
    }
    device_linkage(src, rows, cols, ld, direction, method, snoop, *h);
    *out = h.release();
}

void need_handle(const scanrs_hclust *h) {
    if (!h) fail(SCANRS_ERR_ARGUMENT, "null handle");
}

// ---- SimpleOrdering (hclust/src/lib.rs:74-116) and the two rules of :150-193 -----------------------------------------------------
constexpr uint32_t NONE = 0xFFFFFFFFu;
void leaves(const scanrs_hclust &h, int ordering, uint32_t *out) {
    const uint64_t n = h.n;
    std::vector<uint32_t> left(2 * n - 1, NONE), right(2 * n - 1, NONE), nb_left(n, NONE), nb_right(n, NONE);
    for (uint64_t i = 0; i < n; i++) left[i] = right[i] = (uint32_t)i;
    std::vector<double> min_diss;
    if (ordering == SCANRS_LEAF_MODULAR_SMALLEST) {
        min_diss.assign(2 * n - 1, std::numeric_limits<double>::max());
        for (uint64_t i = 0; i + 1 < n; i++) // f64::min: a NaN loses (there is none: heights are finite or +inf)
            min_diss[n + i] = std::fmin(std::fmin(min_diss[h.c1[i]], min_diss[h.c2[i]]), h.diss[i]);
    }
    for (uint64_t i = 0; i + 1 < n; i++) {
        const uint32_t c1 = h.c1[i], c2 = h.c2[i];
        const bool first_left = ordering == SCANRS_LEAF_NAIVE ? c1 < c2 : min_diss[c1] <= min_diss[c2];
        const uint32_t l = first_left ? c1 : c2, r = first_left ? c2 : c1;
        left[n + i] = left[l];
        right[n + i] = right[r];
        nb_right[right[l]] = left[r];
        nb_left[left[r]] = right[l];
    }
    uint64_t start = 0;
    while (start < n && nb_left[start] != NONE) start++;
    uint64_t k = 0;
    for (uint32_t at = (uint32_t)start; at != NONE && k < n; at = nb_right[at]) out[k++] = at;
    if (start >= n || k != n) fail(SCANRS_ERR_NUMERICAL, "the leaf order visits %llu of %llu leaves", (unsigned long long)k, (unsigned long long)n);
}

// merge_clusters_below_distance_threshold (:210-227) + relabel_vector (:122-125)
void merge_below(const scanrs_hclust &h, double threshold, uint32_t *labels) {
    const uint64_t n = h.n;
    std::vector<uint32_t> parent(n), to_old(n - 1, NONE);
    for (uint64_t i = 0; i < n; i++) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t i) {
        while (parent[i] != i) {
            parent[i] = parent[parent[i]];
            i = parent[i];
        }
        return i;
    };
    auto old = [&](uint32_t c) -> uint32_t {
        if (c < n) return c;
        if (to_old[c - n] == NONE) // a step below the threshold over one that is not: the steps are not sorted (the reference panics)
            fail(SCANRS_ERR_ARGUMENT, "cluster %u is merged below the threshold but was made above it", c);
        return to_old[c - n];
    };
    for (uint64_t i = 0; i + 1 < n; i++) {
        if (!(h.diss[i] < threshold)) continue;
        const uint32_t a = find(old(h.c1[i])), b = find(old(h.c2[i]));
        if (a != b) parent[b] = a;
        to_old[i] = a;
    }
    std::vector<uint32_t> name(n, 0);
    uint32_t next = 1;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t r = find((uint32_t)i);
        if (!name[r]) name[r] = next++;
        labels[i] = name[r];
    }
}

} // namespace
} // namespace scanrs

using namespace scanrs;
extern "C" {
int scanrs_hclust_create(const double *x, uint64_t rows, uint64_t cols, uint64_t ld, int direction, int method, const scanrs_snoop *snoop,
                         scanrs_hclust **out) {
    return guard([&] { create_common(x, false, rows, cols, ld, direction, method, snoop, out); });
}
int scanrs_hclust_create_device(const double *d_x, uint64_t rows, uint64_t cols, uint64_t ld, int direction, int method, const scanrs_snoop *snoop,
                                scanrs_hclust **out) {
    return guard([&] { create_common(d_x, true, rows, cols, ld, direction, method, snoop, out); });
}
int scanrs_hclust_from_steps(uint64_t n, const uint32_t *c1, const uint32_t *c2, const double *diss, const uint32_t *size, scanrs_hclust **out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        check_n(n);
        if (!c1 || !c2 || !diss || !size) fail(SCANRS_ERR_ARGUMENT, "null argument");
        std::vector<uint8_t> used(2 * n - 1, 0);
        std::vector<uint64_t> sz(2 * n - 1, 1);
        for (uint64_t i = 0; i + 1 < n; i++) {
            const uint64_t a = c1[i], b = c2[i];
            if (a >= n + i || b >= n + i) fail(SCANRS_ERR_ARGUMENT, "step %llu merges a cluster that no earlier step has made", (unsigned long long)i);
            if (a == b || used[a] || used[b]) fail(SCANRS_ERR_ARGUMENT, "step %llu merges a cluster that has been merged already", (unsigned long long)i);
            used[a] = used[b] = 1;
            sz[n + i] = sz[a] + sz[b];
            if (size[i] != sz[n + i])
                fail(SCANRS_ERR_ARGUMENT, "step %llu: size %u, its clusters hold %llu observations", (unsigned long long)i, size[i], (unsigned long long)sz[n + i]);
            if (std::isnan(diss[i]) || (i > 0 && diss[i] < diss[i - 1]))
                fail(SCANRS_ERR_ARGUMENT, "step %llu: the dissimilarities must be sorted and not NaN", (unsigned long long)i);
        }
        // (n - 1 steps, two distinct clusters each, none twice: every cluster but the last has been merged exactly once)
        std::unique_ptr<scanrs_hclust> h(new scanrs_hclust());
        h->n = n;
        h->c1.assign(c1, c1 + n - 1);
        h->c2.assign(c2, c2 + n - 1);
        h->diss.assign(diss, diss + n - 1);
        h->size.assign(size, size + n - 1);
        h->info[6] = n - 1;
        *out = h.release();
    });
}
void scanrs_hclust_free(scanrs_hclust *h) { delete h; }
int scanrs_hclust_n(const scanrs_hclust *h, uint64_t *n) {
    return guard([&] {
        need_handle(h);
        if (!n) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *n = h->n;
    });
}
int scanrs_hclust_steps(const scanrs_hclust *h, uint32_t *c1, uint32_t *c2, double *diss, uint32_t *size) {
    return guard([&] {
        need_handle(h);
        if (c1) std::copy(h->c1.begin(), h->c1.end(), c1);
        if (c2) std::copy(h->c2.begin(), h->c2.end(), c2);
        if (diss) std::copy(h->diss.begin(), h->diss.end(), diss);
        if (size) std::copy(h->size.begin(), h->size.end(), size);
    });
}
int scanrs_hclust_leaves(const scanrs_hclust *h, int ordering, uint32_t *out) {
    return guard([&] {
        need_handle(h);
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (ordering != SCANRS_LEAF_NAIVE && ordering != SCANRS_LEAF_MODULAR_SMALLEST) fail(SCANRS_ERR_ARGUMENT, "unknown leaf ordering %d", ordering);
        leaves(*h, ordering, out);
    });
}
int scanrs_hclust_merge_below(const scanrs_hclust *h, double threshold, uint32_t *labels) {
    return guard([&] {
        need_handle(h);
        if (!labels) fail(SCANRS_ERR_ARGUMENT, "null argument");
        merge_below(*h, threshold, labels);
    });
}
int scanrs_hclust_fcluster(const scanrs_hclust *h, uint64_t num_clusters, uint32_t *labels) {
    return guard([&] {
        need_handle(h);
        if (!labels) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (num_clusters <= 1) {
            std::fill(labels, labels + h->n, 1u);
            return;
        }
        // steps[n.saturating_sub(k)]: k = 1 would index past the end, but never gets here
        const uint64_t at = h->n > num_clusters ? h->n - num_clusters : 0;
        merge_below(*h, h->diss[at], labels);
    });
}
int scanrs_hclust_info(const scanrs_hclust *h, uint64_t *out, uint32_t n_out) {
    return guard([&] {
        need_handle(h);
        if (!out && n_out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        for (uint32_t i = 0; i < n_out; i++) out[i] = i < 7 ? h->info[i] : 0;
    });
}
int scanrs_host_hclust_linkage(const double *x, uint64_t n, uint32_t d, int method, uint32_t *c1, uint32_t *c2, double *diss, uint32_t *size) {
    return guard([&] {
        check_method(method);
        check_n(n);
        if ((!x && d) || !c1 || !c2 || !diss || !size) fail(SCANRS_ERR_ARGUMENT, "null argument");
        scanrs_hclust h;
        twin_linkage(x, n, d, method, h);
        std::copy(h.c1.begin(), h.c1.end(), c1);
        std::copy(h.c2.begin(), h.c2.end(), c2);
        std::copy(h.diss.begin(), h.diss.end(), diss);
        std::copy(h.size.begin(), h.size.end(), size);
    });
}
int scanrs_debug_hclust_pdist(const double *x, uint64_t n, uint32_t d, uint64_t ld, int squared, double *out_condensed) {
    return guard([&] {
        if (n > 8192) fail(SCANRS_ERR_ARGUMENT, "a test entry point: at most 8192 observations");
        if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
        if (n < 2) return;
        if ((!x && d) || !out_condensed) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        CurrentHandle cur(nullptr);
        const hipStream_t s = nullptr;
        const uint64_t count = (n - 1) * ld + d;
        DevBuf<double> d_x(std::max<uint64_t>(1, count)), d_dist(n * n), d_obs;
        DevBuf<unsigned long long> d_bad;
        if (count) {
            SCANRS_HIP(hipMemcpyAsync(d_x.p, x, count * 8, hipMemcpyHostToDevice, s));
            SCANRS_SYNC(s);
        }
        queue_pdist(s, d_x.p, n, d, ld, 0, squared, d_obs, d_bad, d_dist.p);
        refuse_not_finite(SCANRS_D2H_VALUE(d_bad.p, s), std::max<uint32_t>(1, d));
        std::vector<double> full(n * n);
        SCANRS_D2H(full.data(), d_dist.p, n * n * 8, s);
        uint64_t k = 0;
        for (uint64_t i = 0; i < n; i++)
            for (uint64_t j = i + 1; j < n; j++) out_condensed[k++] = full[i * n + j];
    });
}
} // extern "C"
