// knn_metric.hip — nearest_neighbors(data, k, distance_type) of umap-rs (umap-rs/src/knn.rs:112-166, dist.rs:12-35, 69-124): the
// indices AND the distances of the k nearest other rows under Euclidean, Pearson or cosine distance. DESIGN.md §7q.
//
// Pearson / cosine. The reference ranks by key = sqrt(D(x, y)) with D = max(1 - s_xy / sqrt(s_xx s_yy), 0) (two special cases first,
// knn_metric.hpp) and returns key * key. Every fold is serial f64 and unfused, so the value of a pair is reproducible bit for bit;
// this file is compiled with -ffp-contract=off. mu, c = x - mu and s_xx depend on one row only and are formed once per row
// (km_prep_kernel) with the bits the reference gets; only s_xy is per pair. Ties, including the ones sqrt creates, come in ascending
// index order (the rule of scanrs_knn; the vp-tree's order among equal keys is a property of that crate). The search itself is the
// one of knn_search.hpp under the policy Metric below, instantiated here under this file's flags. Its two routes:
//  * knn_exhaustive_kernel: one thread per query with its prepared row in registers, the candidate row wave-uniform, a sorted k-list
//    per thread. Answers every shape.
//  * the filtered route (knn_filtered): 1 - rho is half the squared Euclidean distance between the standardised rows z = c / |c|, so
//    the bf16-MFMA filter of knn.hip (kf_prepare / kf_filter_pass, knn_filter.hpp) runs on z with a threshold converted from the
//    query's k-th key, and knn_rerank_kernel ranks what passes by the reference formula on c / s_xx - never on z.
// Euclidean. The reference calls simd_euclidean::Vectorized::distance, whose summation order is not in the reference tree: this kind
// is the library's own search (knn_device_into: ordered by the fma-chain squared distance, then index) followed by one square root.
//
// Two row sets. Every kernel takes the queries and the points apart (KnnRows: C, s_xx and Z of each side), with the global rows q_off
// and p_off of their first rows: a pair is the query's own row when p_off + prow == q_off + qrow. nearest_neighbors is the case where the
// two are one array; nearest_neighbors_query has a query set of its own; nearest_neighbors_sharded (the walk of
// knn_shard.hpp) searches the rank's rows against one block of the global point set at a time. prepare_row depends on one row only,
// so every rank forms the same bits from the same raw row, and only raw rows cross the shards. The searches leave KEYS (sqrt(D));
// the running list of a sharded search is (key, global index), merged by the rule of knn_merge.hpp, and one last kernel writes
// key * key (metric2dist).
// The seed of a block is the query's k-th key so far (+inf while it holds fewer than k), and it is strict: the exhaustive kernel
// drops a candidate unless key < seed. Blocks arrive in ascending global index, so a later block's candidate whose key EQUALS the
// query's current k-th key has a larger global index than every entry it would displace, and loses the tie: key < seed drops only
// losers. The filter's threshold takes min(seed, own k-th key) where the bound below has key_k; the rerank kernel drops nothing
// because of the seed, the merge does.
//
// The threshold. The filter's contract (knn.hip): every point whose COMPUTED fma-chain squared distance to the query's z row is
// <= tau passes. Write u = 2^-53, c_q and c_p for the prepared rows as stored (they are the inputs of everything below), rho* =
// c_q.c_p / (|c_q| |c_p|) exactly and zh = c / |c| exactly, so |zh_q - zh_p|^2 = 2 (1 - rho*). gamma_m = m u / (1 - m u).
//  1. The folds. Computed s_xy = c_q.c_p + e, |e| <= gamma_d sum |c_qj c_pj| <= gamma_d |c_q| |c_p| (d products, d - 1 effective
//     additions, Cauchy-Schwarz); computed s_xx = |c_q|^2 (1 + t_q), |t_q| <= gamma_d, s_yy likewise.
//  2. The denominator. fl(sqrt(fl(s_xx s_yy))) = |c_q| |c_p| (1 + eta), 1 + eta = sqrt((1 + t_q)(1 + t_p)(1 + e1)) (1 + e2), |e_i| <= u:
//     |eta| <= gamma_d + 2 u =: (d + 2) u up to second order.
//  3. The quotient r = fl(s_xy / denominator) = (rho* + e') (1 + e3) / (1 + eta), |e'| <= gamma_d, |rho*| <= 1:
//     |r - rho*| <= gamma_d + (1 + gamma_d)(|eta| + u + ...) <= (2 d + 5) u =: a    (d <= 58: a <= 121 u).
//  4. D = max(fl(1 - r), 0). fl(1 - r) = (1 - r)(1 + e4), so 1 - r <= D (1 + 2 u) whether or not the maximum cut in (it cuts in only
//     when 1 - r <= 0), and 1 - rho* <= D (1 + 2 u) + a. The two special cases never occur on the filtered route (no degenerate row;
//     s_xy == 0 gives D = 1 where the formula would give 1 - 0 = 1).
//  5. The key. key = fl(sqrt(D)) = sqrt(D)(1 + e5). A point belongs to the query's answer only if key_p <= key_k (ties included: a
//     smaller index wins), i.e. D_p <= key_k^2 (1 + u)^2, and the kernel forms kk = fl(key_k key_k) >= key_k^2 (1 - u):
//     D_p <= kk (1 + 4 u).  Hence 2 (1 - rho*) <= 2 kk (1 + 7 u) + 2 a.
//  6. The z rows. fl(sqrt(s_xx)) = |c| (1 + eta1), |eta1| <= gamma_d / 2 + u; z_j = fl(c_j / that) = zh_j (1 + zeta_j),
//     |zeta_j| <= (d / 2 + 3) u =: b (d <= 58: b <= 32 u). So |z_q - z_p| <= |zh_q - zh_p| + b (|zh_q| + |zh_p|) = Delta + 2 b with
//     Delta <= 2, and the EXACT |z_q - z_p|^2 <= Delta^2 + 8 b + 4 b^2.
//  7. The filter's own chain over z: differences (1 + u), squares, an fma chain of at most 58 terms: computed <= exact (1 + (d + 3) u)
//     <= exact + 4.1 * 61 u; KM_CHAIN = 2^-44 = 512 u is that allowance.
//  Sum: computed chain <= 2 kk (1 + (d + 11) u) + [2 a + 8 b + 4 b^2] (1 + 61 u) + 251 u <= 2 kk (1 + 69 u) + 750 u.
//  KM_DELTA = KM_E = 2^-40 = 8192 u cover that ten times over and cost nothing against the filter's margin gamma S = 0.0079 (S = 2).
//  All of it is relative error analysis and holds while nothing overflows or goes subnormal: hence the window KM_SXX_MIN <= s_xx <=
//  KM_SXX_MAX over all rows. Inside it s_xx s_yy, its root and the quotients are normal; single products c_qj c_pj or coordinates z_j
//  may still underflow, each by at most 2^-1074 absolutely against |c_q| |c_p| >= 2^-400 (or |z| = 1): below 2^-600 in all, which KM_E
//  swallows. A degenerate row (s_xx == 0, D 1 or 0 by rule and not by geometry) lies outside the window, so does an overflowed s_xx:
//  then the filter declines and the exhaustive kernel answers. z itself always lies inside the filter's own window (max |z_j| >=
//  1 / sqrt(d)). tests/test_metric_knn_cpu.py checks the bound in exact rational arithmetic on adversarial rows.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "knn_filter.hpp"
#include "knn_metric.hpp"
#include "knn_search.hpp"
#include "knn_shard.hpp"

namespace scanrs {

using namespace knn_metric;

namespace {

// One pass over the rows, a row per thread: C (n x dmax, zero-padded behind column d) = the centred row (pearson) or the row
// (cosine), sxx[r], Z (n x d, or null) = the standardised row for the filter. info[0] = degenerate rows (s_xx == 0),
// info[1] / info[2] = min / max of s_xx as bit patterns (for non-negative doubles the unsigned order of the bits is the numerical
// order; +inf and NaN sort above every finite value).
// Zero padding does not change a bit of any fold over the padded row: acc + 0 * 0 leaves acc as it is, and acc is never -0.0 (the
// fold starts from +0.0, and +0.0 + (-0.0) = +0.0), so no sign of zero can flip either.
__global__ __launch_bounds__(256) void km_prep_kernel(int kind, const double *__restrict__ X, uint32_t ld, uint64_t n, uint32_t d, uint32_t dmax,
                                                      double *__restrict__ C, double *__restrict__ sxx, double *__restrict__ Z,
                                                      unsigned long long *__restrict__ info) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long lo = ~0ull, hi = 0ull, deg = 0ull;
    if (r < n) {
        double *c = C + r * dmax;
        const double s = prepare_row(kind, X + r * ld, d, c, Z ? Z + r * d : nullptr);
        for (uint32_t j = d; j < dmax; j++) c[j] = 0.0;
        sxx[r] = s;
        lo = hi = (unsigned long long)__double_as_longlong(s);
        deg = s == 0.0 ? 1ull : 0ull;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = min(lo, (unsigned long long)__shfl_xor((long long)lo, off, 64));
        hi = max(hi, (unsigned long long)__shfl_xor((long long)hi, off, 64));
        deg += (unsigned long long)__shfl_xor((long long)deg, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (deg) atomicAdd(&info[0], deg);
        atomicMin(&info[1], lo);
        atomicMax(&info[2], hi);
    }
}

// The policy of the search (knn_search.hpp): the unfused dot product s_xy over the padded rows, key = sqrt(D) with the per-row scalars
// s_xx and s_yy (pair_value, knn_metric.hpp), and the threshold derived at the top of this file. Compiled with -ffp-contract=off.
struct Metric {
    static __device__ __forceinline__ double step(double acc, double q, double p) { return acc + q * p; }
    static __device__ __forceinline__ double finish(double acc, double s_xx, double s_yy) { return sqrt(pair_value(s_xx, s_yy, acc)); }
    static __device__ __forceinline__ double threshold(double key) {
        const double kk = key * key;
        return 2.0 * kk * (1.0 + KM_DELTA) + KM_E;
    }
};

__global__ void km_sqrt_kernel(double *__restrict__ x, uint64_t n) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) x[e] = sqrt(x[e]);
}
// metric2dist (dist.rs:24, 32): the key of every entry -> its distance; +inf padding stays +inf
__global__ void km_square_kernel(double *__restrict__ x, uint64_t n) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) x[e] = x[e] * x[e];
}
void km_square(hipStream_t s, double *x, uint64_t n) {
    if (n) hipLaunchKernelGGL(km_square_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n);
}
void km_sqrt(hipStream_t s, double *x, uint64_t n) {
    if (n) hipLaunchKernelGGL(km_sqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n);
}

// the prepared rows of one side and the memory they live in (kept across the blocks of a sharded search)
struct KmPrepared {
    DevBuf<double> C, sxx, Z;
    DevBuf<unsigned long long> info;
    KnnRows rows; // C (n x knn_dmax(d)) and sxx for the exact kernels, Z for the filter
};
// with_z: the standardised rows are made only where the filter can take the shape; then this waits for the window test, and the side
// may take the filter when it has no degenerate row and every s_xx lies inside [KM_SXX_MIN, KM_SXX_MAX]
void km_prepare(hipStream_t s, int kind, const double *X, uint32_t ld, uint64_t n, uint32_t d, bool with_z, KmPrepared &r) {
    const uint32_t dmax = knn_dmax(d);
    if (r.C.n < n * dmax) r.C.alloc(n * dmax);
    if (r.sxx.n < n) r.sxx.alloc(n);
    if (with_z && r.Z.n < n * d) r.Z.alloc(n * d);
    if (!r.info.p) r.info.alloc(3);
    const unsigned long long init[3] = {0ull, ~0ull, 0ull};
    kf_h2d(s, r.info.p, init, 24);
    hipLaunchKernelGGL(km_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kind, X, ld, n, d, dmax, r.C.p, r.sxx.p,
                       with_z ? r.Z.p : nullptr, r.info.p);
    SCANRS_HIP(hipGetLastError());
    r.rows = KnnRows{r.C.p, dmax, r.sxx.p, with_z ? r.Z.p : nullptr, d, n, false};
    if (with_z) {
        unsigned long long h[3];
        kf_d2h(s, h, r.info.p, 24);
        double lo, hi;
        memcpy(&lo, &h[1], 8);
        memcpy(&hi, &h[2], 8);
        r.rows.may_filter = h[0] == 0 && lo >= KM_SXX_MIN && hi <= KM_SXX_MAX; // (false for NaN)
    }
}

// true: the filter answered. (This search has never sent more queries through the filter than 32-bit offsets into the candidate lists
// would address; the exhaustive kernel answers those.)
bool km_search(hipStream_t s, KnnRows Q, const KnnRows &P, uint32_t d, uint32_t k, const KnnPlace &pl, uint32_t *dout, double *dkey,
               KnnLastStats &stats) {
    Q.may_filter = Q.may_filter && Q.n <= 0xFFFFFFFFull / KF_CAP;
    return knn_search<Metric>(s, "nearest_neighbors", Q, P, d, k, pl, dout, dkey, stats);
}

void km_refuse_not_finite(hipStream_t s, const double *X, uint32_t ld, uint64_t n, uint32_t d, const char *what) {
    if (!n) return;
    DevBuf<unsigned long long> first(1);
    SCANRS_HIP(hipMemsetAsync(first.p, 0xFF, 8, s));
    hipLaunchKernelGGL(ks_scan_kernel, dim3((unsigned)std::min<uint64_t>((n * d + 255) / 256, 2048)), dim3(256), 0, s, X, ld, n, d, first.p);
    const unsigned long long bad = SCANRS_D2H_VALUE(first.p, s);
    if (bad != ~0ull) fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: row %llu of the %s holds a coordinate that is not finite", bad, what);
}

// n_q queries against n_p >= 1 points in device memory (one array where the pointers, leading dimensions and counts coincide);
// dout / ddist: the lists in device memory, n_q x k
void km_two_sets_resident(const double *dq, uint64_t n_q, uint32_t ld_q, const double *dp, uint64_t n_p, uint32_t ld_p, uint32_t d, uint32_t k,
                          int kind, bool skip, DevBuf<uint32_t> &dout, DevBuf<double> &ddist) {
    hipStream_t s = 0;
    dout.alloc(n_q * k);
    ddist.alloc(n_q * k);
    if (kind == EUCLIDEAN) {
        knn_device_into(dq, ld_q, n_q, dp, ld_p, n_p, d, k, skip, dout.p, ddist.p);
        km_sqrt(s, ddist.p, n_q * k); // +inf padding stays +inf
    } else {
        const GlobalOptions &go = global_options();
        const bool same = dq == dp && ld_q == ld_p && n_q == n_p;
        const bool may_filter = !go.knn_exhaustive && d <= KF_DMAX && k <= KF_KMAX && n_q >= KF_NQ_MIN && n_p >= go.knn_filter_min_points;
        KmPrepared P, Qown;
        km_prepare(s, kind, dp, ld_p, n_p, d, may_filter, P);
        if (!same) km_prepare(s, kind, dq, ld_q, n_q, d, may_filter, Qown);
        KnnPlace pl;
        pl.skip = skip ? 1 : 0;
        KnnLastStats stats;
        km_search(s, same ? P.rows : Qown.rows, P.rows, d, k, pl, dout.p, ddist.p, stats);
        km_square(s, ddist.p, n_q * k);
        knn_publish_stats(std::move(stats));
        SCANRS_SYNC(s); // the prepared rows are released on leaving this block
    }
    SCANRS_HIP(hipGetLastError());
}
// indices / distances: host arrays, n_q x k
void km_two_sets(const double *dq, uint64_t n_q, uint32_t ld_q, const double *dp, uint64_t n_p, uint32_t ld_p, uint32_t d, uint32_t k, int kind,
                 bool skip, uint32_t *indices, double *distances) {
    DevBuf<uint32_t> dout;
    DevBuf<double> ddist;
    km_two_sets_resident(dq, n_q, ld_q, dp, n_p, ld_p, d, k, kind, skip, dout, ddist);
    SCANRS_HIP(hipMemcpy(indices, dout.p, n_q * k * 4, hipMemcpyDeviceToHost));
    SCANRS_HIP(hipMemcpy(distances, ddist.p, n_q * k * 8, hipMemcpyDeviceToHost));
}

} // namespace

void nearest_neighbors_device(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, uint32_t *indices,
                              double *distances) {
    nearest_neighbors_check_args(n, ld, d, k, kind);
    if (k == 0 || n == 0) return;
    km_refuse_not_finite(0, d_data, ld, n, d, "data");
    if (n < 2) { // no other row: padding only
        for (uint32_t i = 0; i < k; i++) indices[i] = 0xFFFFFFFFu, distances[i] = INFINITY;
        return;
    }
    km_two_sets(d_data, n, ld, d_data, n, ld, d, k, kind, true, indices, distances);
}

// umap_graph (fuzzy_host.cpp): the same search with the lists left where the graph stage reads them; 1 <= k <= n - 1, so no padding
void nearest_neighbors_resident(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, DevBuf<uint32_t> &idx,
                                DevBuf<double> &dist) {
    nearest_neighbors_check_args(n, ld, d, k, kind);
    km_refuse_not_finite(0, d_data, ld, n, d, "data");
    km_two_sets_resident(d_data, n, ld, d_data, n, ld, d, k, kind, true, idx, dist);
}

void nearest_neighbors_query_device(const double *d_queries, uint64_t n_q, uint32_t ld_q, const double *d_points, uint64_t n_p, uint32_t ld_p,
                                    uint32_t d, uint32_t k, int kind, bool include_self, uint32_t *indices, double *distances) {
    nearest_neighbors_check_args(n_p, ld_p, d, k, kind);
    nearest_neighbors_check_args(n_q, ld_q, d, k, kind);
    if (k == 0 || n_q == 0) return;
    km_refuse_not_finite(0, d_queries, ld_q, n_q, d, "queries");
    km_refuse_not_finite(0, d_points, ld_p, n_p, d, "points");
    if (n_p == 0) { // no point: padding only
        for (uint64_t i = 0; i < n_q * k; i++) indices[i] = 0xFFFFFFFFu, distances[i] = INFINITY;
        return;
    }
    km_two_sets(d_queries, n_q, ld_q, d_points, n_p, ld_p, d, k, kind, !include_self, indices, distances);
}

// The search over a sharded point set: the walk of knn_shard.hpp with this file's search of one block. The rank's own rows are
// prepared once, every block once as it arrives; the route of a block (filter or exhaustive) never changes a bit of its list, so the
// ranks need not agree on it.
void nearest_neighbors_sharded(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d,
                               uint32_t k, int kind, uint32_t *out, double *distances) {
    KnnBlockSearch bs;
    bs.name = "nearest_neighbors_sharded";
    bs.check = "nearest_neighbors";
    bs.kind = kind;
    if (kind == EUCLIDEAN) { // knn_sharded with its squared distances, then the square root
        bs.finish = km_sqrt;
        knn_sharded_euclidean(st, d_pts, ld, begin, n_local, n, d, k, bs, out, distances);
        return;
    }
    const GlobalOptions &go = global_options();
    const uint64_t largest = std::min<uint64_t>(std::max<uint64_t>(1, go.knn_block_rows), n);
    KmPrepared Q, P;
    KfQueries qs;
    bool ready = false, may_filter = false;
    // (called after the first exchange has checked the arguments)
    bs.search = [&](hipStream_t s, const double *blk, uint64_t rows, uint64_t b0, const double *seed, uint32_t *bidx, double *bkey,
                    KnnLastStats &stats) {
        if (!ready) {
            may_filter = !go.knn_exhaustive && d <= KF_DMAX && k <= KF_KMAX && n_local >= KF_NQ_MIN && largest >= go.knn_filter_min_points;
            km_prepare(s, kind, d_pts, ld, n_local, d, may_filter, Q);
            may_filter = Q.rows.may_filter;
            if (may_filter) kf_prepare_queries(s, Q.rows.F, d, n_local, d, qs);
            ready = true;
        }
        km_prepare(s, kind, blk, d, rows, d, may_filter, P);
        KnnPlace pl;
        pl.p_off = b0;
        pl.q_off = begin;
        pl.seed = seed;
        pl.seed_ld = k;
        pl.queries = may_filter ? &qs : nullptr;
        if (km_search(s, Q.rows, P.rows, d, k, pl, bidx, bkey, stats)) st.knn_blocks_filtered++;
    };
    bs.finish = km_square;
    knn_sharded_blocks(st, d_pts, ld, begin, n_local, n, d, k, bs, out, distances);
}


// scanrs_init(): one empty launch per translation unit makes the runtime load this file's code object now instead of inside the
// first real call
__global__ void warm_knn_metric_kernel() {}
void warm_knn_metric(hipStream_t s) { hipLaunchKernelGGL(warm_knn_metric_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
