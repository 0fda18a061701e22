// knn_metric.hip — nearest_neighbors(data, k, distance_type) of umap-rs (umap-rs/src/knn.rs:112-166, dist.rs:12-35, 69-124): the
// indices AND the distances of the k nearest other rows under Euclidean, Pearson or cosine distance. DESIGN.md §7q.
//
// Pearson / cosine. The reference ranks by key = sqrt(D(x, y)) with D = max(1 - s_xy / sqrt(s_xx s_yy), 0) (two special cases first,
// knn_metric.hpp) and returns key * key. Every fold is serial f64 and unfused, so the value of a pair is reproducible bit for bit;
// this file is compiled with -ffp-contract=off. mu, c = x - mu and s_xx depend on one row only and are formed once per row
// (km_prep_kernel) with the bits the reference gets; only s_xy is per pair. Ties, including the ones sqrt creates, come in ascending
// index order (the rule of scanrs_knn; the vp-tree's order among equal keys is a property of that crate). Two routes:
//  * km_exhaustive_kernel: the shape of knn_kernel (knn.hip) - one thread per query with its prepared row in registers, the candidate
//    row wave-uniform, a sorted k-list per thread. Answers every shape.
//  * the filtered route (km_filtered): 1 - rho is half the squared Euclidean distance between the standardised rows z = c / |c|, so
//    the bf16-MFMA filter of knn.hip (kf_prepare / kf_filter_pass, knn_filter.hpp) runs on z with a threshold converted from the
//    query's k-th key, and km_rerank_kernel ranks what passes by the reference formula on c / s_xx - never on z.
// Euclidean. The reference calls simd_euclidean::Vectorized::distance, whose summation order is not in the reference tree: this kind
// is the library's own search (knn_device_into: ordered by the fma-chain squared distance, then index) followed by one square root.
//
// Two row sets. Every kernel takes the queries (Cq, sxx_q, Zq) and the points (Cp, sxx_p, Zp) apart, with the global rows q_off and
// p_off of their first rows: a pair is the query's own row when p_off + prow == q_off + qrow. nearest_neighbors is the case where the
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
#include "knn_shard.hpp"

namespace scanrs {

using namespace knn_metric;

namespace {

// the first row that holds a coordinate which is not finite (an integer minimum; ~0 stays when there is none)
__global__ __launch_bounds__(256) void km_scan_kernel(const double *__restrict__ X, uint32_t ld, uint64_t n, uint32_t d,
                                                      unsigned long long *__restrict__ first) {
    const uint64_t total = n * d, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const uint64_t r = e / d;
        const double x = X[r * ld + (e % d)];
        if (!(fabs(x) <= DBL_MAX)) atomicMin(first, (unsigned long long)r);
    }
}

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

// The prepared rows of one side of a search (km_prep_kernel): C n x dmax, sxx n, Z n x d or null. The two sides of nearest_neighbors
// are one of these.
struct KmRows {
    const double *C = nullptr, *sxx = nullptr, *Z = nullptr;
    uint64_t n = 0;
    bool in_window = false; // no degenerate row and every s_xx inside [KM_SXX_MIN, KM_SXX_MAX]; known only where Z was made
};
// Where a search stands in a larger one (all defaults: the points are the whole set and the queries its rows, as in nearest_neighbors).
struct KmPlace {
    uint64_t p_off = 0, q_off = 0; // the global rows of point row 0 and of query 0
    int skip = 1;                  // drop the pair whose global rows coincide (query.idx != idx, knn.rs:155)
    const double *seed = nullptr;  // per query the k-th key it already holds (element q * seed_ld; +inf: none), see the top of this file
    uint64_t seed_ld = 0;
    const KfQueries *queries = nullptr; // the query side of the filter, prepared once for all blocks
};

// Exhaustive route. Query t is row qrows[t] (or t) of Cq; the candidates are rows 0, p_stride, 2 p_stride, ... of Cp (n_sub of them),
// each wave-uniform. The inner loop is the unfused dot product s_xy over the padded row, then D and key = sqrt(D) (knn_metric.hpp).
// Writes, at the query's own row: the indices (rows of Cp), the keys, and kth = the k-th key (+inf while fewer than k exist).
template <int DMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void km_exhaustive_kernel(const double *__restrict__ Cq, const double *__restrict__ sxx_q,
                                                                const double *__restrict__ Cp, const double *__restrict__ sxx_p,
                                                                const uint32_t *__restrict__ qrows, uint64_t n_q, uint64_t n_sub,
                                                                uint64_t p_stride, uint64_t p_off, uint64_t q_off, int skip,
                                                                const double *__restrict__ seed, uint64_t seed_ld, uint32_t k,
                                                                uint32_t *__restrict__ out, double *__restrict__ out_key, double *__restrict__ kth) {
    const uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool live = t < n_q;
    const uint64_t qrow = live ? (qrows ? (uint64_t)qrows[t] : t) : 0;
    double q[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; j++) q[j] = live ? Cq[qrow * DMAX + j] : 0.0;
    const double s_q = live ? sxx_q[qrow] : 0.0;
    // the point row that is the query itself; no row when nothing is skipped (p_off + prow == q_off + qrow, without a wrap)
    const uint64_t self = skip ? q_off + qrow - p_off : ~0ull;
    double best_d[KMAX];
    uint32_t best_i[KMAX];
    uint32_t have = 0;
    // the key a candidate has to beat: the seed, then the list's own k-th key once it is full (never above the seed, since every
    // entry beat it). +inf means "no bound yet": a key of +inf is a legitimate one (a quotient by an underflowed s_xx s_yy) and still
    // enters a list that is not full
    double worst = (live && seed) ? seed[qrow * seed_ld] : INFINITY;
    for (uint64_t pi = 0; pi < n_sub; pi++) {
        const uint64_t prow = pi * p_stride;
        const double *__restrict__ pt = Cp + prow * DMAX;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < DMAX; j++) s = s + q[j] * pt[j];
        if (!live || prow == self) continue; // query.idx != idx, knn.rs:155
        const double key = sqrt(pair_value(s_q, sxx_p[prow], s));
        if ((have == k || worst != INFINITY) && !(key < worst)) continue;
        // sorted insertion; equal keys stay in index order because candidates arrive in index order
        uint32_t pos = have < k ? have : k - 1u;
        while (pos > 0 && best_d[pos - 1] > key) {
            best_d[pos] = best_d[pos - 1];
            best_i[pos] = best_i[pos - 1];
            pos--;
        }
        best_d[pos] = key;
        best_i[pos] = (uint32_t)prow;
        if (have < k) have++;
        if (have == k) worst = best_d[k - 1];
    }
    if (!live) return;
    for (uint32_t i = 0; i < k; i++) {
        out[qrow * k + i] = i < have ? best_i[i] : 0xFFFFFFFFu; // the reference's initial fill, knn.rs:139-140
        out_key[qrow * k + i] = i < have ? best_d[i] : INFINITY;
    }
    if (kth) kth[qrow] = have == k ? best_d[k - 1] : INFINITY;
}

// one exhaustive search: n_q queries (rows qrows[t] of Q, or its first n_q rows) against rows 0, p_stride, ... of P (n_sub of them)
struct KmExhaustive {
    KmRows Q, P;
    KmPlace pl;
    const uint32_t *qrows;
    uint64_t n_q, n_sub, p_stride;
    uint32_t k;
    uint32_t *out;
    double *out_key, *kth;
};
template <int DMAX, int THREADS>
void km_launch(hipStream_t s, const KmExhaustive &e) {
    hipLaunchKernelGGL((km_exhaustive_kernel<DMAX, THREADS>), dim3((unsigned)((e.n_q + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, e.Q.C, e.Q.sxx,
                       e.P.C, e.P.sxx, e.qrows, e.n_q, e.n_sub, e.p_stride, e.pl.p_off, e.pl.q_off, e.pl.skip, e.pl.seed, e.pl.seed_ld, e.k, e.out,
                       e.out_key, e.kth);
}
// the instances of knn.hip's exhaustive(): the padded width of a row for d coordinates
uint32_t km_dmax(uint32_t d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 52 ? 52 : d <= 64 ? 64 : 128; }
void km_exhaustive(hipStream_t s, uint32_t dmax, const KmExhaustive &e) {
    if (e.n_q == 0) return;
    switch (dmax) {
    case 8: km_launch<8, 256>(s, e); break;
    case 16: km_launch<16, 256>(s, e); break;
    case 32: km_launch<32, 256>(s, e); break;
    case 52: km_launch<52, 256>(s, e); break;
    case 64: km_launch<64, 256>(s, e); break;
    default: km_launch<128, 64>(s, e); break;
    }
    SCANRS_HIP(hipGetLastError());
}

// The rerank of the filtered route: kf_rerank_kernel's shape (one wave per query, a candidate per lane, k rounds of a wave-wide
// lexicographic minimum), with the reference formula on C / sxx as the value of a pair and (key, index) as the order. Query q is row
// q of Cq, a candidate a row of Cp; the pair whose global rows coincide is dropped when skip is set. Writes the indices (rows of Cp),
// the keys and the query's k-th key (+inf while fewer than k exist). Overflowed lists (cnt > KF_CAP) are left alone.
__global__ __launch_bounds__(256) void km_rerank_kernel(const double *__restrict__ Cq, const double *__restrict__ sxx_q,
                                                        const double *__restrict__ Cp, const double *__restrict__ sxx_p, uint32_t ldc, uint64_t n_q,
                                                        uint32_t d, uint32_t k, uint64_t p_off, uint64_t q_off, int skip,
                                                        const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cnt,
                                                        uint32_t *__restrict__ out, double *__restrict__ out_key, double *__restrict__ kth_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= n_q) return;
    const uint32_t c = cnt[q];
    if (c > KF_CAP) return; // the host reads cnt and redoes this query exhaustively
    double key[KF_PER_LANE];
    uint32_t idx[KF_PER_LANE];
    const double *__restrict__ qr = Cq + q * ldc;
    const double s_q = sxx_q[q];
    const uint64_t self = skip ? q_off + q - p_off : ~0ull; // the point row that is the query itself, if any
#pragma unroll
    for (uint32_t u = 0; u < KF_PER_LANE; u++) {
        const uint32_t j = u * 64u + lane;
        key[u] = INFINITY;
        idx[u] = 0xFFFFFFFFu;
        if (j < c) {
            const uint32_t p = cand[q * KF_CAP + j];
            if ((uint64_t)p != self) {
                const double *__restrict__ pr = Cp + (uint64_t)p * ldc;
                double s = 0.0;
                for (uint32_t t = 0; t < d; t++) s = s + qr[t] * pr[t];
                key[u] = sqrt(pair_value(s_q, sxx_p[p], s));
                idx[u] = p;
            }
        }
    }
    double kth = INFINITY;
    bool full = true;
    for (uint32_t it = 0; it < k; it++) {
        // lane-local minimum, then the wave's; an empty slot (index UINT32_MAX) loses against every candidate, whatever its key
        double bd = INFINITY;
        uint32_t bi = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t u = 0; u < KF_PER_LANE; u++)
            if (idx[u] != 0xFFFFFFFFu && (key[u] < bd || (key[u] == bd && idx[u] < bi))) {
                bd = key[u];
                bi = idx[u];
            }
        double wd = bd;
        uint32_t wi = bi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(wd, off, 64);
            const uint32_t oi = (uint32_t)__shfl_xor((int)wi, off, 64);
            if (oi != 0xFFFFFFFFu && (od < wd || (od == wd && oi < wi))) {
                wd = od;
                wi = oi;
            }
        }
        if (wi == 0xFFFFFFFFu) { // fewer than k candidates: the rest is padding
            for (uint32_t r2 = it; r2 < k; r2++)
                if (lane == 0) {
                    out[q * k + r2] = 0xFFFFFFFFu;
                    out_key[q * k + r2] = INFINITY;
                }
            full = false;
            break;
        }
        if (lane == 0) {
            out[q * k + it] = wi;
            out_key[q * k + it] = wd;
        }
        kth = wd;
        // the owner retires that entry (indices are unique within a list: a point is appended once per round)
#pragma unroll
        for (uint32_t u = 0; u < KF_PER_LANE; u++)
            if (idx[u] == wi) {
                key[u] = INFINITY;
                idx[u] = 0xFFFFFFFFu;
            }
    }
    if (lane == 0) kth_out[q] = full ? kth : INFINITY;
}

// the k-th key of a query -> the filter's threshold in z-space (the derivation at the top of this file); +inf: everything passes
// (of a seeded search: the smaller of that key and the seed - a point at or beyond the seed is no part of the answer either)
__global__ void km_tau_kernel(const double *__restrict__ kth, const double *__restrict__ seed, uint64_t seed_ld, uint64_t n,
                              double *__restrict__ tau) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const double key = seed ? fmin(kth[q], seed[q * seed_ld]) : kth[q];
    const double kk = key * key;
    tau[q] = 2.0 * kk * (1.0 + KM_DELTA) + KM_E;
}

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

// The filtered route: knn_filtered's rounds (knn.hip) on the standardised rows Zq against Zp - nested strided subsets of the points,
// the coarsest ranked exactly, every further one through the filter with the threshold of the round before, overflowed lists redone
// exhaustively (seeded like everything else). false: the filter declines (a shape it does not take, a degenerate row or an s_xx
// outside the window on either side) and nothing has been written.
bool km_filtered(hipStream_t s, const KmRows &Q, const KmRows &P, uint32_t dmax, uint32_t d, uint32_t k, const KmPlace &pl, uint32_t *dout,
                 double *dkey, KnnLastStats &stats) {
    const GlobalOptions &go = global_options();
    const uint64_t n_q = Q.n, n_p = P.n;
    if (go.knn_exhaustive != 0 || d > KF_DMAX || n_p < go.knn_filter_min_points || k > KF_KMAX || n_q < KF_NQ_MIN) return false;
    if (!Q.in_window || !P.in_window || !Q.Z || !P.Z) return false;
    if (n_q > 0xFFFFFFFFull / KF_CAP) return false; // the candidate lists are addressed in 32 bits per query
    const uint64_t ratio = std::max<uint64_t>(2, go.knn_ratio);
    const uint64_t n0_max = pl.seed ? KF_SEED_N0 : KF_CAP;
    std::vector<uint64_t> strides;
    uint64_t st0 = 1;
    while ((n_p + st0 - 1) / st0 > n0_max) st0 *= 2;
    for (uint64_t st = st0; st > 1;) {
        st = st / ratio > 0 ? st / ratio : 1;
        strides.push_back(st);
    }
    if (strides.empty()) return false;
    KfOperands op;
    if (!kf_prepare(s, Q.Z, d, n_q, P.Z, d, n_p, d, op, pl.queries)) return false;
    stats.first_stride = st0;
    DevBuf<double> tau(n_q), kth(n_q);
    DevBuf<uint32_t> cnt(n_q), cand(n_q * KF_CAP);
    const dim3 g4((unsigned)((n_q + 3) / 4)), g256((unsigned)((n_q + 255) / 256)), b256(256);
    auto rerank = [&] {
        hipLaunchKernelGGL(km_rerank_kernel, g4, b256, 0, s, Q.C, Q.sxx, P.C, P.sxx, dmax, n_q, d, k, pl.p_off, pl.q_off, pl.skip, cand.p, cnt.p, dout,
                           dkey, kth.p);
    };
    { // round 0: exact ranking of the coarsest subset
        const uint32_t n0 = (uint32_t)((n_p + st0 - 1) / st0);
        hipLaunchKernelGGL(kf_fill_all_kernel, dim3((unsigned)((n_q * n0 + 255) / 256)), b256, 0, s, n_q, n0, st0, cand.p, cnt.p);
        rerank();
    }
    std::vector<uint32_t> h_cnt(n_q);
    for (uint64_t st : strides) {
        const uint64_t n_sub = (n_p + st - 1) / st;
        hipLaunchKernelGGL(km_tau_kernel, g256, b256, 0, s, kth.p, pl.seed, pl.seed_ld, n_q, tau.p);
        kf_filter_pass(s, op, tau.p, n_q, n_p, st, cand.p, cnt.p);
        rerank();
        SCANRS_HIP(hipGetLastError());
        kf_d2h(s, h_cnt.data(), cnt.p, n_q * 4);
        KfRound rd{st, n_sub, 0, 0, 0};
        std::vector<uint32_t> rows;
        for (uint64_t q = 0; q < n_q; q++) {
            const uint32_t c = h_cnt[q];
            rd.cand_sum += c; // an overflowed list counts with what its counter reached
            rd.cand_max = std::max(rd.cand_max, c);
            if (c > KF_CAP) rows.push_back((uint32_t)q);
        }
        rd.overflowed = (uint32_t)rows.size();
        stats.rounds.push_back(rd);
        if (go.knn_stats != 0)
            fprintf(stderr, "[scanrs nearest_neighbors] stride %llu: %llu points, candidates per query mean %.1f max %u, %u lists overflowed\n",
                    (unsigned long long)st, (unsigned long long)n_sub, (double)rd.cand_sum / (double)n_q, rd.cand_max, rd.overflowed);
        if (!rows.empty()) { // overflowed lists (heavy ties, tight clusters): those queries search this subset exhaustively, in place
            DevBuf<uint32_t> d_rows(rows.size());
            kf_h2d(s, d_rows.p, rows.data(), rows.size() * 4);
            km_exhaustive(s, dmax, KmExhaustive{Q, P, pl, d_rows.p, rows.size(), n_sub, st, k, dout, dkey, kth.p});
            SCANRS_SYNC(s); // d_rows is released on leaving this block
        }
    }
    SCANRS_SYNC(s);
    stats.filtered = true;
    return true;
}

// the prepared rows of one side and the memory they live in (kept across the blocks of a sharded search)
struct KmPrepared {
    DevBuf<double> C, sxx, Z;
    DevBuf<unsigned long long> info;
    KmRows rows;
};
// with_z: the standardised rows are made only where the filter can take the shape; then this waits for the window test
void km_prepare(hipStream_t s, int kind, const double *X, uint32_t ld, uint64_t n, uint32_t d, uint32_t dmax, bool with_z, KmPrepared &r) {
    if (r.C.n < n * dmax) r.C.alloc(n * dmax);
    if (r.sxx.n < n) r.sxx.alloc(n);
    if (with_z && r.Z.n < n * d) r.Z.alloc(n * d);
    if (!r.info.p) r.info.alloc(3);
    const unsigned long long init[3] = {0ull, ~0ull, 0ull};
    kf_h2d(s, r.info.p, init, 24);
    hipLaunchKernelGGL(km_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kind, X, ld, n, d, dmax, r.C.p, r.sxx.p,
                       with_z ? r.Z.p : nullptr, r.info.p);
    SCANRS_HIP(hipGetLastError());
    r.rows = KmRows{r.C.p, r.sxx.p, with_z ? r.Z.p : nullptr, n, false};
    if (with_z) {
        unsigned long long h[3];
        kf_d2h(s, h, r.info.p, 24);
        double lo, hi;
        memcpy(&lo, &h[1], 8);
        memcpy(&hi, &h[2], 8);
        r.rows.in_window = h[0] == 0 && lo >= KM_SXX_MIN && hi <= KM_SXX_MAX; // (false for NaN)
    }
}

// true: the filter answered
bool km_search(hipStream_t s, const KmRows &Q, const KmRows &P, uint32_t dmax, uint32_t d, uint32_t k, const KmPlace &pl, uint32_t *dout,
               double *dkey, KnnLastStats &stats) {
    if (km_filtered(s, Q, P, dmax, d, k, pl, dout, dkey, stats)) return true;
    stats = KnnLastStats();
    km_exhaustive(s, dmax, KmExhaustive{Q, P, pl, nullptr, Q.n, P.n, 1, k, dout, dkey, nullptr});
    return false;
}

void km_refuse_not_finite(hipStream_t s, const double *X, uint32_t ld, uint64_t n, uint32_t d, const char *what) {
    if (!n) return;
    DevBuf<unsigned long long> first(1);
    SCANRS_HIP(hipMemsetAsync(first.p, 0xFF, 8, s));
    hipLaunchKernelGGL(km_scan_kernel, dim3((unsigned)std::min<uint64_t>((n * d + 255) / 256, 2048)), dim3(256), 0, s, X, ld, n, d, first.p);
    const unsigned long long bad = SCANRS_D2H_VALUE(first.p, s);
    if (bad != ~0ull) fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: row %llu of the %s holds a coordinate that is not finite", bad, what);
}

// n_q queries against n_p >= 1 points in device memory (one array where the pointers, leading dimensions and counts coincide);
// indices / distances: host arrays, n_q x k
void km_two_sets(const double *dq, uint64_t n_q, uint32_t ld_q, const double *dp, uint64_t n_p, uint32_t ld_p, uint32_t d, uint32_t k, int kind,
                 bool skip, uint32_t *indices, double *distances) {
    hipStream_t s = 0;
    DevBuf<uint32_t> dout(n_q * k);
    DevBuf<double> ddist(n_q * k);
    if (kind == EUCLIDEAN) {
        knn_device_into(dq, ld_q, n_q, dp, ld_p, n_p, d, k, skip, dout.p, ddist.p);
        km_sqrt(s, ddist.p, n_q * k); // +inf padding stays +inf
    } else {
        const GlobalOptions &go = global_options();
        const uint32_t dmax = km_dmax(d);
        const bool same = dq == dp && ld_q == ld_p && n_q == n_p;
        const bool may_filter = !go.knn_exhaustive && d <= KF_DMAX && k <= KF_KMAX && n_q >= KF_NQ_MIN && n_p >= go.knn_filter_min_points;
        KmPrepared P, Qown;
        km_prepare(s, kind, dp, ld_p, n_p, d, dmax, may_filter, P);
        if (!same) km_prepare(s, kind, dq, ld_q, n_q, d, dmax, may_filter, Qown);
        KmPlace pl;
        pl.skip = skip ? 1 : 0;
        KnnLastStats stats;
        km_search(s, same ? P.rows : Qown.rows, P.rows, dmax, d, k, pl, dout.p, ddist.p, stats);
        km_square(s, ddist.p, n_q * k);
        knn_publish_stats(std::move(stats));
    }
    SCANRS_HIP(hipGetLastError());
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
        knn_sharded_blocks(st, d_pts, ld, begin, n_local, n, d, k, bs, out, distances);
        return;
    }
    const GlobalOptions &go = global_options();
    const uint64_t largest = std::min<uint64_t>(std::max<uint64_t>(1, go.knn_block_rows), n);
    KmPrepared Q, P;
    KfQueries qs;
    bool ready = false, may_filter = false;
    uint32_t dmax = 0;
    // (called after the first exchange has checked the arguments)
    bs.search = [&](hipStream_t s, const double *blk, uint64_t rows, uint64_t b0, const double *seed, uint32_t *bidx, double *bkey,
                    KnnLastStats &stats) {
        if (!ready) {
            dmax = km_dmax(d);
            may_filter = !go.knn_exhaustive && d <= KF_DMAX && k <= KF_KMAX && n_local >= KF_NQ_MIN && largest >= go.knn_filter_min_points;
            km_prepare(s, kind, d_pts, ld, n_local, d, dmax, may_filter, Q);
            may_filter = may_filter && Q.rows.in_window;
            if (may_filter) kf_prepare_queries(s, Q.rows.Z, d, n_local, d, qs);
            ready = true;
        }
        km_prepare(s, kind, blk, d, rows, d, dmax, may_filter, P);
        KmPlace pl;
        pl.p_off = b0;
        pl.q_off = begin;
        pl.seed = seed;
        pl.seed_ld = k;
        pl.queries = may_filter ? &qs : nullptr;
        if (km_search(s, Q.rows, P.rows, dmax, d, k, pl, bidx, bkey, stats)) st.knn_blocks_filtered++;
    };
    bs.finish = km_square;
    knn_sharded_blocks(st, d_pts, ld, begin, n_local, n, d, k, bs, out, distances);
}


// scanrs_init(): one empty launch per translation unit makes the runtime load this file's code object now instead of inside the
// first real call
__global__ void warm_knn_metric_kernel() {}
void warm_knn_metric(hipStream_t s) { hipLaunchKernelGGL(warm_knn_metric_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
