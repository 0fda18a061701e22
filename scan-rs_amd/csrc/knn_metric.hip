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

// Exhaustive route. Query t is row qrows[t] (or t) of C; the candidates are rows 0, p_stride, 2 p_stride, ... (n_sub of them), each
// wave-uniform. The inner loop is the unfused dot product s_xy over the padded row, then D and key = sqrt(D) (knn_metric.hpp).
// Writes, at the query's own row: the indices (rows of C), key * key, and kth = the k-th key (+inf while fewer than k exist).
template <int DMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void km_exhaustive_kernel(const double *__restrict__ C, const double *__restrict__ sxx,
                                                                const uint32_t *__restrict__ qrows, uint64_t n_q, uint64_t n_sub,
                                                                uint64_t p_stride, uint32_t k, uint32_t *__restrict__ out,
                                                                double *__restrict__ out_d, double *__restrict__ kth) {
    const uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool live = t < n_q;
    const uint64_t qrow = live ? (qrows ? (uint64_t)qrows[t] : t) : 0;
    double q[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; j++) q[j] = live ? C[qrow * DMAX + j] : 0.0;
    const double s_q = live ? sxx[qrow] : 0.0;
    double best_d[KMAX];
    uint32_t best_i[KMAX];
    uint32_t have = 0;
    double worst = INFINITY; // key a candidate has to beat once the list is full
    for (uint64_t pi = 0; pi < n_sub; pi++) {
        const uint64_t prow = pi * p_stride;
        const double *__restrict__ pt = C + prow * DMAX;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < DMAX; j++) s = s + q[j] * pt[j];
        if (!live || prow == qrow) continue; // query.idx != idx, knn.rs:155
        const double key = sqrt(pair_value(s_q, sxx[prow], s));
        if (have == k && !(key < worst)) continue;
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
        out_d[qrow * k + i] = i < have ? best_d[i] * best_d[i] : INFINITY;
    }
    if (kth) kth[qrow] = have == k ? best_d[k - 1] : INFINITY;
}

template <int DMAX, int THREADS>
void km_launch(hipStream_t s, const double *C, const double *sxx, const uint32_t *qrows, uint64_t n_q, uint64_t n_sub, uint64_t p_stride,
               uint32_t k, uint32_t *out, double *out_d, double *kth) {
    hipLaunchKernelGGL((km_exhaustive_kernel<DMAX, THREADS>), dim3((unsigned)((n_q + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, C, sxx, qrows,
                       n_q, n_sub, p_stride, k, out, out_d, kth);
}
// the instances of knn.hip's exhaustive(): the padded width of a row for d coordinates
uint32_t km_dmax(uint32_t d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 52 ? 52 : d <= 64 ? 64 : 128; }
void km_exhaustive(hipStream_t s, uint32_t dmax, const double *C, const double *sxx, const uint32_t *qrows, uint64_t n_q, uint64_t n_sub,
                   uint64_t p_stride, uint32_t k, uint32_t *out, double *out_d, double *kth) {
    if (n_q == 0) return;
    switch (dmax) {
    case 8: km_launch<8, 256>(s, C, sxx, qrows, n_q, n_sub, p_stride, k, out, out_d, kth); break;
    case 16: km_launch<16, 256>(s, C, sxx, qrows, n_q, n_sub, p_stride, k, out, out_d, kth); break;
    case 32: km_launch<32, 256>(s, C, sxx, qrows, n_q, n_sub, p_stride, k, out, out_d, kth); break;
    case 52: km_launch<52, 256>(s, C, sxx, qrows, n_q, n_sub, p_stride, k, out, out_d, kth); break;
    case 64: km_launch<64, 256>(s, C, sxx, qrows, n_q, n_sub, p_stride, k, out, out_d, kth); break;
    default: km_launch<128, 64>(s, C, sxx, qrows, n_q, n_sub, p_stride, k, out, out_d, kth); break;
    }
    SCANRS_HIP(hipGetLastError());
}

// The rerank of the filtered route: kf_rerank_kernel's shape (one wave per query, a candidate per lane, k rounds of a wave-wide
// lexicographic minimum), with the reference formula on C / sxx as the value of a pair and (key, index) as the order. Writes the
// indices, key * key and the query's k-th key (+inf while fewer than k exist). Overflowed lists (cnt > KF_CAP) are left alone.
__global__ __launch_bounds__(256) void km_rerank_kernel(const double *__restrict__ C, uint32_t ldc, const double *__restrict__ sxx, uint64_t n_q,
                                                        uint32_t d, uint32_t k, const uint32_t *__restrict__ cand,
                                                        const uint32_t *__restrict__ cnt, uint32_t *__restrict__ out,
                                                        double *__restrict__ out_d, double *__restrict__ kth_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= n_q) return;
    const uint32_t c = cnt[q];
    if (c > KF_CAP) return; // the host reads cnt and redoes this query exhaustively
    double key[KF_PER_LANE];
    uint32_t idx[KF_PER_LANE];
    const double *__restrict__ qr = C + q * ldc;
    const double s_q = sxx[q];
#pragma unroll
    for (uint32_t u = 0; u < KF_PER_LANE; u++) {
        const uint32_t j = u * 64u + lane;
        key[u] = INFINITY;
        idx[u] = 0xFFFFFFFFu;
        if (j < c) {
            const uint32_t p = cand[q * KF_CAP + j];
            if ((uint64_t)p != q) {
                const double *__restrict__ pr = C + (uint64_t)p * ldc;
                double s = 0.0;
                for (uint32_t t = 0; t < d; t++) s = s + qr[t] * pr[t];
                key[u] = sqrt(pair_value(s_q, sxx[p], s));
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
                    out_d[q * k + r2] = INFINITY;
                }
            full = false;
            break;
        }
        if (lane == 0) {
            out[q * k + it] = wi;
            out_d[q * k + it] = wd * wd;
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
__global__ void km_tau_kernel(const double *__restrict__ kth, uint64_t n, double *__restrict__ tau) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const double kk = kth[q] * kth[q];
    tau[q] = 2.0 * kk * (1.0 + KM_DELTA) + KM_E;
}

__global__ void km_sqrt_kernel(double *__restrict__ x, uint64_t n) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) x[e] = sqrt(x[e]);
}

// The filtered route: knn_filtered's rounds (knn.hip) on the standardised rows Z - nested strided subsets, the coarsest ranked
// exactly, every further one through the filter with the threshold of the round before, overflowed lists redone exhaustively.
// false: the filter declines (a shape it does not take, a degenerate row, s_xx outside the window) and nothing has been written.
bool km_filtered(hipStream_t s, const double *C, uint32_t dmax, const double *sxx, const double *Z, bool in_window, uint64_t n, uint32_t d,
                 uint32_t k, uint32_t *dout, double *ddist, KnnLastStats &stats) {
    const GlobalOptions &go = global_options();
    if (go.knn_exhaustive != 0 || d > KF_DMAX || n < go.knn_filter_min_points || k > KF_KMAX || n < KF_NQ_MIN || !in_window || !Z) return false;
    if (n > 0xFFFFFFFFull / KF_CAP) return false; // the candidate lists are addressed in 32 bits per query
    const uint64_t ratio = std::max<uint64_t>(2, go.knn_ratio);
    std::vector<uint64_t> strides;
    uint64_t st0 = 1;
    while ((n + st0 - 1) / st0 > KF_CAP) st0 *= 2;
    for (uint64_t st = st0; st > 1;) {
        st = st / ratio > 0 ? st / ratio : 1;
        strides.push_back(st);
    }
    if (strides.empty()) return false;
    KfOperands op;
    if (!kf_prepare(s, Z, d, n, Z, d, n, d, op)) return false;
    stats.first_stride = st0;
    DevBuf<double> tau(n), kth(n);
    DevBuf<uint32_t> cnt(n), cand(n * KF_CAP);
    const dim3 g4((unsigned)((n + 3) / 4)), g256((unsigned)((n + 255) / 256)), b256(256);
    { // round 0: exact ranking of the coarsest subset
        const uint32_t n0 = (uint32_t)((n + st0 - 1) / st0);
        hipLaunchKernelGGL(kf_fill_all_kernel, dim3((unsigned)((n * n0 + 255) / 256)), b256, 0, s, n, n0, st0, cand.p, cnt.p);
        hipLaunchKernelGGL(km_rerank_kernel, g4, b256, 0, s, C, dmax, sxx, n, d, k, cand.p, cnt.p, dout, ddist, kth.p);
    }
    std::vector<uint32_t> h_cnt(n);
    for (uint64_t st : strides) {
        const uint64_t n_sub = (n + st - 1) / st;
        hipLaunchKernelGGL(km_tau_kernel, g256, b256, 0, s, kth.p, n, tau.p);
        kf_filter_pass(s, op, tau.p, n, n, st, cand.p, cnt.p);
        hipLaunchKernelGGL(km_rerank_kernel, g4, b256, 0, s, C, dmax, sxx, n, d, k, cand.p, cnt.p, dout, ddist, kth.p);
        SCANRS_HIP(hipGetLastError());
        kf_d2h(s, h_cnt.data(), cnt.p, n * 4);
        KfRound rd{st, n_sub, 0, 0, 0};
        std::vector<uint32_t> rows;
        for (uint64_t q = 0; q < n; q++) {
            const uint32_t c = h_cnt[q];
            rd.cand_sum += c; // an overflowed list counts with what its counter reached
            rd.cand_max = std::max(rd.cand_max, c);
            if (c > KF_CAP) rows.push_back((uint32_t)q);
        }
        rd.overflowed = (uint32_t)rows.size();
        stats.rounds.push_back(rd);
        if (go.knn_stats != 0)
            fprintf(stderr, "[scanrs nearest_neighbors] stride %llu: %llu points, candidates per query mean %.1f max %u, %u lists overflowed\n",
                    (unsigned long long)st, (unsigned long long)n_sub, (double)rd.cand_sum / (double)n, rd.cand_max, rd.overflowed);
        if (!rows.empty()) { // overflowed lists (heavy ties, tight clusters): those queries search this subset exhaustively, in place
            DevBuf<uint32_t> d_rows(rows.size());
            kf_h2d(s, d_rows.p, rows.data(), rows.size() * 4);
            km_exhaustive(s, dmax, C, sxx, d_rows.p, rows.size(), n_sub, st, k, dout, ddist, kth.p);
            SCANRS_SYNC(s); // d_rows is released on leaving this block
        }
    }
    SCANRS_SYNC(s);
    stats.filtered = true;
    return true;
}

} // namespace

void nearest_neighbors_device(const double *d_data, uint64_t n, uint32_t ld, uint32_t d, uint32_t k, int kind, uint32_t *indices,
                              double *distances) {
    nearest_neighbors_check_args(n, ld, d, k, kind);
    if (k == 0 || n == 0) return;
    hipStream_t s = 0;
    {
        DevBuf<unsigned long long> first(1);
        SCANRS_HIP(hipMemsetAsync(first.p, 0xFF, 8, s));
        hipLaunchKernelGGL(km_scan_kernel, dim3((unsigned)std::min<uint64_t>((n * d + 255) / 256, 2048)), dim3(256), 0, s, d_data, ld, n, d, first.p);
        const unsigned long long bad = SCANRS_D2H_VALUE(first.p, s);
        if (bad != ~0ull) fail(SCANRS_ERR_ARGUMENT, "nearest_neighbors: row %llu of the data holds a coordinate that is not finite", bad);
    }
    if (n < 2) { // no other row: padding only
        for (uint32_t i = 0; i < k; i++) indices[i] = 0xFFFFFFFFu, distances[i] = INFINITY;
        return;
    }
    DevBuf<uint32_t> dout(n * k);
    DevBuf<double> ddist(n * k);
    if (kind == EUCLIDEAN) {
        knn_device_into(d_data, ld, n, d_data, ld, n, d, k, true, dout.p, ddist.p);
        hipLaunchKernelGGL(km_sqrt_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, s, ddist.p, n * k); // +inf padding stays +inf
    } else {
        const GlobalOptions &go = global_options();
        const uint32_t dmax = km_dmax(d);
        // the standardised rows are made only where the filter can take the shape
        const bool may_filter = !go.knn_exhaustive && d <= KF_DMAX && k <= KF_KMAX && n >= KF_NQ_MIN && n >= go.knn_filter_min_points;
        DevBuf<double> C(n * dmax), sxx(n), Z;
        if (may_filter) Z.alloc(n * d);
        DevBuf<unsigned long long> info(3);
        const unsigned long long init[3] = {0ull, ~0ull, 0ull};
        kf_h2d(s, info.p, init, 24);
        hipLaunchKernelGGL(km_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kind, d_data, ld, n, d, dmax, C.p, sxx.p, Z.p, info.p);
        SCANRS_HIP(hipGetLastError());
        KnnLastStats stats;
        bool done = false;
        if (may_filter) {
            unsigned long long h[3];
            kf_d2h(s, h, info.p, 24);
            double lo, hi;
            memcpy(&lo, &h[1], 8);
            memcpy(&hi, &h[2], 8);
            const bool in_window = h[0] == 0 && lo >= KM_SXX_MIN && hi <= KM_SXX_MAX; // (false for NaN)
            done = km_filtered(s, C.p, dmax, sxx.p, Z.p, in_window, n, d, k, dout.p, ddist.p, stats);
        }
        if (!done) {
            stats = KnnLastStats();
            km_exhaustive(s, dmax, C.p, sxx.p, nullptr, n, n, 1, k, dout.p, ddist.p, nullptr);
        }
        knn_publish_stats(std::move(stats));
    }
    SCANRS_HIP(hipGetLastError());
    SCANRS_HIP(hipMemcpy(indices, dout.p, n * k * 4, hipMemcpyDeviceToHost));
    SCANRS_HIP(hipMemcpy(distances, ddist.p, n * k * 8, hipMemcpyDeviceToHost));
}

// scanrs_init(): one empty launch per translation unit makes the runtime load this file's code object now instead of inside the
// first real call
__global__ void warm_knn_metric_kernel() {}
void warm_knn_metric(hipStream_t s) { hipLaunchKernelGGL(warm_knn_metric_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
