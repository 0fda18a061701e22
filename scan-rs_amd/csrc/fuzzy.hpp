// fuzzy.hpp — the arithmetic of fuzzy_simplicial_set (umap-rs/src/fuzzy.rs:30-181) and of the pruned edge list
// (embedding.rs:38-53, 75-85), written once for the kernels of fuzzy.hip and the host twin of fuzzy_host.cpp. DESIGN.md §7r.
// Every operation is a separate IEEE f64 operation: both files are built with -ffp-contract=off, and nothing here calls the
// platform's libm except floor (exact). The reference is followed literally, also where it looks like a slip; those places say so.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define FZ_HD __host__ __device__ inline
#else
#define FZ_HD inline
#endif

namespace scanrs {
namespace fuzzy {

constexpr double FZ_BANDWIDTH = 1.0;         // fuzzy.rs:7
constexpr uint32_t FZ_NITER = 64;            // fuzzy.rs:8
constexpr double FZ_SMOOTH_K_TOLERANCE = 1e-5; // fuzzy.rs:9
constexpr double FZ_MIN_K_DIST_SCALE = 1e-3; // fuzzy.rs:10
constexpr uint32_t FZ_KMAX = 128;
constexpr uint32_t FZ_NO_INDEX = 0xFFFFFFFFu; // P::MAX of the reference's padded lists
constexpr uint32_t FZ_TREE = 256;             // the width of one node of the global-mean tree

// what a row is refused for; the smaller code wins within a row, the smaller row wins overall (code = row * 4 + kind)
enum { FZ_BAD_NAN = 0, FZ_BAD_INDEX = 1, FZ_BAD_RHO = 2, FZ_BAD_REPEAT = 3 };

FZ_HD uint64_t fz_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}
FZ_HD double fz_from_bits(uint64_t u) {
    double x;
    memcpy(&x, &u, 8);
    return x;
}
// f64::max of Rust: the other operand where one is NaN
FZ_HD double fz_max(double a, double b) { return (a != a) ? b : (b != b) ? a : (a < b ? b : a); }

// The library's own exponential: the argument reduction and the rational form of fdlibm's e_exp.c (x = k ln2 + r, |r| <= ln2 / 2,
// exp(r) = 1 + r + r c / (2 - c) with c = r - r^2 P(r^2)), whose authors bound its error below 1 ulp; tests/test_fuzzy_cpu.py measures
// it against mpmath. Unfused IEEE operations only, so the host and the device return the same bits for every argument.
// fz_exp(+-0) = 1, fz_exp(-inf) = 0, NaN -> NaN, gradual underflow below 2^-1022, +inf above the overflow threshold.
FZ_HD double fz_exp(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    if (x != x) return x + x;
    if (x > 7.09782712893383973096e+02) return INFINITY;
    if (x < -7.45133219101941108420e+02) return 0.0;
    const double ax = x < 0.0 ? -x : x;
    double hi = x, lo = 0.0;
    int k = 0;
    if (ax > 0.34657359027997264) { // 0.5 ln2
        k = (int)(inv_ln2 * x + (x < 0.0 ? -0.5 : 0.5));
        const double t = (double)k;
        hi = x - t * ln2_hi; // t * ln2_hi is exact: ln2_hi has 32 significant bits, |t| < 2^11
        lo = t * ln2_lo;
        x = hi - lo;
    } else if (ax < 3.725290298461914e-09) { // 2^-28
        return 1.0 + x;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    if (k >= -1021) return fz_from_bits(fz_bits(y) + ((uint64_t)(int64_t)k << 52)); // y * 2^k, exact
    // below the normal range: y * 2^(k + 1000) is exact, the last product rounds once into the subnormals
    return fz_from_bits(fz_bits(y) + ((uint64_t)(int64_t)(k + 1000) << 52)) * 9.33263618503218878990e-302;
}

// rho of one row (fuzzy.rs:79-99). dist(j): the row's distances in column order. false: the reference would index past the end of
// non_zero_dist (non_zero_dist[index] with index == len, or non_zero_dist[0] of an empty list) and panic; the caller refuses.
template <class Row>
FZ_HD bool fz_rho(const Row &dist, uint32_t k, double local_connectivity, double *rho_out) {
    // `local_connectivity as usize`: truncation, saturating (the caller has refused NaN and negatives)
    const uint64_t lc_trunc = local_connectivity >= 18446744073709551615.0 ? ~0ull : (uint64_t)local_connectivity;
    const double index_f = floor(local_connectivity);
    const double interpolation = local_connectivity - index_f;
    const uint64_t index = lc_trunc; // floor == truncation for a value >= 0
    uint64_t len = 0;
    double first = 0.0, at_im1 = 0.0, at_i = 0.0, mx = -DBL_MAX; // Q::MIN
    for (uint32_t j = 0; j < k; j++) {
        const double v = dist(j);
        if (v > 0.0) { // +inf counts
            if (len == 0) first = v;
            if (len + 1 == index) at_im1 = v;
            if (len == index) at_i = v;
            mx = fz_max(mx, v);
            len++;
        }
    }
    double rho = 0.0;
    if (len >= lc_trunc) {
        if (index_f > 0.0) {
            rho = at_im1;
            if (interpolation > FZ_SMOOTH_K_TOLERANCE) {
                if (index >= len) return false;
                rho = rho + interpolation * (at_i - at_im1);
            }
        } else {
            if (len == 0) return false;
            rho = interpolation * first;
        }
    } else if (len != 0) {
        rho = mx;
    }
    *rho_out = rho;
    return true;
}

// smooth_knn_dist (fuzzy.rs:117-145). target = log2(k) * bandwidth is formed once by the caller, on the host. psum folds v, NOT
// v - rho: max(max(v, -rho), 0) is what the reference writes (fuzzy.rs:126), and it is kept.
template <class Row>
FZ_HD double fz_smooth_knn_dist(const Row &dist, uint32_t k, double rho, double target, uint32_t n_iter, uint32_t *iterations) {
    double lo = 0.0, mid = 1.0, hi = DBL_MAX;
    uint32_t it = 0;
    for (; it < n_iter;) {
        it++;
        double psum = 0.0;
        for (uint32_t j = 0; j < k; j++) psum = psum + fz_exp(-(fz_max(fz_max(dist(j), -rho), 0.0) / mid));
        const double diff = psum - target;
        if ((diff < 0.0 ? -diff : diff) < FZ_SMOOTH_K_TOLERANCE) break;
        if (psum > target) {
            hi = mid;
            mid = lo + (hi - lo) / 2.0;
        } else {
            lo = mid;
            if (hi == DBL_MAX)
                mid = mid * 2.0;
            else
                mid = lo + (hi - lo) / 2.0;
        }
    }
    if (iterations) *iterations = it;
    return mid;
}

template <class Row>
FZ_HD double fz_row_fold(const Row &dist, uint32_t k) {
    double acc = 0.0;
    for (uint32_t j = 0; j < k; j++) acc = acc + dist(j);
    return acc;
}

// the floor of a row with rho > 0 (fuzzy.rs:103-108)
FZ_HD double fz_floor_row(double sigma, double fold, uint32_t k) {
    const double m = FZ_MIN_K_DIST_SCALE * (fold / (double)k);
    return sigma < m ? m : sigma;
}
// the floor of the other rows (fuzzy.rs:109-111); total: the sum over all rows' folds (the tree of fz_tree_host / fz_tree_kernel)
FZ_HD double fz_floor_global(double sigma, double total, uint64_t n, uint32_t k) {
    const double m = FZ_MIN_K_DIST_SCALE * (total / ((double)n * (double)k));
    return sigma < m ? m : sigma;
}

// one membership strength (fuzzy.rs:166-172). The reference compares the column POSITION j with the neighbour's index
// (`j == knn_indices[[i, j]]`, where a self test would compare i): kept as written.
FZ_HD double fz_membership(uint32_t j, uint32_t index, double d, double rho, double sigma) {
    if (j == index) return 0.0;
    const double e = d - rho;
    if (e <= 0.0 || sigma == 0.0) return 1.0;
    return fz_exp(-(e / sigma));
}

// the fuzzy union at one position (fuzzy.rs:52-58); a missing operand is +0.0. Symmetric in (r, t).
FZ_HD double fz_union(double r, double t, double ratio) {
    const double sum = r + t;
    const double prod = r * t;
    const double lhs = (sum - prod) * ratio;
    const double rhs = prod * (1.0 - ratio);
    return lhs + rhs;
}

// embedding.rs:40-44: does the value survive the pruning and the `!= 0.0` test?
FZ_HD bool fz_edge_kept(double v, double threshold) { return !(v < threshold) && v != 0.0; }
// make_epochs_per_sample (embedding.rs:75-85)
FZ_HD double fz_epochs_per_sample(double w, double max_w, double n_epochs) {
    const double n = (w / max_w) * n_epochs;
    return n > 0.0 ? n_epochs / n : -1.0;
}

// One level of the global-mean tree: node b sums entries [b * FZ_TREE, (b + 1) * FZ_TREE) (a missing one is +0.0) by halving strides
// 128, 64, .., 1 (a[t] += a[t + s]); the levels repeat until one node is left. The shape depends on the count alone.
inline double fz_tree_host(const double *x, uint64_t n) {
    if (n == 0) return 0.0;
    std::vector<double> cur(x, x + n), nxt;
    do {
        const uint64_t m = cur.size(), nodes = (m + FZ_TREE - 1) / FZ_TREE;
        nxt.assign(nodes, 0.0);
        for (uint64_t b = 0; b < nodes; b++) {
            double a[FZ_TREE];
            for (uint32_t t = 0; t < FZ_TREE; t++) a[t] = b * FZ_TREE + t < m ? cur[b * FZ_TREE + t] : 0.0;
            for (uint32_t s = FZ_TREE / 2; s >= 1; s >>= 1)
                for (uint32_t t = 0; t < s; t++) a[t] = a[t] + a[t + s];
            nxt[b] = a[0];
        }
        cur.swap(nxt);
    } while (cur.size() > 1);
    return cur[0];
}

} // namespace fuzzy
} // namespace scanrs
