// knn_search.hpp — the one exact nearest-neighbour search under knn.hip (squared Euclidean distance) and knn_metric.hip (Pearson and
// cosine distance): templates over a distance policy `Dist`, instantiated in each of the two files under that file's compile flags
// (knn_metric.hip is built with -ffp-contract=off, knn.hip is not). This header holds NO floating-point arithmetic beyond comparisons
// and fmin: every operation that decides a bit of a key is in the policy, three device functions,
//     step(acc, q_j, p_j)         one coordinate of the fold over a pair of rows
//     finish(acc, aux_q, aux_p)   the fold -> the key the pair is ranked by (aux: the optional per-row scalar of either side)
//     threshold(key)              a query's k-th key -> the threshold of the bf16 filter (kf_filter_pass, knn_filter.hpp)
// Two routes, both ordered by (key, index) with ties in ascending index order:
//  * knn_exhaustive_kernel: one thread per query with its row in registers, the candidate row wave-uniform (scalar loads of whole
//    zero-padded rows), a sorted k-list per thread in private memory. Answers every shape.
//  * knn_filtered: nested strided subsets of the points. The coarsest is ranked exactly for every query (knn_rerank_kernel: one wave
//    per query, a candidate per lane), every further one goes through the bf16-MFMA filter with the threshold of the round before and
//    the rerank kernel ranks what passes. A query whose candidate list overflows searches that subset exhaustively, in place.
// A search may be one block of a larger one (KnnPlace): the self exclusion compares global rows, and a seed - the k-th key the query
// already holds - is strict: the exhaustive kernel drops a candidate unless key < seed, the filter's threshold takes min(seed, own
// k-th key), the rerank kernel drops nothing because of it (the merge of knn_shard.hpp does).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "common.hpp"
#include "knn_filter.hpp"

namespace scanrs {

// where a search stands in a larger one (all defaults: the points are the whole set and the queries its rows, as in scanrs_knn)
struct KnnPlace {
    uint64_t p_off = 0, q_off = 0;      // the global rows of point row 0 and of query 0
    int skip = 1;                       // drop the pair whose global rows coincide
    const double *seed = nullptr;       // per query the k-th key it already holds (element q * seed_ld; +inf: none)
    uint64_t seed_ld = 0;
    const KfQueries *queries = nullptr; // the query side of the filter, prepared once for all blocks
};
// one side of a search
struct KnnRows {
    const double *X = nullptr; // the rows the exact kernels read
    uint32_t ld = 0;
    const double *aux = nullptr; // a scalar per row for Dist::finish, or null
    const double *F = nullptr;   // the rows the filter reads
    uint32_t ldf = 0;
    uint64_t n = 0;
    bool may_filter = false; // this side is fit for the filter (the shapes and the filter's own magnitude window are tested by the search)
    // Point side only. The exhaustive kernel loads whole zero-padded rows (n x knn_dmax(d)) through the scalar cache. Empty: X is that
    // copy (ld == knn_dmax(d)). Otherwise it returns the copy and makes it on first use, so that a filtered search none of whose
    // lists overflows never pays for one.
    std::function<const double *()> padded;
};
// the padded width of a row for d coordinates: the instances of the exhaustive kernel
inline uint32_t knn_dmax(uint32_t d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 52 ? 52 : d <= 64 ? 64 : 128; }

// Query t is row qrows[t] (or t) of Q; the candidates are rows 0, p_stride, 2 p_stride, ... of P (n_sub of them), each wave-uniform.
// Writes, at the query's own row: the indices (rows of P, UINT32_MAX padded), the keys (+inf padded; out_key may be null) and kth =
// the k-th key (+inf while fewer than k exist; may be null).
template <class Dist, int DMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void knn_exhaustive_kernel(const double *__restrict__ Q, uint32_t ldq, const double *__restrict__ aux_q,
                                                                 const double *__restrict__ P, const double *__restrict__ aux_p, uint32_t d,
                                                                 const uint32_t *__restrict__ qrows, uint64_t n_q, uint64_t n_sub,
                                                                 uint64_t p_stride, uint64_t p_off, uint64_t q_off, int skip,
                                                                 const double *__restrict__ seed, uint64_t seed_ld, uint32_t k,
                                                                 uint32_t *__restrict__ out, double *__restrict__ out_key, double *__restrict__ kth) {
    const uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool live = t < n_q;
    const uint64_t qrow = live ? (qrows ? (uint64_t)qrows[t] : t) : 0;
    double q[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; j++) q[j] = (live && (uint32_t)j < d) ? Q[qrow * ldq + j] : 0.0;
    const double a_q = (live && aux_q) ? aux_q[qrow] : 0.0;
    double best_d[KMAX];
    uint32_t best_i[KMAX];
    uint32_t have = 0;
    // the key a candidate has to beat: the seed, then the list's own k-th key once it is full (never above the seed, since every
    // entry beat it). +inf means "no bound yet": a key of +inf is a legitimate one and still enters a list that is not full
    double worst = (live && seed) ? seed[qrow * seed_ld] : INFINITY;
    for (uint64_t pi = 0; pi < n_sub; pi++) {
        const uint64_t prow = pi * p_stride;
        const double *__restrict__ pt = P + prow * DMAX;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < DMAX; j++) s = Dist::step(s, q[j], pt[j]);
        // The pair of one global row is the query itself. Written as this sum and not against a hoisted row number: with the latter
        // the Euclidean instances load a candidate row in pieces (66 SGPRs instead of 106) and the kernel runs 45 % longer.
        if (!live || (skip && p_off + prow == q_off + qrow)) continue;
        const double key = Dist::finish(s, a_q, aux_p ? aux_p[prow] : 0.0);
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
        out[qrow * k + i] = i < have ? best_i[i] : 0xFFFFFFFFu;
        if (out_key) out_key[qrow * k + i] = i < have ? best_d[i] : INFINITY;
    }
    if (kth) kth[qrow] = have == k ? best_d[k - 1] : INFINITY;
}

// one exhaustive search: n_q queries (rows qrows[t] of Q, or its first n_q rows) against rows 0, p_stride, ... of P (n_sub of them)
struct KnnExhaustive {
    KnnRows Q, P;
    KnnPlace pl;
    uint32_t d, k;
    const uint32_t *qrows;
    uint64_t n_q, n_sub, p_stride;
    uint32_t *out;
    double *out_key, *kth;
};
template <class Dist, int DMAX, int THREADS>
void knn_launch(hipStream_t s, const KnnExhaustive &e, const double *padded) {
    hipLaunchKernelGGL((knn_exhaustive_kernel<Dist, DMAX, THREADS>), dim3((unsigned)((e.n_q + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, e.Q.X,
                       e.Q.ld, e.Q.aux, padded, e.P.aux, e.d, e.qrows, e.n_q, e.n_sub, e.p_stride, e.pl.p_off, e.pl.q_off, e.pl.skip, e.pl.seed,
                       e.pl.seed_ld, e.k, e.out, e.out_key, e.kth);
}
template <class Dist>
void knn_exhaustive(hipStream_t s, const KnnExhaustive &e) {
    if (e.n_q == 0) return;
    if (!e.P.padded && e.P.ld != knn_dmax(e.d)) fail(SCANRS_ERR_ARGUMENT, "knn: the point rows are not padded to the kernel's width");
    const double *p = e.P.padded ? e.P.padded() : e.P.X;
    switch (knn_dmax(e.d)) {
    case 8: knn_launch<Dist, 8, 256>(s, e, p); break;
    case 16: knn_launch<Dist, 16, 256>(s, e, p); break;
    case 32: knn_launch<Dist, 32, 256>(s, e, p); break;
    case 52: knn_launch<Dist, 52, 256>(s, e, p); break; // top-50 PCA scores, the default of scan-rs-cmd (tools/src/bin/cmd.rs:46-48)
    case 64: knn_launch<Dist, 64, 256>(s, e, p); break;
    default: knn_launch<Dist, 128, 64>(s, e, p); break;
    }
    SCANRS_HIP(hipGetLastError());
}

// Exact ranking of a query's candidates: one wave per query, a candidate per lane (the fold of the exhaustive kernel over the d
// coordinates), then k rounds of a wave-wide lexicographic (key, index) minimum. Query q is row q of Q, a candidate a row of P.
// Writes the indices (UINT32_MAX padded), the keys (+inf padded; out_key may be null) and the query's k-th key (+inf while fewer than
// k exist). Overflowed lists (cnt > KF_CAP) are left alone.
// An empty slot is recognised by its index UINT32_MAX and not by a sentinel key, because +inf is a legitimate Pearson / cosine key.
// For the squared Euclidean distance that is the result a sentinel key of DBL_MAX gave: the filter runs only inside its magnitude
// window (max |coordinate| <= 2^46, d <= 58), where every squared distance is finite and below DBL_MAX.
template <class Dist>
__global__ __launch_bounds__(256) void knn_rerank_kernel(const double *__restrict__ Q, uint32_t ldq, const double *__restrict__ aux_q,
                                                         const double *__restrict__ P, uint32_t ldp, const double *__restrict__ aux_p, uint64_t n_q,
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
    const double *__restrict__ qr = Q + q * ldq;
    const double a_q = aux_q ? aux_q[q] : 0.0;
    const uint64_t self = skip ? q_off + q - p_off : ~0ull; // the point row that is the query itself, if any
#pragma unroll
    for (uint32_t u = 0; u < KF_PER_LANE; u++) {
        const uint32_t j = u * 64u + lane;
        key[u] = INFINITY;
        idx[u] = 0xFFFFFFFFu;
        if (j < c) {
            const uint32_t p = cand[q * KF_CAP + j];
            if ((uint64_t)p != self) {
                const double *__restrict__ pr = P + (uint64_t)p * ldp;
                double s = 0.0;
                for (uint32_t t = 0; t < d; t++) s = Dist::step(s, qr[t], pr[t]);
                key[u] = Dist::finish(s, a_q, aux_p ? aux_p[p] : 0.0);
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
                    if (out_key) out_key[q * k + r2] = INFINITY;
                }
            full = false;
            break;
        }
        if (lane == 0) {
            out[q * k + it] = wi;
            if (out_key) out_key[q * k + it] = wd;
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

// the k-th key of a query -> the filter's threshold; +inf: everything passes. Of a seeded search: the smaller of that key and the
// seed - a point at or beyond the seed is no part of the answer either
template <class Dist>
__global__ void knn_threshold_kernel(const double *__restrict__ kth, const double *__restrict__ seed, uint64_t seed_ld, uint64_t n,
                                     double *__restrict__ tau) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    tau[q] = Dist::threshold(seed ? fmin(kth[q], seed[q * seed_ld]) : kth[q]);
}

// The filtered route. Nested strided subsets S_0 < S_1 < ... < all points: S_0 (at most KF_CAP points, KF_SEED_N0 of a seeded search)
// is ranked exactly for every query, which gives an upper bound of the k-th key; every further subset is "knn_ratio" times denser and
// goes through the filter with the threshold of the round before. false: the filter declines (a shape it does not take, a side that
// may not take it, a coordinate of the filter rows outside its magnitude window) and nothing has been written.
// who: the search's name in the "knn_stats" lines on stderr.
template <class Dist>
bool knn_filtered(hipStream_t s, const char *who, const KnnRows &Q, const KnnRows &P, uint32_t d, uint32_t k, const KnnPlace &pl, uint32_t *dout,
                  double *dkey, KnnLastStats &stats) {
    const GlobalOptions &go = global_options(); // scanrs_set_global_option (read per call: tests flip them)
    const uint64_t n_q = Q.n, n_p = P.n;
    if (go.knn_exhaustive != 0 || d > KF_DMAX || n_p < go.knn_filter_min_points || k > KF_KMAX || n_q < KF_NQ_MIN) return false;
    if (!Q.may_filter || !P.may_filter) return false;
    // default ratio 4: 1M x 50, k = 15: 487 ms at 4, 553 at 8, 606 at 16 (fewer passes, but longer candidate lists and the first overflows)
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
    if (!kf_prepare(s, Q.F, Q.ldf, n_q, P.F, P.ldf, n_p, d, op, pl.queries)) return false; // outside the magnitude window
    stats.first_stride = st0;
    DevBuf<double> tau(n_q), kth(n_q);
    DevBuf<uint32_t> cnt(n_q), cand(n_q * KF_CAP);
    const dim3 g4((unsigned)((n_q + 3) / 4)), g256((unsigned)((n_q + 255) / 256)), b256(256);
    auto rerank = [&] {
        hipLaunchKernelGGL(knn_rerank_kernel<Dist>, g4, b256, 0, s, Q.X, Q.ld, Q.aux, P.X, P.ld, P.aux, n_q, d, k, pl.p_off, pl.q_off, pl.skip, cand.p,
                           cnt.p, dout, dkey, kth.p);
    };
    { // round 0: exact ranking of the coarsest subset
        const uint32_t n0 = (uint32_t)((n_p + st0 - 1) / st0);
        hipLaunchKernelGGL(kf_fill_all_kernel, dim3((unsigned)((n_q * n0 + 255) / 256)), b256, 0, s, n_q, n0, st0, cand.p, cnt.p);
        rerank();
    }
    std::vector<uint32_t> h_cnt(n_q);
    for (uint64_t st : strides) {
        const uint64_t n_sub = (n_p + st - 1) / st;
        hipLaunchKernelGGL(knn_threshold_kernel<Dist>, g256, b256, 0, s, kth.p, pl.seed, pl.seed_ld, n_q, tau.p);
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
            fprintf(stderr, "[scanrs %s] stride %llu: %llu points, candidates per query mean %.1f max %u, %u lists overflowed\n", who,
                    (unsigned long long)st, (unsigned long long)n_sub, (double)rd.cand_sum / (double)n_q, rd.cand_max, rd.overflowed);
        if (!rows.empty()) { // overflowed lists (heavy ties, tight clusters): those queries search this subset exhaustively, in place
            DevBuf<uint32_t> d_rows(rows.size());
            kf_h2d(s, d_rows.p, rows.data(), rows.size() * 4);
            knn_exhaustive<Dist>(s, KnnExhaustive{Q, P, pl, d, k, d_rows.p, rows.size(), n_sub, st, dout, dkey, kth.p});
            SCANRS_SYNC(s); // d_rows is released on leaving this block
        }
    }
    SCANRS_SYNC(s);
    stats.filtered = true;
    return true;
}

// the whole search: the filtered route where it takes the shape, the exhaustive kernel otherwise. true: the filter answered
template <class Dist>
bool knn_search(hipStream_t s, const char *who, const KnnRows &Q, const KnnRows &P, uint32_t d, uint32_t k, const KnnPlace &pl, uint32_t *dout,
                double *dkey, KnnLastStats &stats) {
    if (knn_filtered<Dist>(s, who, Q, P, d, k, pl, dout, dkey, stats)) return true;
    stats = KnnLastStats(); // declined (possibly after the magnitude check): nothing of the filter ran
    knn_exhaustive<Dist>(s, KnnExhaustive{Q, P, pl, d, k, nullptr, Q.n, P.n, 1, dout, dkey, nullptr});
    return false;
}

} // namespace scanrs
