// knn.hip — exact k-nearest-neighbours of the PCA scores (scan-rs/src/nn.rs:38-83), SURVEY.md §8 f4.
//
// The reference builds a ball tree (ball_tree crate) over the rows of a cells x d matrix and asks it for the k+1
// nearest points of every row, dropping the row itself. Same result here by search over all pairs, in two forms:
//  * knn_kernel (small point sets, d > 58, k > 64): one thread per query (its d coordinates in registers), the candidate point
//    wave-uniform in SGPRs (scalar loads), the squared distance as the reference forms it (sum of squared differences,
//    nn.rs:14-21 — not the |p|^2 + |q|^2 - 2 p.q expansion, whose cancellation would reorder near neighbours), a sorted k-list
//    per thread in private memory. f64 vector FMA bound: n_q x n x d multiply-adds (8 s at 10^6 x 50).
//  * the filtered form (>= 32768 points, max |coordinate| inside the magnitude window): the distance matrix is GEMM-shaped, so its bulk runs on the matrix cores
//    (v_mfma_f32_32x32x16_bf16) as a FILTER with a rigorous error margin, and only the few pairs that pass are ranked, by the
//    exact f64 distance above (kf_* kernels below: 0.54 s at 10^6 x 50, k = 15, identical output; `python tools/knn_bench.py
//    1000000 50 15`, same MI355X: 479 ms with the margin 0.0021 this file had until it was re-derived, 102 candidates per query in
//    the last round; 536 ms and 158 candidates with 0.00395. Subtracting a common centre before kf_prep_* would shrink the
//    |q|^2 + |p|^2 the margin is relative to and win that back: not done yet).
//  * over a sharded point set (knn_sharded at the end of this file): the points pass by in global blocks, each block
//    searched by the two forms above (seeded with what the query already holds) and merged into a running list per query by
//    (squared distance, global index) - knn_merge.hpp. Equal to the search of the whole set bit for bit, whatever the cut.
// Ties keep ascending index order (the rule of the reference's own test oracle, `exhaustive_knn`, nn.rs:112-137; the ball
// tree's order among exactly equidistant points is a property of that crate).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "knn_filter.hpp"
#include "knn_merge.hpp"
#include "knn_shard.hpp"
#include "shard_exchange.hpp"

namespace scanrs {

namespace {

template <int DMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void knn_kernel(const double *__restrict__ queries, uint64_t n_q, const double *__restrict__ points,
                                                     uint64_t n_p, uint32_t d, uint32_t k, int skip_same_index, uint64_t skip_stride,
                                                     uint64_t p_off, uint64_t q_off, uint32_t *__restrict__ out,
                                                     double *__restrict__ out_d) {
    const uint64_t qi = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool live = qi < n_q;
    double q[DMAX];
#pragma unroll
    for (int j = 0; j < DMAX; j++) q[j] = (live && (uint32_t)j < d) ? queries[qi * d + j] : 0.0;
    double best_d[KMAX];
    uint32_t best_i[KMAX];
    uint32_t have = 0;
    double worst = DBL_MAX; // distance a candidate has to beat once the list is full
    // `points` is the (n_p x DMAX) zero-padded copy: the candidate's coordinates are wave-uniform, so they arrive through
    // the scalar cache into SGPRs (s_load_dwordx16) and every lane's VALU work is just subtract + fma per coordinate
    for (uint64_t pi = 0; pi < n_p; pi++) {
        const double *__restrict__ pt = points + pi * DMAX;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < DMAX; j++) {
            const double t = pt[j] - q[j];
            s = fma(t, t, s);
        }
        // candidate pi is row pi * skip_stride of the point set, whose row 0 is global row p_off; query qi is global row q_off + qi
        if (!live || (skip_same_index && p_off + pi * skip_stride == q_off + qi)) continue;
        if (have == k && !(s < worst)) continue;
        // sorted insertion; equal distances stay in index order because candidates arrive in index order
        uint32_t pos = have < k ? have : k - 1u;
        while (pos > 0 && best_d[pos - 1] > s) {
            best_d[pos] = best_d[pos - 1];
            best_i[pos] = best_i[pos - 1];
            pos--;
        }
        best_d[pos] = s;
        best_i[pos] = (uint32_t)pi;
        if (have < k) have++;
        if (have == k) worst = best_d[k - 1];
    }
    if (!live) return;
    for (uint32_t i = 0; i < k; i++) out[qi * k + i] = i < have ? best_i[i] : 0xFFFFFFFFu; // T::max_value() padding, nn.rs:66
    if (out_d)
        for (uint32_t i = 0; i < k; i++) out_d[qi * k + i] = i < have ? best_d[i] : INFINITY;
}

// dst row r = src row r * row_stride, zero-padded to dmax columns
__global__ void pad_points_kernel(const double *__restrict__ src, uint32_t ld, uint64_t n, uint32_t d, uint32_t dmax,
                                  double *__restrict__ dst, uint64_t row_stride) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * dmax) return;
    const uint64_t r = e / dmax;
    const uint32_t j = (uint32_t)(e % dmax);
    dst[e] = j < d ? src[r * row_stride * ld + j] : 0.0;
}

template <int DMAX, int THREADS>
void launch(const double *dq, uint32_t ldq, uint64_t n_q, const double *dp, uint32_t ldp, uint64_t n_p, uint32_t d, uint32_t k, int skip,
            uint32_t *dout, hipStream_t s, uint64_t p_stride, uint64_t p_off, uint64_t q_off, double *ddist) {
    // p_stride > 1: the candidates are rows 0, p_stride, 2 p_stride, ... of dp (n_p of them); indices written are subset-local
    // zero-padded (n x DMAX) copies: the candidate's coordinates arrive as whole scalar-cache lines, the query's as one run per thread
    DevBuf<double> pp, qp;
    pp.alloc(n_p * DMAX ? n_p * DMAX : 1);
    if (n_p)
        hipLaunchKernelGGL(pad_points_kernel, dim3((unsigned)((n_p * DMAX + 255) / 256)), dim3(256), 0, s, dp, ldp, n_p, d, (uint32_t)DMAX, pp.p, p_stride);
    const double *q = pp.p;
    if (dq != dp || n_q != n_p || ldq != ldp || p_stride != 1) {
        qp.alloc(n_q * DMAX);
        hipLaunchKernelGGL(pad_points_kernel, dim3((unsigned)((n_q * DMAX + 255) / 256)), dim3(256), 0, s, dq, ldq, n_q, d, (uint32_t)DMAX, qp.p, (uint64_t)1);
        q = qp.p;
    }
    const dim3 grid((unsigned)((n_q + THREADS - 1) / THREADS)), block(THREADS);
    hipLaunchKernelGGL((knn_kernel<DMAX, THREADS>), grid, block, 0, s, q, n_q, pp.p, n_p, (uint32_t)DMAX, k, skip, p_stride, p_off, q_off, dout,
                       ddist);
    SCANRS_SYNC(s); // the padded copies are released on return
}

// exhaustive search of every query against rows 0, p_stride, 2 p_stride, ... of the point set (n_sub of them); subset-local indices.
// p_off / q_off: the global rows of point row 0 and of query 0 (what the self exclusion compares); ddist: the k squared distances
// beside the indices (+inf in padded slots), or nullptr
void exhaustive(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, const double *dp, uint32_t ldp, uint64_t n_sub, uint32_t d,
                uint32_t k, int skip, uint32_t *dout, uint64_t p_stride = 1, uint64_t p_off = 0, uint64_t q_off = 0, double *ddist = nullptr) {
    if (d <= 8)
        launch<8, 256>(dq, ldq, n_q, dp, ldp, n_sub, d, k, skip, dout, s, p_stride, p_off, q_off, ddist);
    else if (d <= 16)
        launch<16, 256>(dq, ldq, n_q, dp, ldp, n_sub, d, k, skip, dout, s, p_stride, p_off, q_off, ddist);
    else if (d <= 32)
        launch<32, 256>(dq, ldq, n_q, dp, ldp, n_sub, d, k, skip, dout, s, p_stride, p_off, q_off, ddist);
    else if (d <= 52) // top-50 PCA scores, the default of scan-rs-cmd (tools/src/bin/cmd.rs:46-48)
        launch<52, 256>(dq, ldq, n_q, dp, ldp, n_sub, d, k, skip, dout, s, p_stride, p_off, q_off, ddist);
    else if (d <= 64)
        launch<64, 256>(dq, ldq, n_q, dp, ldp, n_sub, d, k, skip, dout, s, p_stride, p_off, q_off, ddist);
    else
        launch<128, 64>(dq, ldq, n_q, dp, ldp, n_sub, d, k, skip, dout, s, p_stride, p_off, q_off, ddist);
    SCANRS_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// Large point sets: filter on the matrix cores, decide in f64.
//
// The distance matrix is GEMM-shaped work, so its bulk goes to bf16 MFMA (v_mfma_f32_32x32x16_bf16) — but only as a
// FILTER whose error is bounded rigorously; every neighbour that is returned was ranked by the exact f64 distance
// (sum of squared differences in coordinate order, nn.rs:14-21), ties by index, exactly as the exhaustive kernel does.
//   d^2(q, p) = |q|^2 + |p|^2 - 2 G,  G = q.p, and with tau_q an upper bound of q's (computed) k-th distance a true neighbour
//   has T = G + tau_q / 2 - (|q|^2 + |p|^2) / 2 = (tau_q - d^2) / 2 >= 0. The tile computes
//       T~ = G~ + A_q - N_p,   A_q = tau_q / 2 - |q|^2 (1/2 - gamma),   N_p = |p|^2 (1/2 - gamma),
//   i.e. T plus the margin gamma (|q|^2 + |p|^2), and the margin has to cover every error of T~ (write S = |q|^2 + |p|^2):
//    * operands. A coordinate goes f64 -> f32 (relative 2^-24) -> bf16. bf16 has 8 significant bits, so round to nearest has
//      unit roundoff u = 2^-8 (NOT 2^-9): x~ = x (1 + e), |e| <= eps = 2^-8 (1 + 2^-15). Per coordinate
//      |q~_j p~_j - q_j p_j| <= (2 eps + eps^2) |q_j p_j|, and with Cauchy-Schwarz sum |q_j p_j| <= |q| |p| <= S / 2:
//      |sum q~_j p~_j - G| <= (eps + eps^2 / 2) S = 0.0039140 S   (2^-8 (1 + 2^-9) = 0.0039139 is the floor no bf16 filter of
//      this form gets under).
//    * accumulation. The products of two bf16 are exact in f32; the 64 operand slots of a row (4 chained 32x32x16 MFMAs) are
//      summed in f32 in an order the hardware does not document. Allowing every slot an error of 2 ulp of the running (or the
//      largest) magnitude, whatever the order: <= eta (sum of |terms|), eta = 64 * 2 * 2^-24 = 2^-17 ... taken as 2^-16.
//      The terms are the products (<= (1 + eps)^2 S / 2), the three pieces of A (|A| <= tau / 2 + |q|^2 / 2) and of N
//      (<= |p|^2 / 2), pieces summing to <= (1 + 2^-7) of their value. With tau = d^2 + 2 T and d^2 <= 2 S:
//      sum |terms| <= 2.02 S + 1.01 T, so this error is <= 2.02 * 2^-16 S = 0.0000309 S, plus 1.01 eta T which T itself absorbs.
//    * A and N. Both are formed in f64 (|q|^2, |p|^2 by an fma chain: 58 * 2^-53 relative), converted to f32 (2^-24) and split
//      into three bf16 pieces (split3: residual <= 2^-24 |v|); the shaves (1 - 4e-7) / (1 + 4e-7) = 6.7 * 2^-24 push those
//      2 * 2^-24 the safe way (N down, A up), so they cost nothing here; tau is the f64 distance the rerank kernel computed,
//      and "true neighbour" means the same computed distance (<= 1e-14 S apart from the exact one).
//   Sum: 0.0039140 + 0.0000309 = 0.0039449 < gamma = 0.00395 (the rest, 5e-6 S, is slack). The same bound read the other way
//   limits what passes: no candidate has d^2 > tau_q + 4 gamma S.
//   All of this is RELATIVE error analysis: it holds while no operand, product, piece or sum overflows or falls into the
//   f32 / bf16 subnormal range (which the matrix cores may flush). Hence the magnitude window on M = max |coordinate| of
//   queries and points (kf_maxabs_kernel, one pass): KF_COORD_MIN <= M <= KF_COORD_MAX, every coordinate finite; outside it
//   knn_filtered declines and the exhaustive kernel answers.
//    * upper end 2^46: |p|^2 <= 58 M^2, tau <= 232 M^2, so |A| <= 116 M^2 = 5.8e29 stays under KF_A_PASS = 9e29, the value
//      "everything passes" (tau = +inf) is clamped to, which itself stays under the 1e30 of the sentinel rows: a sentinel row
//      fails every test (9e29 - 1e30 < 0) and a real point passes the clamp (9e29 - |G~| - N >= 9e29 - 87 M^2 > 0).
//    * lower end 2^-48: single coordinates may still be tiny (or 0), so values below 2^-126 cannot be excluded; each such
//      value (a coordinate, a product, a piece of A or N, a partial sum) is off by at most 2^-126 absolutely if flushed, in
//      total <= 2^-126 (116 (1 + eps) M + 64 + 64 + 8) < 2^-118 (M + 1). A_q carries that as an absolute slack
//      2^-117 (M + 1), so completeness holds for every pair; the window only keeps the slack negligible against
//      gamma S for points of norm ~M (2^-117 against 0.004 * 2^-95 at the lower end), i.e. keeps the filter selective.
// A_q and N_p ride in spare k-slots of the operands (three bf16 pieces each, against 1.0 on the other side), so the
// accumulator tile IS the test value and the epilogue is one max-tree per tile plus a rare append to the query's
// candidate list. tau_q comes from exact searches on nested strided subsets (every 256th point exhaustively, then every
// 16th and finally all points through the filter): a round passes about k * 16 * (volume inflation of the margin)
// candidates per query, which the rerank kernel evaluates exactly. A query whose list overflows is redone exhaustively.
// (the constants KF_*, the operands and the statistics of a filtered search: knn_filter.hpp, shared with knn_metric.hip)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint16_t to_bf16(float f) { // round to nearest even
    uint32_t u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float from_bf16(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
// v = h + m + l up to 2^-24 |v|
__device__ __forceinline__ void split3(float v, uint16_t &h, uint16_t &m, uint16_t &l) {
    h = to_bf16(v);
    const float r1 = v - from_bf16(h);
    m = to_bf16(r1);
    l = to_bf16(r1 - from_bf16(m));
}

// operand rows of the point side: [p_0 .. p_{d-1}, 0.., 1, 1, 1, -N_h, -N_m, -N_l]; rows >= n are sentinels that fail every test
__global__ void kf_prep_points_kernel(const double *__restrict__ P, uint32_t ld, uint64_t n, uint64_t n_rows, uint32_t d,
                                      uint16_t *__restrict__ Pb) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    uint16_t *row = Pb + r * KF_DP;
    double nn = 0.0;
    for (uint32_t j = 0; j < KF_DP - 6; j++) {
        const double x = (r < n && j < d) ? P[r * ld + j] : 0.0;
        nn = fma(x, x, nn);
        row[j] = to_bf16((float)x);
    }
    // N rounded DOWN (it is subtracted): shave a few ulps before the split
    float nf = r < n ? (float)(nn * (0.5 - KF_GAMMA) * (1.0 - 4e-7)) : KF_SENTINEL;
    uint16_t h, m, l;
    split3(-nf, h, m, l);
    row[KF_DP - 6] = row[KF_DP - 5] = row[KF_DP - 4] = 0x3F80; // 1.0
    row[KF_DP - 3] = h;
    row[KF_DP - 2] = m;
    row[KF_DP - 1] = l;
}
// query side: [q_0 .. q_{d-1}, 0.., A_h, A_m, A_l, 1, 1, 1]; the A slots are rewritten every round
__global__ void kf_prep_queries_kernel(const double *__restrict__ Q, uint32_t ld, uint64_t n, uint64_t n_rows, uint32_t d,
                                       uint16_t *__restrict__ Qb, double *__restrict__ qn) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    uint16_t *row = Qb + r * KF_DP;
    double nn = 0.0;
    for (uint32_t j = 0; j < KF_DP - 6; j++) {
        const double x = (r < n && j < d) ? Q[r * ld + j] : 0.0;
        nn = fma(x, x, nn);
        row[j] = to_bf16((float)x);
    }
    if (r < n) qn[r] = nn;
    uint16_t h, m, l;
    split3(-KF_SENTINEL, h, m, l); // until a threshold is set nothing passes (and never for sentinel rows)
    row[KF_DP - 6] = h;
    row[KF_DP - 5] = m;
    row[KF_DP - 4] = l;
    row[KF_DP - 3] = row[KF_DP - 2] = row[KF_DP - 1] = 0x3F80;
}
// slack: the absolute error bound 2^-117 (M + 1) of values the matrix cores may flush (see the derivation above)
__global__ void kf_set_threshold_kernel(const double *__restrict__ tau, const double *__restrict__ qn, uint64_t n, double slack,
                                        uint16_t *__restrict__ Qb, uint32_t *__restrict__ cnt) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    cnt[r] = 0;
    double a = 0.5 * tau[r] - qn[r] * (0.5 - KF_GAMMA);
    a += fabs(a) * 4e-7 + slack; // rounded UP
    float af = a > KF_A_PASS ? (float)KF_A_PASS : (float)a; // tau = +inf (fewer than k neighbours so far): everything passes
    if (!(af == af)) af = (float)KF_A_PASS;
    uint16_t h, m, l;
    split3(af, h, m, l);
    uint16_t *row = Qb + r * KF_DP;
    row[KF_DP - 6] = h;
    row[KF_DP - 5] = m;
    row[KF_DP - 4] = l;
}

// max |x| over an n x d matrix as the bit pattern of the double: for non-negative doubles the unsigned order of the bits is the
// numerical order, +inf sorts above every finite value and NaN above +inf, so one atomicMax also reports non-finite input
__global__ __launch_bounds__(256) void kf_maxabs_kernel(const double *__restrict__ X, uint32_t ld, uint64_t n, uint32_t d,
                                                        unsigned long long *__restrict__ out) {
    unsigned long long m = 0ull;
    const uint64_t total = n * d, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step)
        m = max(m, (unsigned long long)__double_as_longlong(fabs(X[(e / d) * ld + (e % d)])));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned long long)__shfl_xor((long long)m, off, 64));
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(out, m);
}

// One wave: 128 queries (4 row blocks of 32) x 32 points per step; the 4 waves of a workgroup share the query tile and take
// every fourth 32-point block. Points are rows t * stride of Pb, t < n_sub; t >= n_sub reads the sentinel row. A passing
// (query, point) pair is parked in a per-wave LDS buffer (LDS atomic for the position, ~100 clk) and the buffer is flushed to the
// queries' global candidate lists in batches: with about one passing pair per tile a returning GLOBAL atomic per pair would
// stall the wave for a memory round trip every tile (and drain the prefetched point blocks with it). The buffer holds a whole
// 32 x 32 block of pairs and is flushed when the next block's pairs (at most 16 per lane that has one) might not fit, so no pair
// is ever dropped: where a large share of all pairs passes (a small or tightly clustered point set) a query still overflows only
// when its own list does.
constexpr uint32_t KF_BUF = 1024; // parked pairs per wave = the pairs of one 32 x 32 block
__device__ __forceinline__ void kf_flush(uint32_t lane, uint32_t n, const uint2 *buf, uint32_t *__restrict__ cand, uint32_t *__restrict__ cnt) {
    for (uint32_t e = lane; e < n; e += 64u) {
        const uint2 qp = buf[e];
        const uint32_t slot = atomicAdd(&cnt[qp.x], 1u);
        if (slot < KF_CAP) cand[(uint64_t)qp.x * KF_CAP + slot] = qp.y;
    }
}
__global__ __launch_bounds__(256, 2) void kf_filter_kernel(const uint16_t *__restrict__ Qb, uint64_t n_q, const uint16_t *__restrict__ Pb,
                                                           uint64_t n_sub, uint64_t stride, uint64_t sentinel_row,
                                                           uint32_t *__restrict__ cand, uint32_t *__restrict__ cnt) {
    __shared__ uint2 park[4][KF_BUF];
    __shared__ uint32_t park_n[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint64_t q0 = (uint64_t)blockIdx.x * 128u;
    if (lane == 0) park_n[wave] = 0u;
    uint32_t parked = 0u; // wave-uniform upper bound of park_n[wave]
    bf16x8 a[4][4];
#pragma unroll
    for (int rb = 0; rb < 4; rb++)
#pragma unroll
        for (int ks = 0; ks < 4; ks++)
            a[rb][ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(Qb + (q0 + 32u * rb + r) * KF_DP + 16u * ks + 8u * h));
    const uint64_t n_blocks = (n_sub + 31u) / 32u;
    auto load_b = [&](uint64_t blk, bf16x8 (&b)[4], uint32_t &prow) {
        const uint64_t t = blk * 32u + r;
        const uint64_t pr = t < n_sub ? t * stride : sentinel_row;
        prow = (uint32_t)pr;
#pragma unroll
        for (int ks = 0; ks < 4; ks++)
            b[ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(Pb + pr * KF_DP + 16u * ks + 8u * h));
    };
    // Register ring of KF_STAGES point blocks: the loads of block i + KF_STAGES are issued right after block i has been consumed, so
    // ~3 tiles of MFMA work (plus the SIMD's other wave) cover the L2 / HBM latency of every load. Blocks past the end read the
    // sentinel row: no branch around any load, so the loads in flight can be counted (counted s_waitcnt vmcnt).
    constexpr int KF_STAGES = 3;
    bf16x8 b[KF_STAGES][4];
    uint32_t prow[KF_STAGES];
#pragma unroll
    for (int st = 0; st < KF_STAGES; st++) load_b(wave + 4u * st, b[st], prow[st]);
    for (uint64_t base = wave; base < n_blocks; base += 4u * KF_STAGES) {
#pragma unroll
        for (int st = 0; st < KF_STAGES; st++) {
            const uint64_t blk = base + 4u * st;
            const uint32_t pr = prow[st];
#pragma unroll
            for (int half = 0; half < 2; half++) { // two row blocks at a time: 32 accumulator registers live instead of 64
                f32x16 acc[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    acc[e] = (f32x16){0};
#pragma unroll
                    for (int ks = 0; ks < 4; ks++)
                        acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2 * half + e][ks], b[st][ks], acc[e], 0, 0, 0);
                }
                if (half == 1) {
                    load_b(blk + 4u * KF_STAGES, b[st], prow[st]);
                    asm volatile("" ::: "memory"); // the refill is ISSUED here: left alone, the compiler sinks it next to its use, tiles later
                }
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int rb = 2 * half + e;
                    float mx = acc[e][0];
#pragma unroll
                    for (int i = 1; i < 16; i++) mx = fmaxf(mx, acc[e][i]);
                    const uint64_t lanes = __builtin_amdgcn_ballot_w64(mx >= 0.0f);
                    if (lanes == 0) continue; // no pair of this 32 x 32 block passes
                    const uint32_t room = 16u * (uint32_t)__popcll(lanes); // at most this many pairs follow (<= 1024 = KF_BUF)
                    if (parked + room > KF_BUF) {
                        parked = park_n[wave]; // the exact count
                        if (parked + room > KF_BUF) { // make room first
                            kf_flush(lane, parked, park[wave], cand, cnt);
                            if (lane == 0) park_n[wave] = 0u;
                            parked = 0u;
                        }
                    }
                    parked += room;
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        if (acc[e][i] >= 0.0f) { // sentinel rows (queries past n_q, points past the subset) never get here: their A / N slots are -/+1e30
                            const uint32_t q = (uint32_t)q0 + 32u * rb + (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h;
                            const uint32_t pos = atomicAdd(&park_n[wave], 1u);
                            if (pos < KF_BUF)
                                park[wave][pos] = make_uint2(q, pr);
                            else
                                atomicMax(&cnt[q], KF_CAP + 1u); // cannot happen (room was made above); if it did, the query would go to the exhaustive kernel
                        }
                    }
                }
            }
        }
    }
    kf_flush(lane, min(park_n[wave], KF_BUF), park[wave], cand, cnt);
}

// exact f64 ranking of a query's candidates: one wave per query, a candidate per lane (the same fma chain over the coordinates as
// knn_kernel), then k rounds of a wave-wide lexicographic (distance, index) minimum. Writes the k neighbours (UINT32_MAX padded)
// and tau = the k-th distance (+inf when fewer than k exist). Overflowed lists (cnt > KF_CAP) are left to the exhaustive kernel.
__global__ __launch_bounds__(256) void kf_rerank_kernel(const double *__restrict__ Q, uint32_t ldq, uint64_t n_q, const double *__restrict__ P,
                                                        uint32_t ldp, uint32_t d, uint32_t k, int skip_same_index, uint64_t p_off,
                                                        uint64_t q_off, const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cnt,
                                                        uint32_t *__restrict__ out, double *__restrict__ out_d, double *__restrict__ tau) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= n_q) return;
    const uint32_t c = cnt[q];
    if (c > KF_CAP) return; // the host reads cnt and redoes this query exhaustively
    double dist[KF_PER_LANE];
    uint32_t idx[KF_PER_LANE];
    const double *__restrict__ qr = Q + q * ldq;
#pragma unroll
    for (uint32_t u = 0; u < KF_PER_LANE; u++) {
        const uint32_t j = u * 64u + lane;
        dist[u] = DBL_MAX;
        idx[u] = 0xFFFFFFFFu;
        if (j < c) {
            const uint32_t p = cand[q * KF_CAP + j];
            if (!(skip_same_index && p_off + p == q_off + q)) { // global rows: the offsets are 0 unless the points are one block of a sharded set
                const double *__restrict__ pr = P + (uint64_t)p * ldp;
                double s = 0.0;
                for (uint32_t t = 0; t < d; t++) {
                    const double df = pr[t] - qr[t];
                    s = fma(df, df, s);
                }
                dist[u] = s;
                idx[u] = p;
            }
        }
    }
    double kth = DBL_MAX;
    for (uint32_t it = 0; it < k; it++) {
        // lane-local minimum, then the wave's
        double bd = DBL_MAX;
        uint32_t bi = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t u = 0; u < KF_PER_LANE; u++)
            if (dist[u] < bd || (dist[u] == bd && idx[u] < bi)) {
                bd = dist[u];
                bi = idx[u];
            }
        double wd = bd;
        uint32_t wi = bi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(wd, off, 64);
            const uint32_t oi = (uint32_t)__shfl_xor((int)wi, off, 64);
            if (od < wd || (od == wd && oi < wi)) {
                wd = od;
                wi = oi;
            }
        }
        if (lane == 0) out[q * k + it] = wi;
        if (lane == 0 && out_d) out_d[q * k + it] = wi == 0xFFFFFFFFu ? INFINITY : wd;
        if (wi == 0xFFFFFFFFu) { // fewer than k candidates: the rest is padding
            for (uint32_t r2 = it + 1; r2 < k; r2++)
                if (lane == 0) {
                    out[q * k + r2] = 0xFFFFFFFFu;
                    if (out_d) out_d[q * k + r2] = INFINITY;
                }
            kth = DBL_MAX;
            break;
        }
        kth = wd;
        // the owner retires that entry (indices are unique within a list: a point is appended once per round)
#pragma unroll
        for (uint32_t u = 0; u < KF_PER_LANE; u++)
            if (idx[u] == wi) {
                dist[u] = DBL_MAX;
                idx[u] = 0xFFFFFFFFu;
            }
    }
    if (lane == 0) tau[q] = kth == DBL_MAX ? INFINITY : kth;
}

// tau of round 0 from the exhaustive search on the coarsest subset: exact distance to the k-th neighbour found there
__global__ void kf_tau0_kernel(const double *__restrict__ Q, uint32_t ldq, uint64_t n_q, const double *__restrict__ P, uint32_t ldp,
                               uint32_t d, uint32_t k, uint64_t stride, const uint32_t *__restrict__ nbr, double *__restrict__ tau) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_q) return;
    const uint32_t t = nbr[q * k + (k - 1u)];
    if (t == 0xFFFFFFFFu) {
        tau[q] = INFINITY;
        return;
    }
    const double *pr = P + (uint64_t)t * stride * ldp, *qr = Q + q * ldq;
    double s = 0.0;
    for (uint32_t j = 0; j < d; j++) {
        const double df = pr[j] - qr[j];
        s = fma(df, df, s);
    }
    tau[q] = s;
}

__global__ void kf_gather_rows_kernel(const double *__restrict__ src, uint32_t ld, uint32_t d, const uint32_t *__restrict__ rows, uint64_t n,
                                      double *__restrict__ dst) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * d) return;
    dst[e] = src[(uint64_t)rows[e / d] * ld + (e % d)];
}
template <typename T>
__global__ void kf_scatter_result_kernel(const T *__restrict__ res, const uint32_t *__restrict__ rows, uint64_t n, uint32_t k,
                                         T *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * k) return;
    out[(uint64_t)rows[e / k] * k + (e % k)] = res[e];
}
// a seeded search (one block of a sharded point set): no threshold above the k-th distance the query already holds
// from the blocks before (seed[q * seed_ld]; +inf while it holds fewer than k)
__global__ void kf_seed_kernel(double *__restrict__ tau, const double *__restrict__ seed, uint64_t seed_ld, uint64_t n) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    tau[q] = fmin(tau[q], seed[q * seed_ld]);
}

// what the last scanrs_knn* / scanrs_find_nn / scanrs_nearest_neighbors* call of the process did (KnnLastStats, knn_filter.hpp)
std::mutex g_stats_mutex;
KnnLastStats g_last_stats;

// max |coordinate| of up to two matrices in one pass and one wait; NaN when a coordinate is not finite
double kf_maxabs(hipStream_t s, const double *a, uint32_t lda, uint64_t na, const double *b, uint32_t ldb, uint64_t nb, uint32_t d) {
    DevBuf<unsigned long long> mx(1);
    SCANRS_HIP(hipMemsetAsync(mx.p, 0, 8, s));
    auto reduce = [&](const double *x, uint32_t ld, uint64_t n) {
        const uint64_t blocks = std::min<uint64_t>((n * d + 255) / 256, 2048);
        hipLaunchKernelGGL(kf_maxabs_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, ld, n, d, mx.p);
    };
    if (na) reduce(a, lda, na);
    if (nb) reduce(b, ldb, nb);
    const unsigned long long bits = SCANRS_D2H_VALUE(mx.p, s);
    double m;
    memcpy(&m, &bits, 8);
    return m <= DBL_MAX ? m : NAN; // +inf and the NaN patterns sort above every finite value
}
void kf_launch_prep_queries(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, uint32_t d, KfQueries &qs) {
    qs.nq_rows = (n_q + 127) / 128 * 128;
    qs.Qb.alloc(qs.nq_rows * KF_DP);
    qs.qn.alloc(n_q);
    hipLaunchKernelGGL(kf_prep_queries_kernel, dim3((unsigned)((qs.nq_rows + 255) / 256)), dim3(256), 0, s, dq, ldq, n_q, qs.nq_rows, d, qs.Qb.p,
                       qs.qn.p);
}
} // namespace

// the query side alone, for a search whose points arrive in blocks: its max-abs pass and its operands are made once
void kf_prepare_queries(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, uint32_t d, KfQueries &qs) {
    qs.maxabs = kf_maxabs(s, dq, ldq, n_q, nullptr, 0, 0, d);
    if (qs.maxabs <= KF_COORD_MAX) kf_launch_prep_queries(s, dq, ldq, n_q, d, qs); // (false for NaN: nothing is prepared, no block is filtered)
}

// false: a coordinate is not finite or max |coordinate| lies outside the magnitude window; nothing has been prepared.
// shared: the query side prepared earlier by kf_prepare_queries (nullptr: it is prepared here)
bool kf_prepare(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, const double *dp, uint32_t ldp, uint64_t n_p, uint32_t d,
                KfOperands &op, const KfQueries *shared) {
    const bool own_queries = !shared && (dq != dp || ldq != ldp || n_q > n_p);
    double m = kf_maxabs(s, dp, ldp, n_p, dq, ldq, own_queries ? n_q : 0, d);
    if (shared) m = shared->maxabs > m ? shared->maxabs : (shared->maxabs == shared->maxabs ? m : NAN);
    if (!(m >= KF_COORD_MIN && m <= KF_COORD_MAX)) return false; // NaN fails the comparison too
    op.slack = 0x1p-117 * (m + 1.0);
    const uint64_t np_rows = n_p + 1; // one sentinel row behind the points
    op.Pb.alloc(np_rows * KF_DP);
    hipLaunchKernelGGL(kf_prep_points_kernel, dim3((unsigned)((np_rows + 255) / 256)), dim3(256), 0, s, dp, ldp, n_p, np_rows, d, op.Pb.p);
    if (shared) {
        op.q = shared;
    } else {
        kf_launch_prep_queries(s, dq, ldq, n_q, d, op.own);
        op.q = &op.own;
    }
    return true;
}
// one pass of the filter over rows 0, st, 2 st, ... of the points with the thresholds tau: cnt (n_q) and the lists cand (n_q x KF_CAP)
void kf_filter_pass(hipStream_t s, const KfOperands &op, const double *tau, uint64_t n_q, uint64_t n_p, uint64_t st, uint32_t *cand,
                    uint32_t *cnt) {
    const uint64_t n_sub = (n_p + st - 1) / st;
    hipLaunchKernelGGL(kf_set_threshold_kernel, dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, s, tau, op.q->qn.p, n_q, op.slack, op.q->Qb.p, cnt);
    hipLaunchKernelGGL(kf_filter_kernel, dim3((unsigned)(op.q->nq_rows / 128)), dim3(256), 0, s, op.q->Qb.p, n_q, op.Pb.p, n_sub, st, n_p, cand, cnt);
}

// The copies of a search. The entry points on stream 0 keep the blocking copies they have always made; a search on a handle's own
// (non-blocking) stream queues them there and waits for that stream alone, bounded like every wait of the library.
void kf_d2h(hipStream_t s, void *dst, const void *src, size_t bytes) {
    if (!s) {
        SCANRS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return;
    }
    SCANRS_D2H(dst, src, bytes, s);
    SCANRS_SYNC(s);
}
void kf_h2d(hipStream_t s, void *dst, const void *src, size_t bytes) {
    if (!s) {
        SCANRS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return;
    }
    SCANRS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    SCANRS_SYNC(s); // the source is pageable and the caller's again on return
}
void kf_d2d(hipStream_t s, void *dst, const void *src, size_t bytes) {
    if (!s)
        SCANRS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    else
        SCANRS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
}

namespace {

// where a search stands in a larger one (all defaults: the points are the whole set and the queries its rows, as in scanrs_knn)
struct KnnPlace {
    uint64_t p_off = 0, q_off = 0;   // the global rows of point row 0 and of query 0: the self exclusion compares global rows
    const double *seed = nullptr;    // seeded search: per query the k-th distance it already holds, element q * seed_ld
    uint64_t seed_ld = 0;
    const KfQueries *queries = nullptr; // the query side prepared once for all blocks
};

bool knn_filtered(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, const double *dp, uint32_t ldp, uint64_t n_p, uint32_t d,
                  uint32_t k, int skip, uint32_t *dout, double *ddist, KnnLastStats &stats, const KnnPlace &pl) {
    const GlobalOptions &go = global_options(); // scanrs_set_global_option (read per call: tests flip them)
    const bool off = go.knn_exhaustive != 0;
    const uint64_t min_points = go.knn_filter_min_points;
    if (off || d > KF_DMAX || n_p < min_points || k > KF_KMAX || n_q < KF_NQ_MIN) return false;
    const uint64_t n0_max = pl.seed ? KF_SEED_N0 : KF_CAP;
    auto seed_tau = [&](double *tau) {
        if (pl.seed) hipLaunchKernelGGL(kf_seed_kernel, dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, s, tau, pl.seed, pl.seed_ld, n_q);
    };
    // nested strided subsets S_0 < S_1 < ... < all points: S_0 (at most KF_CAP points) is ranked exactly for every query, which gives
    // an upper bound tau of the k-th distance; every further subset is `ratio` times denser and goes through the filter with the
    // previous tau, which lets about k * ratio * (volume inflation of the margin) pairs per query through.
    const uint64_t ratio = std::max<uint64_t>(2, go.knn_ratio); // default 4: 1M x 50, k = 15: 487 ms at 4, 553 at 8, 606 at 16 (fewer passes, but longer candidate lists and the first overflows)
    const bool print_stats = go.knn_stats != 0;
    std::vector<uint64_t> strides;
    uint64_t st0 = 1;
    while ((n_p + st0 - 1) / st0 > n0_max) st0 *= 2;
    for (uint64_t st = st0; st > 1;) {
        st = st / ratio > 0 ? st / ratio : 1;
        strides.push_back(st);
    }
    if (strides.empty()) return false;
    KfOperands op;
    if (!kf_prepare(s, dq, ldq, n_q, dp, ldp, n_p, d, op, pl.queries)) return false; // outside the magnitude window: the exhaustive kernel answers
    stats.first_stride = st0;
    DevBuf<double> tau(n_q);
    DevBuf<uint32_t> cnt(n_q), cand(n_q * KF_CAP);
    { // round 0: exact ranking of the coarsest subset
        const uint32_t n0 = (uint32_t)((n_p + st0 - 1) / st0);
        hipLaunchKernelGGL(kf_fill_all_kernel, dim3((unsigned)((n_q * n0 + 255) / 256)), dim3(256), 0, s, n_q, n0, st0, cand.p, cnt.p);
        hipLaunchKernelGGL(kf_rerank_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, s, dq, ldq, n_q, dp, ldp, d, k, skip, pl.p_off, pl.q_off,
                           cand.p, cnt.p, dout, ddist, tau.p);
        seed_tau(tau.p);
    }
    std::vector<uint32_t> h_cnt(n_q);
    for (uint64_t st : strides) {
        const uint64_t n_sub = (n_p + st - 1) / st;
        kf_filter_pass(s, op, tau.p, n_q, n_p, st, cand.p, cnt.p);
        hipLaunchKernelGGL(kf_rerank_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, s, dq, ldq, n_q, dp, ldp, d, k, skip, pl.p_off, pl.q_off,
                           cand.p, cnt.p, dout, ddist, tau.p);
        seed_tau(tau.p);
        SCANRS_HIP(hipGetLastError());
        // overflowed lists (rare: heavy ties, adversarial clusters): those queries are redone exhaustively on this subset
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
        if (print_stats)
            fprintf(stderr, "[scanrs knn] stride %llu: %llu points, candidates per query mean %.1f max %u, %u lists overflowed\n",
                    (unsigned long long)st, (unsigned long long)n_sub, (double)rd.cand_sum / (double)n_q, rd.cand_max, rd.overflowed);
        if (!rows.empty()) {
            const uint64_t m = rows.size();
            DevBuf<uint32_t> d_rows(m), res(m * k);
            DevBuf<double> qsel(m * d), tsel(m);
            kf_h2d(s, d_rows.p, rows.data(), m * 4);
            hipLaunchKernelGGL(kf_gather_rows_kernel, dim3((unsigned)((m * d + 255) / 256)), dim3(256), 0, s, dq, ldq, d, d_rows.p, m, qsel.p);
            // the self-exclusion rule compares row numbers, which the gathered copy has lost: search for k + 1 and drop the query's own row on the host
            const uint32_t kk = std::min<uint32_t>(k + (skip ? 1u : 0u), KMAX);
            DevBuf<uint32_t> res2(m * kk);
            DevBuf<double> dist2, dres;
            if (ddist) {
                dist2.alloc(m * kk);
                dres.alloc(m * k);
            }
            exhaustive(s, qsel.p, d, m, dp, ldp, n_sub, d, kk, 0, res2.p, st, 0, 0, dist2.p);
            std::vector<uint32_t> h_res(m * kk), h_out(m * k);
            std::vector<double> h_dist(ddist ? m * kk : 0), h_dout(ddist ? m * k : 0);
            kf_d2h(s, h_res.data(), res2.p, m * kk * 4);
            if (ddist) kf_d2h(s, h_dist.data(), dist2.p, m * kk * 8);
            for (uint64_t i = 0; i < m; i++) {
                uint32_t w = 0;
                for (uint32_t j = 0; j < kk && w < k; j++) {
                    const uint32_t t = h_res[i * kk + j];
                    const uint64_t prow = t == 0xFFFFFFFFu ? 0xFFFFFFFFull : (uint64_t)t * st;
                    if (skip && t != 0xFFFFFFFFu && pl.p_off + prow == pl.q_off + rows[i]) continue; // the query's own (global) row
                    if (ddist) h_dout[i * k + w] = t == 0xFFFFFFFFu ? INFINITY : h_dist[i * kk + j];
                    h_out[i * k + w++] = t == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)prow;
                }
                for (; w < k; w++) {
                    if (ddist) h_dout[i * k + w] = INFINITY;
                    h_out[i * k + w] = 0xFFFFFFFFu;
                }
            }
            kf_h2d(s, res.p, h_out.data(), m * k * 4);
            hipLaunchKernelGGL(kf_scatter_result_kernel<uint32_t>, dim3((unsigned)((m * k + 255) / 256)), dim3(256), 0, s, res.p, d_rows.p, m, k, dout);
            if (ddist) {
                kf_h2d(s, dres.p, h_dout.data(), m * k * 8);
                hipLaunchKernelGGL(kf_scatter_result_kernel<double>, dim3((unsigned)((m * k + 255) / 256)), dim3(256), 0, s, dres.p, d_rows.p, m, k, ddist);
            }
            // their thresholds for the next round: exact distance to the k-th neighbour just found (row indices now)
            if (st != 1) {
                DevBuf<uint32_t> nb(n_q * k);
                kf_d2d(s, nb.p, dout, n_q * k * 4);
                DevBuf<double> tau2(n_q);
                hipLaunchKernelGGL(kf_tau0_kernel, dim3((unsigned)((n_q + 255) / 256)), dim3(256), 0, s, dq, ldq, n_q, dp, ldp, d, k, (uint64_t)1, nb.p,
                                   tau2.p);
                std::vector<double> h_t(n_q), h_t2(n_q);
                kf_d2h(s, h_t.data(), tau.p, n_q * 8);
                kf_d2h(s, h_t2.data(), tau2.p, n_q * 8);
                for (uint32_t rq : rows) h_t[rq] = h_t2[rq];
                kf_h2d(s, tau.p, h_t.data(), n_q * 8);
                seed_tau(tau.p);
            }
        }
    }
    SCANRS_SYNC(s);
    stats.filtered = true;
    return true;
}

} // namespace

void knn_last_stats(bool &filtered, uint64_t &first_stride, std::vector<uint64_t> &strides, std::vector<uint64_t> &points,
                    std::vector<uint64_t> &cand_sum, std::vector<uint32_t> &cand_max, std::vector<uint32_t> &overflowed) {
    std::lock_guard<std::mutex> lock(g_stats_mutex);
    filtered = g_last_stats.filtered;
    first_stride = g_last_stats.first_stride;
    for (const KfRound &r : g_last_stats.rounds) {
        strides.push_back(r.stride);
        points.push_back(r.points);
        cand_sum.push_back(r.cand_sum);
        cand_max.push_back(r.cand_max);
        overflowed.push_back(r.overflowed);
    }
}

void knn_filter_params(double &gamma, uint32_t &cap, uint32_t &dmax, uint32_t &k_max, uint64_t &nq_min, double &coord_min, double &coord_max) {
    gamma = KF_GAMMA;
    cap = KF_CAP;
    dmax = KF_DMAX;
    k_max = KF_KMAX;
    nq_min = KF_NQ_MIN;
    coord_min = KF_COORD_MIN;
    coord_max = KF_COORD_MAX;
}

// scanrs_debug_knn_filter: the operands, thresholds and ONE filter pass of knn_filtered (the same kf_prepare / kf_filter_pass) on host arrays
void knn_filter_debug(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, const double *tau, uint64_t stride,
                      uint32_t *cnt, uint32_t *cand) {
    if (n_q == 0 || n_p == 0 || stride == 0) fail(SCANRS_ERR_ARGUMENT, "knn filter: empty input or stride 0");
    if (d == 0 || d > KF_DMAX) fail(SCANRS_ERR_ARGUMENT, "knn filter: 1 <= dimensions <= 58");
    if (n_p > 0xFFFFFFFEull || n_q > 0xFFFFFFFFull / KF_CAP) fail(SCANRS_ERR_SHAPE, "knn filter: too many points or queries");
    hipStream_t s = 0;
    DevBuf<double> dq(n_q * d), dp(n_p * d), dtau(n_q);
    DevBuf<uint32_t> dcnt(n_q), dcand(n_q * KF_CAP);
    SCANRS_HIP(hipMemcpy(dq.p, queries, n_q * d * 8, hipMemcpyHostToDevice));
    SCANRS_HIP(hipMemcpy(dp.p, points, n_p * d * 8, hipMemcpyHostToDevice));
    SCANRS_HIP(hipMemcpy(dtau.p, tau, n_q * 8, hipMemcpyHostToDevice));
    SCANRS_HIP(hipMemsetAsync(dcand.p, 0xFF, n_q * KF_CAP * 4, s)); // slots the pass does not write read UINT32_MAX
    KfOperands op;
    if (!kf_prepare(s, dq.p, d, n_q, dp.p, d, n_p, d, op))
        fail(SCANRS_ERR_ARGUMENT, "knn filter: a coordinate is not finite or max |coordinate| is outside the magnitude window");
    kf_filter_pass(s, op, dtau.p, n_q, n_p, stride, dcand.p, dcnt.p);
    SCANRS_HIP(hipGetLastError());
    SCANRS_SYNC(s);
    SCANRS_HIP(hipMemcpy(cnt, dcnt.p, n_q * 4, hipMemcpyDeviceToHost));
    SCANRS_HIP(hipMemcpy(cand, dcand.p, n_q * KF_CAP * 4, hipMemcpyDeviceToHost));
}

void knn_publish_stats(KnnLastStats &&stats) {
    std::lock_guard<std::mutex> lock(g_stats_mutex);
    g_last_stats = std::move(stats);
}

namespace {
void knn_check_args(uint32_t ld_q, uint32_t ld_p, uint64_t n_p, uint32_t d, uint32_t k) {
    if (k > KMAX) fail(SCANRS_ERR_ARGUMENT, "knn: k must not exceed 128");
    if (d == 0 || d > 128) fail(SCANRS_ERR_ARGUMENT, "knn: 1 <= dimensions <= 128");
    if (ld_q < d || ld_p < d) fail(SCANRS_ERR_ARGUMENT, "knn: leading dimension smaller than the number of coordinates");
    if (n_p > 0xFFFFFFFEull) fail(SCANRS_ERR_SHAPE, "knn: too many points for u32 indices");
}
} // namespace

void knn_device_into(const double *d_queries, uint32_t ld_q, uint64_t n_q, const double *d_points, uint32_t ld_p, uint64_t n_p, uint32_t d,
                     uint32_t k, bool skip_same_index, uint32_t *d_out, double *d_sq) {
    if (k == 0 || n_q == 0) return;
    knn_check_args(ld_q, ld_p, n_p, d, k);
    const int skip = skip_same_index ? 1 : 0;
    KnnLastStats stats;
    if (!knn_filtered(0, d_queries, ld_q, n_q, d_points, ld_p, n_p, d, k, skip, d_out, d_sq, stats, KnnPlace())) {
        stats = KnnLastStats(); // declined (possibly after the magnitude check): nothing of the filter ran
        exhaustive(0, d_queries, ld_q, n_q, d_points, ld_p, n_p, d, k, skip, d_out, 1, 0, 0, d_sq);
    }
    SCANRS_HIP(hipGetLastError());
    knn_publish_stats(std::move(stats));
}

void knn_device(const double *d_queries, uint32_t ld_q, uint64_t n_q, const double *d_points, uint32_t ld_p, uint64_t n_p, uint32_t d,
                uint32_t k, bool skip_same_index, uint32_t *out, double *sq_dist) {
    if (k == 0 || n_q == 0) return;
    knn_check_args(ld_q, ld_p, n_p, d, k);
    DevBuf<uint32_t> dout;
    DevBuf<double> ddist;
    dout.alloc(n_q * k);
    if (sq_dist) ddist.alloc(n_q * k);
    knn_device_into(d_queries, ld_q, n_q, d_points, ld_p, n_p, d, k, skip_same_index, dout.p, ddist.p);
    SCANRS_HIP(hipMemcpy(out, dout.p, n_q * k * 4, hipMemcpyDeviceToHost));
    if (sq_dist) SCANRS_HIP(hipMemcpy(sq_dist, ddist.p, n_q * k * 8, hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------------------------------------------------------------
// The search over a sharded point set: every rank owns the queries of its own cells, the point set passes by in
// global blocks that one u64 all-reduce hands to every rank (each slot of the zeroed buffer has one writer, so the sum is the bit
// pattern itself), each block is searched with the machinery above, seeded with what the query already holds, and its list is merged
// into the query's running list by (squared distance, global index). The result does not depend on the cut: it is the k smallest
// pairs under that total order, and the distance is the same fma chain everywhere. The walk (its kernels are in knn_shard.hpp) is
// shared with nearest_neighbors_sharded of knn_metric.hip, which brings its own search of one block (KnnBlockSearch).
void knn_sharded_blocks(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d, uint32_t k,
                        const KnnBlockSearch &bs, uint32_t *out, double *keys) {
    const hipStream_t s = st.stream;
    const uint32_t world = st.shard.world, rank = st.shard.rank;
    ShardExchange ex{st, st.knn_allreduces};
    // 1. The ranks agree: the same n, d, k and kind of search everywhere (a rank that differs would bring another count to a later
    //    exchange), and no coordinate that is not finite (with a NaN the order is not total and a blockwise merge could differ from
    //    one pass).
    const bool scannable = n_local && d && ld >= d && d_pts;
    DevBuf<unsigned long long> first(1), hdr(4);
    SCANRS_HIP(hipMemsetAsync(first.p, 0xFF, 8, s));
    if (scannable)
        hipLaunchKernelGGL(ks_scan_kernel, dim3((unsigned)std::min<uint64_t>((n_local * d + 255) / 256, 2048)), dim3(256), 0, s, d_pts, ld, n_local, d,
                           first.p);
    hipLaunchKernelGGL(ks_header_kernel, dim3(1), dim3(64), 0, s, hdr.p, n, d, k, bs.kind, begin, first.p);
    const std::vector<unsigned long long> h = ex.gather(hdr.p, 4);
    const unsigned long long kword = (unsigned long long)k | ((unsigned long long)(uint32_t)bs.kind << 32);
    unsigned long long bad = 0;
    for (uint32_t r = 0; r < world; r++) {
        if (h[4 * r] != n || h[4 * r + 1] != d || h[4 * r + 2] != kword)
            fail(SCANRS_ERR_ARGUMENT,
                 "%s: the ranks disagree (rank %u: n %llu, d %llu, k %llu, distance %llu; rank %u: n %llu, d %u, k %u, distance %d)", bs.name, r,
                 h[4 * r], h[4 * r + 1], h[4 * r + 2] & 0xFFFFFFFFull, h[4 * r + 2] >> 32, rank, (unsigned long long)n, d, k, bs.kind);
        if (h[4 * r + 3] && (!bad || h[4 * r + 3] < bad)) bad = h[4 * r + 3];
    }
    if (bs.kind < 0 || bs.kind > 2) fail(SCANRS_ERR_ARGUMENT, "%s: distance type %d (0 euclidean, 1 pearson, 2 cosine)", bs.check, bs.kind);
    if (k > KMAX) fail(SCANRS_ERR_ARGUMENT, "%s: k must not exceed 128", bs.check);
    if (d == 0 || d > 128) fail(SCANRS_ERR_ARGUMENT, "%s: 1 <= dimensions <= 128", bs.check);
    if (n > 0xFFFFFFFEull) fail(SCANRS_ERR_SHAPE, "%s: too many points for u32 indices", bs.check);
    if (bad) fail(SCANRS_ERR_ARGUMENT, "%s: row %llu of the points holds a coordinate that is not finite", bs.name, bad - 1);
    if (ld < d) fail(SCANRS_ERR_ARGUMENT, "%s: leading dimension smaller than the number of coordinates", bs.check);
    if (k == 0 || n == 0) return;

    // 2. The running lists, sorted, padded with (+inf, UINT32_MAX); two copies: a merge reads one and writes the other.
    const uint64_t n_list = std::max<uint64_t>(1, n_local * k);
    DevBuf<double> rd[2] = {DevBuf<double>(n_list), DevBuf<double>(n_list)}, bdist(n_list);
    DevBuf<uint32_t> ri[2] = {DevBuf<uint32_t>(n_list), DevBuf<uint32_t>(n_list)}, bidx(n_list);
    int cur = 0;
    hipLaunchKernelGGL(ks_fill_kernel, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0, s, rd[0].p, n_list, (double)INFINITY);
    SCANRS_HIP(hipMemsetAsync(ri[0].p, 0xFF, n_list * 4, s));

    // 3. The query side of the filter, once for all blocks - when a block can take the filter at all (the tests of knn_filtered).
    const GlobalOptions &go = global_options();
    const uint64_t block_rows = std::max<uint64_t>(1, go.knn_block_rows);
    const uint64_t largest = std::min(block_rows, n);
    KfQueries qs;
    const bool may_filter =
        !bs.search && !go.knn_exhaustive && d <= KF_DMAX && k <= KF_KMAX && n_local >= KF_NQ_MIN && largest >= go.knn_filter_min_points;
    if (may_filter) kf_prepare_queries(s, d_pts, ld, n_local, d, qs);

    // 4. The blocks. The cut is global, so every rank walks the same blocks and the exchange steps pair up.
    DevBuf<unsigned long long> xbuf(largest * d);
    KnnLastStats stats;
    for (uint64_t b0 = 0; b0 < n; b0 += block_rows) {
        const uint64_t rows = std::min(block_rows, n - b0);
        SCANRS_HIP(hipMemsetAsync(xbuf.p, 0, rows * d * 8, s));
        const uint64_t lo = std::max(b0, begin), hi = std::min(b0 + rows, begin + n_local);
        if (lo < hi)
            hipLaunchKernelGGL(ks_pack_kernel, dim3((unsigned)(((hi - lo) * d + 255) / 256)), dim3(256), 0, s, d_pts + (lo - begin) * ld, ld, d, hi - lo,
                               xbuf.p + (lo - b0) * d);
        ex.sum(xbuf.p, rows * d);
        st.knn_blocks++;
        if (!n_local) continue;
        const double *blk = reinterpret_cast<const double *>(xbuf.p);
        if (st.prof.on) st.prof.begin(s, "knn_search", (double)(rows + n_local) * d * 8.0);
        stats = KnnLastStats();
        if (bs.search) {
            bs.search(s, blk, rows, b0, rd[cur].p + (k - 1), bidx.p, bdist.p, stats);
        } else {
            KnnPlace pl;
            pl.p_off = b0;
            pl.q_off = begin;
            pl.seed = rd[cur].p + (k - 1);
            pl.seed_ld = k;
            pl.queries = may_filter ? &qs : nullptr;
            if (!knn_filtered(s, d_pts, ld, n_local, blk, d, rows, d, k, 1, bidx.p, bdist.p, stats, pl)) {
                stats = KnnLastStats();
                exhaustive(s, d_pts, ld, n_local, blk, d, rows, d, k, 1, bidx.p, 1, b0, begin, bdist.p);
            }
        }
        if (st.prof.on) st.prof.end(s);
        if (st.prof.on) st.prof.begin(s, "knn_merge", (double)n_local * k * 36.0);
        hipLaunchKernelGGL(ks_merge_kernel, dim3((unsigned)((n_local + 3) / 4)), dim3(256), 0, s, n_local, k, rd[cur].p, ri[cur].p, bdist.p, bidx.p,
                           (uint32_t)b0, rd[1 - cur].p, ri[1 - cur].p);
        if (st.prof.on) st.prof.end(s);
        SCANRS_HIP(hipGetLastError());
        cur = 1 - cur;
    }
    if (n_local) {
        if (bs.finish && keys) bs.finish(s, rd[cur].p, n_local * k);
        SCANRS_D2H(out, ri[cur].p, n_local * k * 4, s);
        if (keys) SCANRS_D2H(keys, rd[cur].p, n_local * k * 8, s);
    }
    SCANRS_SYNC(s);
    if (n_local) {
        std::lock_guard<std::mutex> lock(g_stats_mutex);
        g_last_stats = std::move(stats);
    }
}

void knn_sharded(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d, uint32_t k,
                 uint32_t *out, double *sq_dist) {
    knn_sharded_blocks(st, d_pts, ld, begin, n_local, n, d, k, KnnBlockSearch(), out, sq_dist);
}

void knn_host_merge(uint32_t k, const double *da, const uint32_t *ia, const double *db, const uint32_t *ib, double *dout, uint32_t *iout) {
    for (uint32_t e = 0; e < 2u * k; e++) knn_merge::place(k, da, ia, db, ib, e, dout, iout);
}

// queries (n_q x d) against points (n_p x d), both row-major host arrays; out n_q x k.
void knn_host(const double *queries, uint64_t n_q, const double *points, uint64_t n_p, uint32_t d, uint32_t k, bool skip_same_index,
              uint32_t *out) {
    if (k == 0 || n_q == 0) return;
    DevBuf<double> dq, dp;
    const bool same = queries == points && n_q == n_p;
    dp.alloc(n_p * d ? n_p * d : 1);
    if (n_p) SCANRS_HIP(hipMemcpy(dp.p, points, n_p * d * 8, hipMemcpyHostToDevice));
    if (!same) {
        dq.alloc(n_q * d ? n_q * d : 1);
        SCANRS_HIP(hipMemcpy(dq.p, queries, n_q * d * 8, hipMemcpyHostToDevice));
    }
    knn_device(same ? dp.p : dq.p, d, n_q, dp.p, d, n_p, d, k, skip_same_index, out);
}

// scanrs_init(): one empty launch per translation unit makes the runtime load this file's code object now instead of inside the
// first real call
__global__ void warm_knn_kernel() {}
void warm_knn(hipStream_t s) { hipLaunchKernelGGL(warm_knn_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
