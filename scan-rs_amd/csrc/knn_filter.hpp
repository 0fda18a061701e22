// knn_filter.hpp — the bf16-MFMA filter under the filtered route of knn_search.hpp (knn.hip: squared Euclidean distance;
// knn_metric.hip: Pearson and cosine distance on standardised rows). The derivation of the margin and the kernels themselves are in
// knn.hip; this header holds the filter's constants, the operands of one filtered search, its statistics and the host side of one
// filter pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.hpp"

namespace scanrs {

constexpr uint32_t KMAX = 128; // largest k of every search

constexpr uint32_t KF_DP = 64;     // operand row: 58 coordinates + 6 augmentation slots
constexpr uint32_t KF_DMAX = 58;
constexpr uint32_t KF_CAP = 1024;  // candidates per query and round
constexpr uint32_t KF_KMAX = 64;   // largest k and smallest query count the filter takes
constexpr uint64_t KF_NQ_MIN = 256;
constexpr double KF_GAMMA = 0.00395;
constexpr double KF_COORD_MIN = 0x1p-48, KF_COORD_MAX = 0x1p46; // the magnitude window of max |coordinate|
constexpr float KF_SENTINEL = 1e30f; // N of a sentinel point row, -A of a sentinel query row
constexpr double KF_A_PASS = 9e29;   // A of "everything passes": above every legitimate A, below the sentinel
constexpr uint32_t KF_PER_LANE = KF_CAP / 64u; // candidates a lane of the rerank kernel holds
// Round 0 of a seeded search only tightens a threshold the earlier blocks have set already, and it is paid once per block: its
// exactly ranked subset is a quarter of what an unseeded search ranks, one more filter round in exchange.
constexpr uint64_t KF_SEED_N0 = KF_CAP / 4;

// what the last search of the process did (scanrs_debug_knn_last_stats)
struct KfRound {
    uint64_t stride, points, cand_sum;
    uint32_t cand_max, overflowed;
};
struct KnnLastStats {
    bool filtered = false;
    uint64_t first_stride = 0; // stride of the subset that round 0 ranks exactly
    std::vector<KfRound> rounds;
};
void knn_publish_stats(KnnLastStats &&stats);

// the bf16 operands of one filtered search
// the query side: prepared with the points for one search, or once for all the blocks a sharded search passes by (kf_prepare_queries)
struct KfQueries {
    DevBuf<uint16_t> Qb;
    DevBuf<double> qn;
    uint64_t nq_rows = 0;
    double maxabs = 0.0; // max |coordinate| of the queries (NaN: one of them is not finite)
};
struct KfOperands {
    KfQueries own;
    const KfQueries *q = nullptr; // &own, or the caller's
    DevBuf<uint16_t> Pb;
    double slack = 0.0; // absolute part of the margin, 2^-117 (M + 1)
};
// false: a coordinate is not finite or max |coordinate| lies outside the magnitude window; nothing has been prepared.
// shared: the query side prepared earlier by kf_prepare_queries (nullptr: it is prepared here)
bool kf_prepare(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, const double *dp, uint32_t ldp, uint64_t n_p, uint32_t d,
                KfOperands &op, const KfQueries *shared = nullptr);
// the query side alone, for a search whose points arrive in blocks: its max-abs pass and its operands are made once
void kf_prepare_queries(hipStream_t s, const double *dq, uint32_t ldq, uint64_t n_q, uint32_t d, KfQueries &qs);
// one pass of the filter over rows 0, st, 2 st, ... of the points with the thresholds tau: cnt (n_q) and the lists cand (n_q x KF_CAP).
// Every point whose fma-chain squared distance to the query is <= tau[q] is in the query's list (or the list has overflowed).
void kf_filter_pass(hipStream_t s, const KfOperands &op, const double *tau, uint64_t n_q, uint64_t n_p, uint64_t st, uint32_t *cand,
                    uint32_t *cnt);

// The copies of a search. The entry points on stream 0 keep the blocking copies they have always made; a search on a handle's own
// (non-blocking) stream queues them there and waits for that stream alone, bounded like every wait of the library.
void kf_d2h(hipStream_t s, void *dst, const void *src, size_t bytes);
void kf_h2d(hipStream_t s, void *dst, const void *src, size_t bytes);

// round 0: every query's candidate list = the whole coarsest subset (rows 0, stride, 2 stride, ...), ranked exactly by the rerank kernel
static __global__ void kf_fill_all_kernel(uint64_t n_q, uint32_t n_sub, uint64_t stride, uint32_t *__restrict__ cand, uint32_t *__restrict__ cnt) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_q * n_sub) return;
    const uint64_t q = e / n_sub;
    const uint32_t j = (uint32_t)(e % n_sub);
    cand[q * KF_CAP + j] = (uint32_t)(j * stride);
    if (j == 0) cnt[q] = n_sub;
}

// the search of scanrs_knn_device with the result left in device memory (d_out n_q x k, d_sq n_q x k or nullptr); records the stats
void knn_device_into(const double *d_queries, uint32_t ld_q, uint64_t n_q, const double *d_points, uint32_t ld_p, uint64_t n_p, uint32_t d,
                     uint32_t k, bool skip_same_index, uint32_t *d_out, double *d_sq);

} // namespace scanrs
