// knn_shard.hpp — the walk over a sharded point set that the searches share: knn_sharded (knn.hip, squared
// Euclidean distance) and nearest_neighbors_sharded (knn_metric.hip, Pearson and cosine distance). Every rank owns the queries of
// its own rows; the global rows pass by in blocks of "knn_block_rows" raw rows, one u64 all-reduce each; a block is searched with the
// query's k-th key so far as its seed, and its list is merged into the query's running list by (key, global index). What differs
// between the searches is the key of a pair and therefore how one block is searched: KnnBlockSearch.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <functional>

#include "common.hpp"
#include "knn_filter.hpp"
#include "knn_merge.hpp"

namespace scanrs {

// One search over the blocks. `search` ranks one block (rows x d, leading dimension d, global row b0 first) for the rank's n_local
// queries: block-LOCAL indices and keys, n_local x k, sorted by (key, index), padded with (UINT32_MAX, +inf). seed[q * k] is the k-th
// key query q holds from the blocks before (+inf while it holds fewer than k): a search may drop every pair whose key is not below
// it. Blocks arrive in ascending global index, so such a pair has a larger global index than every entry it could tie with, and the
// merge would drop it too. `finish` turns the running keys (count of them, padding +inf) into what the caller gets.
struct KnnBlockSearch {
    const char *name = "knn_sharded"; // of the entry point, for its refusals
    const char *check = "knn";
    int kind = 0; // travels with k in the first exchange: ranks that differ in it are refused like ranks that differ in k
    std::function<void(hipStream_t s, const double *blk, uint64_t rows, uint64_t b0, const double *seed, uint32_t *bidx, double *bkey,
                       KnnLastStats &stats)>
        search;
    std::function<void(hipStream_t s, double *keys, uint64_t count)> finish;
};
// knn.hip. out / keys: host arrays over the rank's rows, GLOBAL indices. Counts st.knn_blocks / st.knn_allreduces.
void knn_sharded_blocks(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d, uint32_t k,
                        const KnnBlockSearch &bs, uint32_t *out, double *keys);
// knn.hip. The walk with the squared Euclidean search of one block as bs.search (knn_sharded; nearest_neighbors_sharded under
// Euclidean distance, whose `finish` is the square root)
void knn_sharded_euclidean(Storage &st, const double *d_pts, uint32_t ld, uint64_t begin, uint64_t n_local, uint64_t n, uint32_t d, uint32_t k,
                           KnnBlockSearch bs, uint32_t *out, double *keys);

static __global__ void ks_fill_kernel(double *__restrict__ x, uint64_t n, double v) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) x[e] = v;
}
// the first local row that holds a coordinate which is not finite (an integer minimum; ~0 stays when there is none)
static __global__ __launch_bounds__(256) void ks_scan_kernel(const double *__restrict__ X, uint32_t ld, uint64_t n, uint32_t d,
                                                             unsigned long long *__restrict__ first) {
    const uint64_t total = n * d, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const uint64_t r = e / d;
        const double x = X[r * ld + (e % d)];
        if (!(fabs(x) <= DBL_MAX)) atomicMin(first, (unsigned long long)r);
    }
}
// what the ranks agree on before the first block: this rank's four words, n, d, k (the kind of the search above bit 32) and
// (first bad global row + 1)
static __global__ void ks_header_kernel(unsigned long long *__restrict__ mine, uint64_t n, uint32_t d, uint32_t k, int kind, uint64_t begin,
                                        const unsigned long long *__restrict__ first) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    mine[0] = n;
    mine[1] = d;
    mine[2] = (unsigned long long)k | ((unsigned long long)(uint32_t)kind << 32);
    mine[3] = *first == ~0ull ? 0ull : begin + *first + 1ull;
}
// the bit patterns of n_rows rows of this rank into their place of the block buffer (rows x d, no padding)
static __global__ void ks_pack_kernel(const double *__restrict__ src, uint32_t ld, uint32_t d, uint64_t n_rows, unsigned long long *__restrict__ dst) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_rows * d) return;
    dst[e] = (unsigned long long)__double_as_longlong(src[(e / d) * ld + (e % d)]);
}
// running list (+) block list -> running list: one wave per query, both lists staged in LDS (the block's indices become global
// there), every lane places its entries by the rule of knn_merge.hpp. No atomics, nothing that depends on an order of arrival.
static __global__ __launch_bounds__(256) void ks_merge_kernel(uint64_t n_q, uint32_t k, const double *__restrict__ rd, const uint32_t *__restrict__ ri,
                                                              const double *__restrict__ bd, const uint32_t *__restrict__ bi, uint32_t b_off,
                                                              double *__restrict__ od, uint32_t *__restrict__ oi) {
    __shared__ double sd[4][2 * KMAX];
    __shared__ uint32_t si[4][2 * KMAX];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + w;
    const bool live = q < n_q;
    if (live)
        for (uint32_t e = lane; e < k; e += 64u) {
            sd[w][e] = rd[q * k + e];
            si[w][e] = ri[q * k + e];
            const uint32_t t = bi[q * k + e];
            sd[w][KMAX + e] = bd[q * k + e];
            si[w][KMAX + e] = t == 0xFFFFFFFFu ? t : t + b_off;
        }
    __syncthreads();
    if (!live) return;
    for (uint32_t e = lane; e < 2u * k; e += 64u)
        knn_merge::place(k, sd[w], si[w], sd[w] + KMAX, si[w] + KMAX, e, od + q * k, oi + q * k);
}

} // namespace scanrs
