// HIP kernels of merge_clusters (scan-rs/src/merge_clusters.rs) + their launchers. Host logic: cluster_host.cpp.
//
//   medoid_gather_kernel      the scores of a column tile, cells grouped by cluster, as order-preserving u64 keys in column-major
//                             segments (one per cluster and column); the first cell holding a NaN is noted
//   medoid_select_kernel      exact median of each (cluster, column) segment by radix select: 8 rounds of 8-bit digits from the
//                             top, one LDS histogram per wanted rank (⌊(n-1)/2⌋ and ⌊n/2⌋), integer counts only: the result
//                             is the sorted list's element and does not depend on launch timing
//   medoid_dist_*_kernel      the same medians when a segment's cells lie on several ranks: per radix round a local
//                             histogram per (cluster, column, wanted rank), a u64 all-reduce between the kernels, a replicated pick
//   merge_gene_major_kernel   the fused pass of a merge run from the gene-major copy: a wave owns a gene, and a per-wave LDS row
//                             of a tile of clusters gathers Σ x (u64) and Σ x/u_c, Σ (x/u_c)² (128-bit fixed point, u_c the
//                             cell's total) with integer LDS atomics
//   merge_cell_major_kernel   the same sums from the cell-major copy: a wave owns a cell (one cluster), scattered over the genes
//                             with integer global atomics
//
// The output of the fused pass is clusters x genes x 5 u64: [Σ x, Σ x/u lo, hi, Σ (x/u)² lo, hi]. Both orientations add the same
// rounded terms into integers, so they give the same bits; sums of two clusters are an exact integer add on the host.
#include "common.hpp"
#include "fixed128.hpp"

namespace scanrs {

// ---- medoids ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long order_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_order_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// keys[jj * n + pos] = key of scores[perm[pos] * ld + j0 + jj], jj < jt
__global__ __launch_bounds__(256) void medoid_gather_kernel(const double *__restrict__ scores, uint64_t n, uint32_t ld, uint32_t j0, uint32_t jt,
                                                            const uint32_t *__restrict__ perm, unsigned long long *__restrict__ keys,
                                                            unsigned long long *__restrict__ nan_cell) {
    const uint64_t total = n * jt;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t pos = i / jt;
        const uint32_t jj = (uint32_t)(i - pos * jt);
        const uint32_t c = perm[pos];
        const double v = scores[(uint64_t)c * ld + j0 + jj];
        if (isnan(v)) atomicMin(nan_cell, (unsigned long long)c);
        keys[(uint64_t)jj * n + pos] = order_key(v);
    }
}

constexpr uint32_t MEDOID_THREADS = 512;

// block (k, jj): segment keys[jj * n + off[k] .. off[k + 1]]; out[k * ldo + j0 + jj]
__global__ __launch_bounds__(MEDOID_THREADS) void medoid_select_kernel(const unsigned long long *__restrict__ keys, uint64_t n,
                                                                       const uint64_t *__restrict__ off, uint32_t j0, double *__restrict__ out,
                                                                       uint32_t ldo) {
    __shared__ uint32_t hist[2][256];
    __shared__ unsigned long long prefix[2];
    __shared__ uint64_t rank[2];
    const uint32_t k = blockIdx.x, jj = blockIdx.y, tid = threadIdx.x;
    const uint64_t b = off[k], e = off[k + 1], len = e - b;
    if (len == 0) return; // (every cluster has a cell: the host checks)
    const unsigned long long *seg = keys + (uint64_t)jj * n + b;
    if (tid < 2) {
        prefix[tid] = 0ull;
        rank[tid] = tid == 0 ? (len - 1) / 2 : len / 2;
    }
    for (uint32_t i = tid; i < 512; i += blockDim.x) (&hist[0][0])[i] = 0u;
    __syncthreads();
    for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        const unsigned long long p0 = prefix[0], p1 = prefix[1];
        for (uint64_t i = tid; i < len; i += blockDim.x) {
            const unsigned long long key = seg[i];
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            if ((key & hi_mask) == p0) atomicAdd(&hist[0][digit], 1u);
            if ((key & hi_mask) == p1) atomicAdd(&hist[1][digit], 1u);
        }
        __syncthreads();
        // wave h finds the bucket of rank h: lane l holds bins 4l .. 4l+3, an inclusive scan over the lanes
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        if (wave < 2) {
            const uint32_t *hb = hist[wave];
            const uint32_t c0 = hb[4 * lane], c1 = hb[4 * lane + 1], c2 = hb[4 * lane + 2], c3 = hb[4 * lane + 3];
            const uint64_t local = (uint64_t)c0 + c1 + c2 + c3;
            uint64_t incl = local;
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t v = (uint64_t)__shfl_up((long long)incl, o);
                if ((int)lane >= o) incl += v;
            }
            const uint64_t excl = incl - local, r = rank[wave];
            if (excl <= r && r < incl) {
                uint64_t cum = excl;
                uint32_t d = 0;
                if (cum + c0 <= r) {
                    cum += c0;
                    d = 1;
                    if (cum + c1 <= r) {
                        cum += c1;
                        d = 2;
                        if (cum + c2 <= r) {
                            cum += c2;
                            d = 3;
                        }
                    }
                }
                rank[wave] = r - cum;
                prefix[wave] |= (unsigned long long)(4 * lane + d) << shift;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < 512; i += blockDim.x) (&hist[0][0])[i] = 0u;
        __syncthreads();
    }
    if (tid == 0) {
        // median_mut (stats.rs:13-39): xs[len / 2] for an odd length, (xs[len / 2] + xs[len / 2 - 1]) / 2 for an even one
        const double lo = from_order_key(prefix[0]), hi = from_order_key(prefix[1]);
        out[(uint64_t)k * ldo + j0 + jj] = (len & 1) ? hi : (hi + lo) / 2.0;
    }
}

// ---- medoids over shards ---------------------------------------------------------------------------------------------
// The cells of a (cluster, column) segment lie on several ranks, so no workgroup holds a segment alone: a radix round is a local
// histogram (medoid_dist_hist_kernel), a u64 all-reduce of the table on the host's side, and a pick that every rank repeats on the same
// integers (medoid_dist_pick_kernel). Pair p = jj * n_clusters + cluster within a column tile; state[4 p + h] is the prefix of wanted
// rank h (0: ⌊(len-1)/2⌋, 1: ⌊len/2⌋ of the GLOBAL segment), state[4 p + 2 + h] what remains of the rank inside the prefix's bucket.
constexpr uint32_t MEDOID_DIST_THREADS = 256, MEDOID_DIST_WAVES = MEDOID_DIST_THREADS / 64;

__global__ void medoid_dist_init_kernel(const uint64_t *__restrict__ len, uint32_t n_clusters, uint32_t n_pairs, unsigned long long *__restrict__ state) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint64_t l = len[p % n_clusters]; // >= 1: the host checks that every cluster has a cell
    state[4ull * p] = state[4ull * p + 1] = 0ull;
    state[4ull * p + 2] = (l - 1) / 2;
    state[4ull * p + 3] = l / 2;
}

// block b: pair p0 + b; the rank's own part of its segment is keys[jj * n + off[k] .. off[k + 1]). A histogram per wave in LDS (integer
// atomics; waves do not contend for a bin), summed in a fixed order into hist[b * 512 + h * 256 + digit]
__global__ __launch_bounds__(MEDOID_DIST_THREADS) void medoid_dist_hist_kernel(const unsigned long long *__restrict__ keys, uint64_t n,
                                                                               const uint64_t *__restrict__ off, uint32_t n_clusters, uint32_t p0,
                                                                               int shift, const unsigned long long *__restrict__ state,
                                                                               unsigned long long *__restrict__ hist) {
    __shared__ uint32_t h[MEDOID_DIST_WAVES][2][256];
    const uint32_t p = p0 + blockIdx.x, k = p % n_clusters, jj = p / n_clusters, tid = threadIdx.x, wave = tid >> 6;
    for (uint32_t i = tid; i < MEDOID_DIST_WAVES * 512; i += MEDOID_DIST_THREADS) (&h[0][0][0])[i] = 0u;
    __syncthreads();
    const uint64_t b = off[k], len = off[k + 1] - b;
    const unsigned long long *seg = keys + (uint64_t)jj * n + b;
    const unsigned long long hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    const unsigned long long q0 = state[4ull * p], q1 = state[4ull * p + 1];
    for (uint64_t i = tid; i < len; i += MEDOID_DIST_THREADS) {
        const unsigned long long key = seg[i];
        const uint32_t digit = (uint32_t)(key >> shift) & 255u;
        if ((key & hi_mask) == q0) atomicAdd(&h[wave][0][digit], 1u);
        if ((key & hi_mask) == q1) atomicAdd(&h[wave][1][digit], 1u);
    }
    __syncthreads();
    for (uint32_t i = tid; i < 512; i += MEDOID_DIST_THREADS) {
        unsigned long long c = 0ull;
#pragma unroll
        for (uint32_t w = 0; w < MEDOID_DIST_WAVES; w++) c += (&h[w][0][0])[i];
        hist[(uint64_t)blockIdx.x * 512 + i] = c;
    }
}

// block b (two waves): pair p0 + b; wave h finds the bucket of wanted rank h in the reduced histogram, as medoid_select_kernel does
__global__ __launch_bounds__(128) void medoid_dist_pick_kernel(const unsigned long long *__restrict__ hist, uint32_t p0, int shift,
                                                               unsigned long long *__restrict__ state) {
    const uint32_t p = p0 + blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long *hb = hist + (uint64_t)blockIdx.x * 512 + wave * 256;
    const uint64_t c0 = hb[4 * lane], c1 = hb[4 * lane + 1], c2 = hb[4 * lane + 2], c3 = hb[4 * lane + 3];
    const uint64_t local = c0 + c1 + c2 + c3;
    uint64_t incl = local;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t v = (uint64_t)__shfl_up((long long)incl, o);
        if ((int)lane >= o) incl += v;
    }
    const uint64_t excl = incl - local, r = state[4ull * p + 2 + wave];
    if (excl <= r && r < incl) { // exactly one lane: the counts of a prefix's buckets add up to more than the remaining rank
        uint64_t cum = excl;
        uint32_t d = 0;
        if (cum + c0 <= r) {
            cum += c0;
            d = 1;
            if (cum + c1 <= r) {
                cum += c1;
                d = 2;
                if (cum + c2 <= r) {
                    cum += c2;
                    d = 3;
                }
            }
        }
        state[4ull * p + 2 + wave] = r - cum;
        state[4ull * p + wave] |= (unsigned long long)(4 * lane + d) << shift;
    }
}

// after the 8 rounds the prefix is the key itself: median_mut (stats.rs:13-39) as medoid_select_kernel writes it
__global__ void medoid_dist_finish_kernel(const unsigned long long *__restrict__ state, const uint64_t *__restrict__ len, uint32_t n_clusters,
                                          uint32_t n_pairs, uint32_t j0, double *__restrict__ out, uint32_t ldo) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t k = p % n_clusters, jj = p / n_clusters;
    const double lo = from_order_key(state[4ull * p]), hi = from_order_key(state[4ull * p + 1]);
    out[(uint64_t)k * ldo + j0 + jj] = (len[k] & 1) ? hi : (hi + lo) / 2.0;
}

// ---- the fused pass --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void merge_terms(uint32_t x, unsigned long long u, double scale1, double scale2, U128 &t1, U128 &t2) {
    const double t = (double)x / (double)u;
    t1 = to_fixed(t, scale1);
    t2 = to_fixed(t * t, scale2);
}

// clusters [t0, t0 + nt) of the tile; a wave's LDS row: Σ x [nt], Σ x/u [nt][2], Σ (x/u)² [nt][2]
__global__ __launch_bounds__(256) void merge_gene_major_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                               const uint32_t *__restrict__ values, uint64_t n_genes,
                                                               const int16_t *__restrict__ labels, const unsigned long long *__restrict__ tot,
                                                               uint32_t t0, uint32_t nt, double scale1, double scale2,
                                                               unsigned long long *__restrict__ out) {
    extern __shared__ unsigned long long mg_acc[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    unsigned long long *acc = mg_acc + (size_t)wave * nt * 5;
    unsigned long long *ax = acc, *a1 = acc + nt, *a2 = acc + 3 * (size_t)nt;
    for (uint64_t g0 = (uint64_t)blockIdx.x * n_waves; g0 < n_genes; g0 += (uint64_t)gridDim.x * n_waves) {
        const uint64_t g = g0 + wave;
        for (uint32_t j = lane; j < 5 * nt; j += 64) acc[j] = 0ull;
        __syncthreads();
        if (g < n_genes) {
            const uint64_t p0 = indptr[g], p1 = indptr[g + 1];
            for (uint64_t p = p0 + lane; p < p1; p += 64) {
                const uint32_t c = indices[p], x = values[p];
                const uint32_t l = (uint32_t)((int)labels[c] - (int)t0);
                if (l >= nt || x == 0) continue;
                U128 t1, t2;
                merge_terms(x, tot[c], scale1, scale2, t1, t2);
                atomicAdd(&ax[l], (unsigned long long)x);
                atomic_add128(&a1[2 * l], t1);
                atomic_add128(&a2[2 * l], t2);
            }
        }
        __syncthreads();
        if (g < n_genes) {
            for (uint32_t j = lane; j < nt; j += 64) {
                unsigned long long *o = out + ((uint64_t)(t0 + j) * n_genes + g) * 5;
                o[0] = ax[j];
                o[1] = a1[2 * j];
                o[2] = a1[2 * j + 1];
                o[3] = a2[2 * j];
                o[4] = a2[2 * j + 1];
            }
        }
    }
}

// out is zeroed by the launcher
__global__ __launch_bounds__(256) void merge_cell_major_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                               const uint32_t *__restrict__ values, uint64_t n_cells, uint64_t n_genes,
                                                               const int16_t *__restrict__ labels, const unsigned long long *__restrict__ tot,
                                                               double scale1, double scale2, unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = blockDim.x >> 6;
    for (uint64_t c = (uint64_t)blockIdx.x * n_waves + (threadIdx.x >> 6); c < n_cells; c += (uint64_t)gridDim.x * n_waves) {
        const int l = labels[c];
        if (l < 0) continue; // uniform over the wave
        const unsigned long long u = tot[c];
        const uint64_t p0 = indptr[c], p1 = indptr[c + 1];
        for (uint64_t p = p0 + lane; p < p1; p += 64) {
            const uint32_t g = indices[p], x = values[p];
            if (x == 0) continue;
            U128 t1, t2;
            merge_terms(x, u, scale1, scale2, t1, t2);
            unsigned long long *o = out + ((uint64_t)l * n_genes + g) * 5;
            atomicAdd(&o[0], (unsigned long long)x);
            atomic_add128(&o[1], t1);
            atomic_add128(&o[3], t2);
        }
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
static inline uint32_t grid_for(uint64_t items, uint32_t per_block, uint32_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (items + per_block - 1) / per_block));
}

void launch_medoids(hipStream_t s, const double *d_scores, uint64_t n, uint32_t ld, uint32_t d, const uint32_t *d_perm, const uint64_t *d_off,
                    uint32_t n_clusters, unsigned long long *d_keys, uint32_t cols_per_tile, unsigned long long *d_nan_cell, double *d_out) {
    SCANRS_HIP(hipMemsetAsync(d_nan_cell, 0xFF, 8, s));
    for (uint32_t j0 = 0; j0 < d; j0 += cols_per_tile) {
        const uint32_t jt = std::min(cols_per_tile, d - j0);
        hipLaunchKernelGGL(medoid_gather_kernel, dim3(grid_for(n * jt, 256, 65536)), dim3(256), 0, s, d_scores, n, ld, j0, jt, d_perm, d_keys,
                           d_nan_cell);
        hipLaunchKernelGGL(medoid_select_kernel, dim3(n_clusters, jt), dim3(MEDOID_THREADS), 0, s, (const unsigned long long *)d_keys, n, d_off, j0,
                           d_out, d);
        SCANRS_HIP(hipGetLastError());
    }
}

void launch_medoid_keys(hipStream_t s, const double *d_scores, uint64_t n, uint32_t ld, uint32_t j0, uint32_t jt, const uint32_t *d_perm,
                        unsigned long long *d_keys, unsigned long long *d_nan_cell) {
    if (!n || !jt) return;
    hipLaunchKernelGGL(medoid_gather_kernel, dim3(grid_for(n * jt, 256, 65536)), dim3(256), 0, s, d_scores, n, ld, j0, jt, d_perm, d_keys, d_nan_cell);
    SCANRS_HIP(hipGetLastError());
}

void launch_medoid_dist_init(hipStream_t s, const uint64_t *d_len, uint32_t n_clusters, uint32_t jt, unsigned long long *d_state) {
    const uint32_t n_pairs = n_clusters * jt;
    hipLaunchKernelGGL(medoid_dist_init_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, s, d_len, n_clusters, n_pairs, d_state);
    SCANRS_HIP(hipGetLastError());
}

void launch_medoid_dist_hist(hipStream_t s, const unsigned long long *d_keys, uint64_t n, const uint64_t *d_off, uint32_t n_clusters, uint32_t p0,
                             uint32_t np, int shift, const unsigned long long *d_state, unsigned long long *d_hist) {
    hipLaunchKernelGGL(medoid_dist_hist_kernel, dim3(np), dim3(MEDOID_DIST_THREADS), 0, s, d_keys, n, d_off, n_clusters, p0, shift, d_state, d_hist);
    SCANRS_HIP(hipGetLastError());
}

void launch_medoid_dist_pick(hipStream_t s, const unsigned long long *d_hist, uint32_t p0, uint32_t np, int shift, unsigned long long *d_state) {
    hipLaunchKernelGGL(medoid_dist_pick_kernel, dim3(np), dim3(128), 0, s, d_hist, p0, shift, d_state);
    SCANRS_HIP(hipGetLastError());
}

void launch_medoid_dist_finish(hipStream_t s, const unsigned long long *d_state, const uint64_t *d_len, uint32_t n_clusters, uint32_t j0, uint32_t jt,
                               double *d_out, uint32_t ldo) {
    const uint32_t n_pairs = n_clusters * jt;
    hipLaunchKernelGGL(medoid_dist_finish_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, s, d_state, d_len, n_clusters, n_pairs, j0, d_out, ldo);
    SCANRS_HIP(hipGetLastError());
}

uint32_t merge_tile_clusters(uint32_t n_clusters) {
    return std::min<uint32_t>(n_clusters, MERGE_TILE_CLUSTERS);
}

uint32_t launch_merge_pass(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_genes, const int16_t *d_labels,
                           uint32_t n_clusters, const unsigned long long *d_tot, double scale1, double scale2, unsigned long long *d_out) {
    uint32_t passes = 0;
    if (gene_major) {
        // a wave's LDS row holds 5 u64 per cluster of the tile: up to 4 waves per workgroup within 60 KB; more clusters than one
        // row holds are done in tiles, the nonzeros re-read once per tile
        const uint32_t tile = merge_tile_clusters(n_clusters);
        const uint32_t waves = std::max<uint32_t>(1, std::min<uint32_t>(4, MERGE_TILE_CLUSTERS / tile));
        const size_t lds = (size_t)waves * tile * 5 * 8;
        const dim3 grid(grid_for(n_genes, waves, 16384)), block(64 * waves);
        for (uint32_t t0 = 0; t0 < n_clusters; t0 += tile) {
            const uint32_t nt = std::min(tile, n_clusters - t0);
            if (n_genes)
                hipLaunchKernelGGL(merge_gene_major_kernel, grid, block, lds, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, n_genes, d_labels,
                                   d_tot, t0, nt, scale1, scale2, d_out);
            passes++;
        }
    } else {
        SCANRS_HIP(hipMemsetAsync(d_out, 0, std::max<uint64_t>(1, (uint64_t)n_clusters * n_genes) * 40, st.stream));
        if (cp.n_outer)
            hipLaunchKernelGGL(merge_cell_major_kernel, dim3(grid_for(cp.n_outer, 4, 16384)), dim3(256), 0, st.stream, cp.indptr.p, cp.indices.p,
                               cp.values.p, cp.n_outer, n_genes, d_labels, d_tot, scale1, scale2, d_out);
        passes++;
    }
    SCANRS_HIP(hipGetLastError());
    return passes;
}

} // namespace scanrs
