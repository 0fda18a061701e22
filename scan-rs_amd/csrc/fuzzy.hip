// fuzzy.hip — fuzzy_simplicial_set (umap-rs/src/fuzzy.rs:30-181) and the pruned edge list of
// initialize_simplicial_set_embedding (embedding.rs:29-54, 75-85, up to but not including the shuffle) on the device. DESIGN.md §7r.
// The arithmetic is fuzzy.hpp's, shared with the host twin (fuzzy_host.cpp) and built with -ffp-contract=off: the device equals the
// twin in every bit of every output. No float atomics anywhere; the only atomic is one 64-bit integer minimum that names the first
// refused row.
//
// The chain over lists in device memory (n x k, leading dimension ld):
//  1. fz_check_kernel, one thread per entry: a NaN distance, an index that is neither < n nor UINT32_MAX, an index a row names twice.
//     The reference's TriMat would ADD duplicates (sprs sums repeated triplets), but nothing in the reference produces them - a
//     neighbour list names a row once - so they are refused, like the rows where the reference panics.
//  2. fz_row_kernel, one lane per row: rho, the bisection of smooth_knn_dist, the row's left fold and the floor of rows with rho > 0.
//     A row's folds are sequential by contract, so the parallelism is across rows. Lanes reading row-major rows directly would stride
//     by k * 8 bytes: a wave's 64 rows are staged through LDS with one coalesced read and an odd row pitch (k | 1 doubles), so the 64
//     lanes reading column j fall into different banks. One wave per workgroup: 64 x 129 x 8 B = 66 KB at k = 128, within the 160 KiB
//     of a CU. A wave runs as long as its slowest row (n_iter at most).
//  3. fz_tree_kernel: the row folds summed in the fixed tree of fz_tree_host (the stated deviation from the reference's sequential
//     global mean; it reaches only sigma of rows whose rho is not > 0).
//  4. fz_entries_kernel, one thread per entry: the floor of the remaining rows, the membership strength, and the directed entries
//     keyed (row << 32 | col): R's (row = the neighbour, col = i) first, then R^T's. Padding (UINT32_MAX) gets the key ~0.
//  5. One stable radix sort of the keys with the value as payload (rocPRIM). Equal keys are adjacent and there are at most two, R's
//     first; the union is symmetric in its operands. fz_head_kernel flags the first of each run, a scan places them, fz_fill_kernel
//     writes indices and values, fz_indptr_kernel finds each row's start by bisection of the sorted keys. Positions depend on the keys
//     alone. Zeros are stored like any other value.
// Edges: a maximum (order-free: no NaN survives fz_max, and a tie of +-0 is not observable), the keep flags, a scan, an ordered
// compaction, epochs_per_sample.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "fuzzy_graph.hpp"

namespace scanrs {

using namespace fuzzy;

namespace {

typedef unsigned long long u64;

struct LdsRow {
    const double *p;
    __host__ __device__ double operator()(uint32_t j) const { return p[j]; }
};
struct FzMaxOp {
    __host__ __device__ double operator()(double a, double b) const { return fz_max(a, b); }
};

__global__ __launch_bounds__(256) void fz_check_kernel(const uint32_t *__restrict__ idx, const double *__restrict__ dist, u64 n, uint32_t ld,
                                                       uint32_t k, u64 *__restrict__ bad) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * k) return;
    const u64 i = e / k;
    const uint32_t j = (uint32_t)(e - i * k);
    const double v = dist[i * ld + j];
    const uint32_t c = idx[i * ld + j];
    int kind = 4;
    if (v != v) kind = FZ_BAD_NAN;
    if (c != FZ_NO_INDEX) {
        if (c >= n) kind = min(kind, (int)FZ_BAD_INDEX);
        for (uint32_t j2 = 0; j2 < j; j2++)
            if (idx[i * ld + j2] == c) kind = min(kind, (int)FZ_BAD_REPEAT);
    }
    if (kind < 4) atomicMin(bad, i * 4ull + (u64)kind);
}

// 64 threads = one wave = 64 rows; dynamic LDS: 64 * (k | 1) doubles
__global__ __launch_bounds__(64) void fz_row_kernel(const double *__restrict__ dist, u64 n, uint32_t ld, uint32_t k, double local_connectivity,
                                                    double target, uint32_t n_iter, double *__restrict__ rho_out, double *__restrict__ sigma_out,
                                                    double *__restrict__ fold_out, u64 *__restrict__ bad) {
    extern __shared__ double fz_rows[];
    const uint32_t pitch = k | 1u;
    const u64 row0 = (u64)blockIdx.x * 64;
    for (uint32_t e = threadIdx.x; e < 64u * k; e += 64u) {
        const uint32_t r = e / k, j = e - r * k;
        if (row0 + r < n) fz_rows[r * pitch + j] = dist[(row0 + r) * ld + j];
    }
    __syncthreads();
    const u64 i = row0 + threadIdx.x;
    if (i >= n) return;
    const LdsRow row{fz_rows + threadIdx.x * pitch};
    double rho = 0.0, sigma = 0.0, fold = 0.0;
    if (fz_rho(row, k, local_connectivity, &rho)) {
        sigma = fz_smooth_knn_dist(row, k, rho, target, n_iter, nullptr);
        fold = fz_row_fold(row, k);
        if (rho > 0.0) sigma = fz_floor_row(sigma, fold, k);
    } else {
        atomicMin(bad, i * 4ull + (u64)FZ_BAD_RHO);
    }
    rho_out[i] = rho;
    sigma_out[i] = sigma;
    fold_out[i] = fold;
}

// one level of the tree of fz_tree_host
__global__ __launch_bounds__(256) void fz_tree_kernel(const double *__restrict__ in, u64 m, double *__restrict__ out) {
    __shared__ double a[FZ_TREE];
    const u64 e = (u64)blockIdx.x * FZ_TREE + threadIdx.x;
    a[threadIdx.x] = e < m ? in[e] : 0.0;
    __syncthreads();
    for (uint32_t s = FZ_TREE / 2; s >= 1; s >>= 1) {
        if (threadIdx.x < s) a[threadIdx.x] = a[threadIdx.x] + a[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = a[0];
}

__global__ __launch_bounds__(256) void fz_entries_kernel(const uint32_t *__restrict__ idx, const double *__restrict__ dist, u64 n, uint32_t ld,
                                                         uint32_t k, const double *__restrict__ rho, const double *__restrict__ sigma_pre,
                                                         const double *__restrict__ total, int combine, u64 *__restrict__ keys,
                                                         double *__restrict__ vals, double *__restrict__ sigma_out) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 nk = n * k;
    if (e >= nk) return;
    const u64 i = e / k;
    const uint32_t j = (uint32_t)(e - i * k);
    const double r = rho[i];
    double s = sigma_pre[i];
    if (!(r > 0.0)) s = fz_floor_global(s, total[0], n, k);
    if (j == 0) sigma_out[i] = s;
    const uint32_t c = idx[i * ld + j];
    u64 key = ~0ull, key_t = ~0ull;
    double v = 0.0;
    if (c != FZ_NO_INDEX) {
        v = fz_membership(j, c, dist[i * ld + j], r, s);
        key = ((u64)c << 32) | i; // R[index, i] (fuzzy.rs:173-175)
        key_t = (i << 32) | (u64)c;
    }
    keys[e] = key, vals[e] = v;
    if (combine) keys[nk + e] = key_t, vals[nk + e] = v;
}

__device__ __forceinline__ bool fz_is_head(const u64 *keys, u64 e) { return keys[e] != ~0ull && (e == 0 || keys[e] != keys[e - 1]); }

// pos has m + 1 entries; the last one is 0 so that the exclusive scan leaves the total there
__global__ __launch_bounds__(256) void fz_head_kernel(const u64 *__restrict__ keys, u64 m, u64 *__restrict__ pos) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e > m) return;
    pos[e] = (e < m && fz_is_head(keys, e)) ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void fz_fill_kernel(const u64 *__restrict__ keys, const double *__restrict__ vals, u64 m,
                                                      const u64 *__restrict__ pos, int combine, double ratio, uint32_t *__restrict__ indices,
                                                      double *__restrict__ values) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e >= m || !fz_is_head(keys, e)) return;
    const u64 p = pos[e];
    double v = vals[e];
    if (combine) v = fz_union(v, (e + 1 < m && keys[e + 1] == keys[e]) ? vals[e + 1] : 0.0, ratio);
    indices[p] = (uint32_t)(keys[e] & 0xFFFFFFFFull);
    values[p] = v;
}

// indptr[r] = the number of distinct keys whose row is < r: the place of the first sorted key >= (r << 32)
__global__ __launch_bounds__(256) void fz_indptr_kernel(const u64 *__restrict__ keys, u64 m, const u64 *__restrict__ pos, u64 n,
                                                        u64 *__restrict__ indptr) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    const u64 want = r << 32;
    u64 lo = 0, hi = m;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (keys[mid] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    indptr[r] = pos[lo];
}

// ---- edges ----
__global__ __launch_bounds__(256) void fz_keep_kernel(const double *__restrict__ values, u64 nnz, double threshold, u64 *__restrict__ pos,
                                                      double *__restrict__ kept) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e > nnz) return;
    const bool keep = e < nnz && fz_edge_kept(values[e], threshold);
    pos[e] = keep ? 1ull : 0ull;
    if (e < nnz) kept[e] = keep ? values[e] : -DBL_MAX; // the start of the reference's fold (Q::MIN) changes no maximum
}
__global__ __launch_bounds__(256) void fz_edges_kernel(const u64 *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                       const double *__restrict__ values, u64 n, u64 nnz, double threshold,
                                                       const u64 *__restrict__ pos, const double *__restrict__ max_w, double n_epochs,
                                                       uint32_t *__restrict__ head, uint32_t *__restrict__ tail, double *__restrict__ weights,
                                                       double *__restrict__ eps) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const double v = values[e];
    if (!fz_edge_kept(v, threshold)) return;
    // the row of entry e: the last r with indptr[r] <= e
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (indptr[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    const u64 p = pos[e];
    tail[p] = (uint32_t)lo;
    head[p] = indices[e];
    weights[p] = v;
    eps[p] = fz_epochs_per_sample(v, max_w[0], n_epochs);
}

unsigned grid_of(u64 count) { return (unsigned)((count + 255) / 256); }

// SCANRS_TRACE=1: the wall time of every stage (the stream is waited for at its end) and the bytes its code reads and writes, on stderr
// (tools/fuzzy_bench.py reads these lines). Without tracing nothing is waited for and nothing is printed.
struct StageClock {
    hipStream_t s;
    std::chrono::steady_clock::time_point t0;
    explicit StageClock(hipStream_t stream) : s(stream) {
        if (trace_on()) {
            SCANRS_SYNC(s);
            t0 = std::chrono::steady_clock::now();
        }
    }
    void done(const char *stage, double bytes) {
        if (!trace_on()) return;
        SCANRS_SYNC(s);
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        fprintf(stderr, "[scanrs trace] fuzzy stage %-8s %9.3f ms %14.0f bytes %8.1f GB/s\n", stage, ms, bytes, bytes / (ms * 1e6));
        t0 = std::chrono::steady_clock::now();
    }
};

void scan_in_place(hipStream_t s, u64 *d, size_t count) {
    size_t bytes = 0;
    SCANRS_HIP(rocprim::exclusive_scan(nullptr, bytes, d, d, 0ull, count, rocprim::plus<u64>(), s));
    DevBuf<char> tmp(std::max<size_t>(bytes, 8));
    SCANRS_HIP(rocprim::exclusive_scan(tmp.p, bytes, d, d, 0ull, count, rocprim::plus<u64>(), s));
    SCANRS_SYNC(s); // tmp is released on return
}
void max_of(hipStream_t s, const double *d, size_t count, double start, double *d_out) {
    size_t bytes = 0;
    SCANRS_HIP(rocprim::reduce(nullptr, bytes, d, d_out, start, count, FzMaxOp(), s));
    DevBuf<char> tmp(std::max<size_t>(bytes, 8));
    SCANRS_HIP(rocprim::reduce(tmp.p, bytes, d, d_out, start, count, FzMaxOp(), s));
    SCANRS_SYNC(s);
}

} // namespace

void fuzzy_device(const char *name, const uint32_t *d_idx, const double *d_dist, uint64_t n, uint32_t ld, uint32_t k, const FuzzyParams &P,
                  scanrs_graph &g) {
    hipStream_t s = 0;
    const u64 nk = n * k;
    DevBuf<u64> bad(1);
    SCANRS_HIP(hipMemsetAsync(bad.p, 0xFF, 8, s));
    StageClock clock(s);
    hipLaunchKernelGGL(fz_check_kernel, dim3(grid_of(nk)), dim3(256), 0, s, d_idx, d_dist, n, ld, k, bad.p);
    SCANRS_HIP(hipGetLastError());
    clock.done("check", 12.0 * nk); // the repeat test reads a row's indices again, from the cache
    DevBuf<double> rho(n), sigma_pre(n), fold(n);
    const size_t lds = (size_t)64 * (k | 1u) * 8;
    if (lds > 64 * 1024) SCANRS_HIP(hipFuncSetAttribute((const void *)fz_row_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fz_row_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, d_dist, n, ld, k, P.local_connectivity, P.target, P.n_iter,
                       rho.p, sigma_pre.p, fold.p, bad.p);
    SCANRS_HIP(hipGetLastError());
    clock.done("rows", 8.0 * nk + 24.0 * n);
    fuzzy_refuse_row(name, SCANRS_D2H_VALUE(bad.p, s));
    // the tree over the row folds: levels of FZ_TREE-wide nodes until one is left
    DevBuf<double> lvl_a((n + FZ_TREE - 1) / FZ_TREE), lvl_b(((n + FZ_TREE - 1) / FZ_TREE + FZ_TREE - 1) / FZ_TREE);
    const double *src = fold.p;
    double *dst = lvl_a.p, *other = lvl_b.p;
    for (u64 m = n;;) {
        const u64 nodes = (m + FZ_TREE - 1) / FZ_TREE;
        hipLaunchKernelGGL(fz_tree_kernel, dim3((unsigned)nodes), dim3(FZ_TREE), 0, s, src, m, dst);
        SCANRS_HIP(hipGetLastError());
        src = dst;
        std::swap(dst, other);
        m = nodes;
        if (m == 1) break;
    }
    const double *total = src;
    clock.done("tree", 8.0 * n);
    const u64 m = P.combine ? 2 * nk : nk;
    DevBuf<u64> keys_a(m), keys_b(m);
    DevBuf<double> vals_a(m), vals_b(m);
    DevBuf<double> sigmas(n);
    hipLaunchKernelGGL(fz_entries_kernel, dim3(grid_of(nk)), dim3(256), 0, s, d_idx, d_dist, n, ld, k, rho.p, sigma_pre.p, total, P.combine ? 1 : 0,
                       keys_a.p, vals_a.p, sigmas.p);
    SCANRS_HIP(hipGetLastError());
    clock.done("entries", 12.0 * nk + 16.0 * n + 16.0 * m + 8.0 * n);
    {
        // rows and columns are < n: the bits above 32 + bits(n - 1) are zero in every key but the padding's, which stays the largest
        unsigned end_bit = 33;
        while (end_bit < 64 && ((n - 1) >> (end_bit - 32)) != 0) end_bit++;
        size_t bytes = 0;
        SCANRS_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (size_t)m, 0u, end_bit, s));
        DevBuf<char> tmp(std::max<size_t>(bytes, 8));
        SCANRS_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (size_t)m, 0u, end_bit, s));
        SCANRS_SYNC(s); // tmp is released on leaving this block
        clock.done("sort", 32.0 * m * ((end_bit + 7) / 8)); // keys and values in and out, once per 8-bit digit at the least
    }
    keys_a.release(), vals_a.release();
    DevBuf<u64> pos(m + 1);
    hipLaunchKernelGGL(fz_head_kernel, dim3(grid_of(m + 1)), dim3(256), 0, s, keys_b.p, m, pos.p);
    SCANRS_HIP(hipGetLastError());
    scan_in_place(s, pos.p, (size_t)m + 1);
    const u64 nnz = SCANRS_D2H_VALUE(pos.p + m, s);
    clock.done("place", 8.0 * m + 8.0 * (m + 1) + 16.0 * (m + 1)); // the flags, then the scan in and out
    g.d_indptr.alloc(n + 1);
    g.d_indices.alloc(std::max<u64>(nnz, 1));
    g.d_values.alloc(std::max<u64>(nnz, 1));
    hipLaunchKernelGGL(fz_fill_kernel, dim3(grid_of(m)), dim3(256), 0, s, keys_b.p, vals_b.p, m, pos.p, P.combine ? 1 : 0, P.set_op_mix_ratio,
                       g.d_indices.p, g.d_values.p);
    SCANRS_HIP(hipGetLastError());
    hipLaunchKernelGGL(fz_indptr_kernel, dim3(grid_of(n + 1)), dim3(256), 0, s, keys_b.p, m, pos.p, n, g.d_indptr.p);
    SCANRS_HIP(hipGetLastError());
    SCANRS_SYNC(s); // the scratch buffers are released on return
    clock.done("fill", 24.0 * m + 12.0 * nnz + 8.0 * (n + 1)); // keys, values, places in; indices, values, indptr out (the bisection hits the cache)
    g.n = n, g.nnz = nnz, g.k = k, g.on_device = true;
    g.d_sigmas = std::move(sigmas);
    g.d_rhos = std::move(rho);
}

void fuzzy_edges_device(const scanrs_graph &g, double n_epochs, uint64_t *count, uint32_t *head, uint32_t *tail, double *weights,
                        double *epochs_per_sample) {
    hipStream_t s = 0;
    *count = 0;
    if (g.nnz == 0) return;
    DevBuf<double> mx(2);
    max_of(s, g.d_values.p, (size_t)g.nnz, 0.0, mx.p); // embedding.rs:38: folded from 0.0
    const double threshold = SCANRS_D2H_VALUE(mx.p, s) / n_epochs;
    DevBuf<u64> pos(g.nnz + 1);
    DevBuf<double> kept(g.nnz);
    hipLaunchKernelGGL(fz_keep_kernel, dim3(grid_of(g.nnz + 1)), dim3(256), 0, s, g.d_values.p, g.nnz, threshold, pos.p, kept.p);
    SCANRS_HIP(hipGetLastError());
    scan_in_place(s, pos.p, (size_t)g.nnz + 1);
    const u64 m = SCANRS_D2H_VALUE(pos.p + g.nnz, s);
    *count = m;
    if (!weights || m == 0) return;
    max_of(s, kept.p, (size_t)g.nnz, -DBL_MAX, mx.p + 1);
    DevBuf<uint32_t> dh(m), dt(m);
    DevBuf<double> dw(m), de(m);
    hipLaunchKernelGGL(fz_edges_kernel, dim3(grid_of(g.nnz)), dim3(256), 0, s, g.d_indptr.p, g.d_indices.p, g.d_values.p, g.n, g.nnz, threshold, pos.p,
                       mx.p + 1, n_epochs, dh.p, dt.p, dw.p, de.p);
    SCANRS_HIP(hipGetLastError());
    SCANRS_D2H(head, dh.p, m * 4, s);
    SCANRS_D2H(tail, dt.p, m * 4, s);
    SCANRS_D2H(weights, dw.p, m * 8, s);
    SCANRS_D2H(epochs_per_sample, de.p, m * 8, s);
}

} // namespace scanrs
