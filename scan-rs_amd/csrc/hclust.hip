// HIP kernels of hclust (hclust/src/lib.rs:132-148 with kodama's linkage) + their launchers. Host logic: hclust_host.cpp.
//
//   hclust_pack_kernel     the observations as a compact n x d array (rows of x, or its columns; any leading dimension), and the
//                          first element that is not finite (an integer minimum)
//   hclust_pdist_kernel    the full symmetric n x n matrix: a workgroup owns a 64 x 64 tile of the upper triangle, stages the two
//                          sets of observation rows in LDS 32 dimensions at a time, and writes the tile and its mirror. Each
//                          squared distance is Σ_k (b_k - a_k)² over k in order, multiply and add rounded separately (hclust_lw.hpp)
//   hclust_scan_kernel     one chain step's decision, ONE workgroup: the row of the chain's top is scanned over the active
//                          clusters for the smallest dissimilarity (the previous element first, then the smallest index); the
//                          step merges (record, pop two, keep the higher index, retire the other) or pushes
//   hclust_update_kernel   the Lance-Williams update of the kept cluster's row and mirror column, many workgroups; returns at
//                          once when the step was a push
//
// No workgroup waits for another inside a launch: a step is two plain launches on one stream, and the state (chain, sizes, merge
// list, counters) lives in device memory, so the host enqueues steps without reading any of it. No floating-point atomics.
#include "common.hpp"
#include "hclust_lw.hpp"

namespace scanrs {

// ---- the observations ---------------------------------------------------------------------------------------------------------
// out[i * d + k] = observation i's k-th coordinate: x[i * ld + k] (by_cols == 0) or x[k * ld + i]; bad = the smallest row-major
// position (row * cols + col of x as given) of an element that is NaN or infinite
__global__ __launch_bounds__(256) void hclust_pack_kernel(const double *__restrict__ x, uint64_t n, uint32_t d, uint64_t ld, int by_cols,
                                                          double *__restrict__ out, unsigned long long *__restrict__ bad) {
    const uint64_t total = n * d;
    const uint64_t cols = by_cols ? n : d;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
        // e walks x in its own row-major order (coalesced reads)
        const uint64_t r = e / cols, c = e - r * cols;
        const double v = x[r * ld + c];
        if (!isfinite(v)) atomicMin(bad, (unsigned long long)e);
        const uint64_t i = by_cols ? c : r, k = by_cols ? r : c;
        out[i * d + k] = v;
    }
}

// ---- the distance pass -------------------------------------------------------------------------------------------------------
constexpr uint32_t PD_TILE = 64; // observations per side of a workgroup's tile (256 threads, 4 x 4 results each)
constexpr uint32_t PD_KC = 32;   // dimensions staged at a time: 2 x 32 x 65 x 8 B = 33 KB of LDS
constexpr uint32_t PD_LD = PD_TILE + 1;

// bad_pair (may be null) = the smallest i * n + j, i < j, of a distance that is not finite: finite coordinates whose squared
// differences overflow
__global__ __launch_bounds__(256) void hclust_pdist_kernel(const double *__restrict__ obs, uint64_t n, uint32_t d, int squared,
                                                           double *__restrict__ dist, unsigned long long *__restrict__ bad_pair) {
    const uint32_t bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return; // the upper triangle's tiles write their mirrors
    __shared__ double As[PD_KC][PD_LD], Bs[PD_KC][PD_LD];
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint64_t i0 = (uint64_t)bi * PD_TILE, j0 = (uint64_t)bj * PD_TILE;
    double s[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) s[r][c] = 0.0;
    for (uint32_t k0 = 0; k0 < d; k0 += PD_KC) {
        const uint32_t kc = min(PD_KC, d - k0);
        for (uint32_t e = tid; e < PD_TILE * PD_KC; e += 256) {
            const uint32_t row = e / PD_KC, kk = e % PD_KC;
            const uint64_t gi = i0 + row, gj = j0 + row;
            As[kk][row] = (gi < n && kk < kc) ? obs[gi * d + k0 + kk] : 0.0;
            Bs[kk][row] = (gj < n && kk < kc) ? obs[gj * d + k0 + kk] : 0.0;
        }
        __syncthreads();
        for (uint32_t kk = 0; kk < kc; kk++) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) a[r] = As[kk][ty * 4 + r];
#pragma unroll
            for (int c = 0; c < 4; c++) b[c] = Bs[kk][tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const double t = b[c] - a[r];
                    const double q = t * t; // (contraction is off: hclust_lw.hpp)
                    s[r][c] = s[r][c] + q;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint64_t i = i0 + ty * 4 + r;
        if (i >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint64_t j = j0 + tx * 4 + c;
            if (j >= n) continue;
            const double v = squared ? s[r][c] : sqrt(s[r][c]);
            dist[i * n + j] = v;
            dist[j * n + i] = v;
            if (bad_pair && !isfinite(v)) atomicMin(bad_pair, (unsigned long long)(i < j ? i * n + j : j * n + i));
        }
    }
}

// ---- the chain ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t SCAN_THREADS = 1024;

__device__ __forceinline__ void best_of(double &v, uint32_t &c, double ov, uint32_t oc) {
    if (hclust_better(ov, oc, v, c)) {
        v = ov;
        c = oc;
    }
}

// the (value, index) minimum of a workgroup under hclust_better; every thread returns it
__device__ void block_best(double &v, uint32_t &c, double *sh_v, uint32_t *sh_c) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off, 64);
        const uint32_t oc = __shfl_down(c, off, 64);
        best_of(v, c, ov, oc);
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads(); // (the previous use of sh_* is over)
    if (lane == 0) {
        sh_v[wave] = v;
        sh_c[wave] = c;
    }
    __syncthreads();
    v = sh_v[0];
    c = sh_c[0];
    for (uint32_t w = 1; w < SCAN_THREADS / 64; w++) best_of(v, c, sh_v[w], sh_c[w]);
}

// One step. State: chain[n], size[n] (0: retired), ctr = {chain length, merges, steps, error}, rec = {merged, a, b, size a, size b}
// of this step for the update kernel, the merge list in discovery order. error: 1 = a Lance-Williams update gave a value that is
// not finite (hclust_update_kernel), 2 = a scan found no finite candidate; once it is set every later step returns at once, so no
// index that a poisoned row could yield is ever pushed or dereferenced.
__global__ __launch_bounds__(SCAN_THREADS) void hclust_scan_kernel(const double *__restrict__ dist, uint32_t n, uint32_t *__restrict__ chain,
                                                                   uint32_t *__restrict__ size, unsigned long long *__restrict__ ctr,
                                                                   uint32_t *__restrict__ rec, uint32_t *__restrict__ m_a,
                                                                   uint32_t *__restrict__ m_b, double *__restrict__ m_h,
                                                                   uint32_t *__restrict__ m_size) {
    __shared__ double sh_v[SCAN_THREADS / 64];
    __shared__ uint32_t sh_c[SCAN_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    const unsigned long long merges = ctr[1];
    uint32_t len = (uint32_t)ctr[0];
    if (merges + 1 >= n || ctr[3] != 0) { // finished or failed: steps queued behind do nothing
        if (tid == 0) rec[0] = 0;
        return;
    }
    uint32_t a;
    if (len == 0) { // a new chain starts at the lowest active cluster
        double v = 0.0;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t j = tid; j < n; j += SCAN_THREADS)
            if (size[j] != 0 && j < c) c = j;
        block_best(v, c, sh_v, sh_c);
        if (c == 0xFFFFFFFFu) { // (no active cluster: cannot happen while merges are left)
            if (tid == 0) {
                ctr[3] = 2;
                rec[0] = 0;
            }
            return;
        }
        a = c;
        len = 1;
    } else {
        a = chain[len - 1];
    }
    const double *row = dist + (uint64_t)a * n;
    double v = INFINITY;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t j = tid; j < n; j += SCAN_THREADS) {
        if (j == a || size[j] == 0) continue;
        best_of(v, c, row[j], j);
    }
    block_best(v, c, sh_v, sh_c);
    if (tid != 0) return;
    // (every thread has read ctr, chain and size: all of them passed the barriers of block_best before thread 0 got here)
    ctr[2] += 1;
    if (c == 0xFFFFFFFFu || !isfinite(v)) { // a row without a finite entry: nothing is pushed, the host reports it
        ctr[3] = 2;
        rec[0] = 0;
        return;
    }
    const uint32_t prev = len > 1 ? chain[len - 2] : 0xFFFFFFFFu;
    if (len > 1 && !(v < row[prev])) c = prev; // the previous element wins when it attains the minimum
    if (len > 1 && c == prev) {
        const uint32_t lo = a < c ? a : c, hi = a < c ? c : a;
        const uint32_t sl = size[lo], sh = size[hi];
        m_a[merges] = lo;
        m_b[merges] = hi;
        m_h[merges] = row[prev];
        m_size[merges] = sl + sh;
        size[lo] = 0;
        size[hi] = sl + sh;
        rec[0] = 1;
        rec[1] = lo;
        rec[2] = hi;
        rec[3] = sl;
        rec[4] = sh;
        ctr[0] = len - 2;
        ctr[1] = merges + 1;
    } else {
        if (len == 1) chain[0] = a;
        chain[len] = c;
        rec[0] = 0;
        ctr[0] = len + 1;
    }
}

// rec = {merged, a, b, size a, size b}: clusters a (retired) and b (kept, now a ∪ b); every other active cluster k gets its new
// dissimilarity to b in row b and in its own row's column b. Row a and row b still hold the values from before the merge.
__global__ __launch_bounds__(256) void hclust_update_kernel(double *__restrict__ dist, uint32_t n, int method, const uint32_t *__restrict__ size,
                                                            const uint32_t *__restrict__ rec, unsigned long long *__restrict__ ctr) {
    if (rec[0] == 0) return;
    const uint32_t a = rec[1], b = rec[2];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n || k == a || k == b) return;
    const uint32_t sk = size[k];
    if (sk == 0) return;
    const double dab = dist[(uint64_t)a * n + b];
    const double dka = dist[(uint64_t)a * n + k], dkb = dist[(uint64_t)b * n + k];
    const double v = hclust_lw(method, dka, dkb, dab, (double)rec[3], (double)rec[4], (double)sk);
    dist[(uint64_t)b * n + k] = v;
    dist[(uint64_t)k * n + b] = v;
    if (!isfinite(v)) atomicMax(&ctr[3], 1ull); // the update overflowed: the chain stops at its next step
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
void launch_hclust_pack(hipStream_t s, const double *d_x, uint64_t n, uint32_t d, uint64_t ld, int by_cols, double *d_obs, unsigned long long *d_bad) {
    SCANRS_HIP(hipMemsetAsync(d_bad, 0xFF, 8, s));
    const uint64_t total = n * d;
    if (!total) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(hclust_pack_kernel, dim3(blocks), dim3(256), 0, s, d_x, n, d, ld, by_cols, d_obs, d_bad);
    SCANRS_HIP(hipGetLastError());
}
void launch_hclust_pdist(hipStream_t s, const double *d_obs, uint64_t n, uint32_t d, int squared, double *d_dist, unsigned long long *d_bad_pair) {
    if (d_bad_pair) SCANRS_HIP(hipMemsetAsync(d_bad_pair, 0xFF, 8, s));
    const uint32_t nb = (uint32_t)((n + PD_TILE - 1) / PD_TILE);
    hipLaunchKernelGGL(hclust_pdist_kernel, dim3(nb, nb), dim3(256), 0, s, d_obs, n, d, squared, d_dist, d_bad_pair);
    SCANRS_HIP(hipGetLastError());
}
void launch_hclust_step(hipStream_t s, double *d_dist, uint32_t n, int method, uint32_t *d_chain, uint32_t *d_size, unsigned long long *d_ctr,
                        uint32_t *d_rec, uint32_t *d_ma, uint32_t *d_mb, double *d_mh, uint32_t *d_msize) {
    hipLaunchKernelGGL(hclust_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, d_dist, n, d_chain, d_size, d_ctr, d_rec, d_ma, d_mb, d_mh, d_msize);
    hipLaunchKernelGGL(hclust_update_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_dist, n, method, d_size, d_rec, d_ctr);
}

} // namespace scanrs
