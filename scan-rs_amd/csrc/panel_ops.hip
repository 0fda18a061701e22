// Dense panel utilities of the solvers for gfx950 (MI355X) + their launchers (they stand where the reference calls ndarray /
// LAPACK on tall-skinny panels, scan-rs/src/dim_red/*.rs):
//   gram_kernel          C = X^T Y, tall-skinny, v_mfma_f64_16x16x4_f64
//   gemm_nn_kernel       Out = beta*C + alpha * X W, tall-skinny times small, same MFMA
//   gram_vec_kernel      C = X^T y for one vector, streaming
//   weighted_colsum_*    w = B^T X, the offset term of a low-rank-offset product
// and the element-wise helpers (column scale / axpy, copy, permute, transpose, fill, the seeded start panel). Which kernel a
// product goes to is decided in dense.hip (gram_route / gemm_route); launch_gram / launch_gemm_nn here ask and dispatch.
#include "common.hpp"
#include "device_map.hpp"
#include "launch_util.hpp"

#include <algorithm>

namespace scanrs {

// ---------------------------------------------------------------------------------------------
// w[q,:] = sum_i B[i,q] * X[i,:]   (the `v.dot(rhs)` / `lhs.dot(u)` of low_rank_offset.rs:76-95)
// Streaming form: a wave walks rows r0 + wave, r0 + wave + 4, ... of its block's slice, lanes own column pairs (one 16-byte load
// per lane per row, a panel row = one coalesced read), 8 rows in flight per wave; the four waves' partial sums meet in LDS in
// wave order (deterministic). HBM-bound: n x l x 8 bytes once.
__global__ __launch_bounds__(256) void weighted_colsum_partial_kernel(const double *__restrict__ B, uint32_t rank,
                                                                      const double *__restrict__ X, uint32_t ldx,
                                                                      uint64_t n, uint32_t l, uint64_t rows_per_block,
                                                                      double *__restrict__ partial, double *__restrict__ Xc, uint32_t ldc) {
    __shared__ d2 part[3][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * rows_per_block;
    const uint64_t r1 = min(n, r0 + rows_per_block);
    for (uint32_t q = 0; q < rank; q++) {
        for (uint32_t c0 = 0; c0 < l; c0 += 128u) {
            const uint32_t col = c0 + lane * 2u;
            const bool act = col < l; // ldx is even and >= l rounded up to even: the pair load stays inside the row
            d2 acc = {0.0, 0.0};
            if (act) {
                uint64_t i = r0 + wave;
                for (; i + 28u < r1; i += 32u) {
                    d2 x[8];
                    double b[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        x[u] = *reinterpret_cast<const d2 *>(X + (i + 4u * u) * ldx + col);
                        b[u] = B[(i + 4u * u) * rank + q];
                    }
                    if (Xc && q == 0u) { // the compact copy of the panel that the tile product stages, from the same read
#pragma unroll
                        for (int u = 0; u < 8; u++) *reinterpret_cast<d2 *>(Xc + (i + 4u * u) * ldc + col) = x[u];
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        acc.x = fma(b[u], x[u].x, acc.x);
                        acc.y = fma(b[u], x[u].y, acc.y);
                    }
                }
                for (; i < r1; i += 4u) {
                    const d2 x = *reinterpret_cast<const d2 *>(X + i * ldx + col);
                    const double b = B[i * rank + q];
                    if (Xc && q == 0u) *reinterpret_cast<d2 *>(Xc + i * ldc + col) = x;
                    acc.x = fma(b, x.x, acc.x);
                    acc.y = fma(b, x.y, acc.y);
                }
            }
            __syncthreads(); // `part` free again
            if (wave > 0) part[wave - 1][lane] = acc;
            __syncthreads();
            if (wave == 0 && act) {
                for (int w = 0; w < 3; w++) {
                    acc.x += part[w][lane].x;
                    acc.y += part[w][lane].y;
                }
                double *dst = partial + ((size_t)blockIdx.x * rank + q) * l + col;
                dst[0] = acc.x;
                if (col + 1 < l) dst[1] = acc.y;
            }
        }
    }
}
// ordered sum of the per-block partials: 64 output entries per workgroup, the blocks dealt to 4 groups of 64 threads
// (8 independent loads in flight each), the four group sums added in group order (deterministic)
__global__ __launch_bounds__(256) void weighted_colsum_finish_kernel(const double *__restrict__ partial, uint32_t nblocks, uint32_t rank,
                                                                     uint32_t l, double *__restrict__ w, uint32_t ldw) {
    __shared__ double part[4][64];
    const uint32_t e = blockIdx.x * 64u + (threadIdx.x & 63u), g = threadIdx.x >> 6;
    const bool act = e < rank * l;
    double s = 0.0;
    if (act) {
        const size_t stride = (size_t)rank * l;
        uint32_t b = g;
        for (; b + 28u < nblocks; b += 32u) {
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; u++) t[u] = partial[(size_t)(b + 4u * u) * stride + e];
#pragma unroll
            for (int u = 0; u < 8; u++) s += t[u];
        }
        for (; b < nblocks; b += 4u) s += partial[(size_t)b * stride + e];
    }
    part[g][threadIdx.x & 63u] = s;
    __syncthreads();
    if (g == 0 && act) {
        const uint32_t q = e / l, c = e % l, t = threadIdx.x;
        w[(size_t)q * ldw + c] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    }
}

// ---------------------------------------------------------------------------------------------
// Tall-skinny dense kernels on v_mfma_f64_16x16x4_f64.
// Operand maps (cdna_hip_programming.md §3): lane l gives A[i = l&15][k = l>>4], B[k = l>>4][j = l&15];
// the 4 results of lane l are D[row = (l>>4) + 4*reg][col = l&15].

// C = X^T Y over a slice of rows; one wave per (32x32 tile of C, row slice).
__global__ __launch_bounds__(64) void gram_kernel(const double *__restrict__ X, uint32_t ldx, uint32_t n,
                                                  const double *__restrict__ Y, uint32_t ldy, uint32_t m, uint64_t rows,
                                                  uint64_t rows_per_split, uint32_t tiles_m,
                                                  double *__restrict__ slab, const int *__restrict__ skip) {
    if (skip && *skip) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t li = lane & 15u, lk = lane >> 4;
    const uint32_t i0 = (blockIdx.x / tiles_m) * 32u, j0 = (blockIdx.x % tiles_m) * 32u;
    const uint64_t r0 = (uint64_t)blockIdx.y * rows_per_split;
    const uint64_t r1 = min(rows, r0 + rows_per_split);
    const bool ai0 = i0 + li < n, ai1 = i0 + 16u + li < n;
    const bool bj0 = j0 + li < m, bj1 = j0 + 16u + li < m;
    d4 acc00 = {0, 0, 0, 0}, acc01 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
    for (uint64_t r = r0; r < r1; r += 8u) {
        double a0[2], a1[2], b0[2], b1[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint64_t rr = r + 4u * h + lk;
            const bool v = rr < r1;
            const double *xr = X + rr * ldx + i0 + li;
            const double *yr = Y + rr * ldy + j0 + li;
            a0[h] = (v && ai0) ? xr[0] : 0.0;
            a1[h] = (v && ai1) ? xr[16] : 0.0;
            b0[h] = (v && bj0) ? yr[0] : 0.0;
            b1[h] = (v && bj1) ? yr[16] : 0.0;
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h], b0[h], acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h], b1[h], acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[h], b0[h], acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[h], b1[h], acc11, 0, 0, 0);
        }
    }
    double *__restrict__ dst = slab + (size_t)blockIdx.y * n * m;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const uint32_t ra = i0 + lk + 4u * reg, rb = ra + 16u;
        const uint32_t ca = j0 + li, cb = ca + 16u;
        if (ra < n && ca < m) dst[(size_t)ra * m + ca] = acc00[reg];
        if (ra < n && cb < m) dst[(size_t)ra * m + cb] = acc01[reg];
        if (rb < n && ca < m) dst[(size_t)rb * m + ca] = acc10[reg];
        if (rb < n && cb < m) dst[(size_t)rb * m + cb] = acc11[reg];
    }
}
__global__ void gram_finish_kernel(const double *__restrict__ slab, uint32_t splits, uint64_t nm,
                                   double *__restrict__ C, const int *__restrict__ skip) {
    if (skip && *skip) return;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nm) return;
    double s = 0.0;
    for (uint32_t k = 0; k < splits; k++) s += slab[(size_t)k * nm + e];
    C[e] = s;
}

// Out = beta*Cin + alpha * X W. One wave per 16 rows x 64 columns. The k index is permuted inside a
// 16-deep step (lane group lk owns k0+4*lk .. +3) so that each lane reads 32 contiguous bytes of X.
template <int NJ>
__global__ __launch_bounds__(256) void gemm_nn_kernel(const double *__restrict__ X, uint32_t ldx, uint32_t n,
                                                      const double *__restrict__ W, uint32_t ldw, uint32_t m,
                                                      uint64_t rows, double alpha, double beta,
                                                      const double *Cin, uint32_t ldc, double *Out,
                                                      uint32_t ldo, const int *__restrict__ skip) {
    if (skip && *skip) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t li = lane & 15u, lk = lane >> 4;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 16u;
    if (r0 >= rows) return;
    const uint32_t j0 = blockIdx.y * 16u * NJ;
    const uint64_t ra = r0 + li;
    const bool rv = ra < rows;
    const double *__restrict__ xrow = X + ra * ldx;
    d4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = (d4){0, 0, 0, 0};
    bool cv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) cv[j] = j0 + 16u * j + li < m;

    for (uint32_t k0 = 0; k0 < n; k0 += 16u) {
        const uint32_t kb = k0 + 4u * lk;
        double xa[4];
        if (rv && kb + 3u < n) {
            const d2 p = *reinterpret_cast<const d2 *>(xrow + kb);
            const d2 q = *reinterpret_cast<const d2 *>(xrow + kb + 2);
            xa[0] = p.x;
            xa[1] = p.y;
            xa[2] = q.x;
            xa[3] = q.y;
        } else {
#pragma unroll
            for (int s = 0; s < 4; s++) xa[s] = (rv && kb + s < n) ? xrow[kb + s] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t kk = kb + s;
            const bool kv = kk < n;
            const double *__restrict__ wr = W + (size_t)kk * ldw + j0 + li;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const double b = (kv && cv[j]) ? wr[16 * j] : 0.0;
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s], b, acc[j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const uint64_t rr = r0 + lk + 4u * reg;
        if (rr >= rows) continue;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            if (!cv[j]) continue;
            const uint32_t cc = j0 + 16u * j + li;
            double r = alpha * acc[j][reg];
            if (beta != 0.0) r = fma(beta, Cin[rr * ldc + cc], r);
            Out[rr * ldo + cc] = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// small element-wise helpers
__global__ void copy_cols_kernel(const double *__restrict__ src, uint32_t lds, double *__restrict__ dst, uint32_t ldd,
                                 uint64_t rows, uint32_t l, const int *__restrict__ skip) {
    if (skip && *skip) return;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * l) return;
    const uint64_t r = e / l;
    const uint32_t c = (uint32_t)(e % l);
    dst[r * ldd + c] = src[r * lds + c];
}
// dst[:, j] = src[:, idx[j]] (gather) or dst[:, idx[j]] = src[:, j] (scatter), j < n_idx
__global__ void permute_cols_kernel(const double *__restrict__ src, uint32_t lds, double *__restrict__ dst, uint32_t ldd,
                                    uint64_t rows, const uint32_t *__restrict__ idx, uint32_t n_idx, int scatter) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * n_idx) return;
    const uint64_t r = e / n_idx;
    const uint32_t j = (uint32_t)(e % n_idx);
    if (scatter)
        dst[r * ldd + idx[j]] = src[r * lds + j];
    else
        dst[r * ldd + j] = src[r * lds + idx[j]];
}
// Seeded start panel generated on the device. The reference draws the panel from ONE sequential stream
// (SmallRng = xoshiro256++, scan-rs/src/dim_red/bk_svd.rs:83-90); the state transition of xoshiro is linear over
// GF(2), so the state after s*d draws is J^s * state0 with J = T^d. The host supplies J^(2^k) (solver.cpp); stream s
// rebuilds its start state from the binary digits of s and then draws its d values sequentially. The values and
// their order are identical to the sequential stream.
__device__ __forceinline__ uint64_t xo_rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
__global__ __launch_bounds__(256) void omega_jump_kernel(const uint64_t *__restrict__ jpow, int n_pow, uint64_t s0, uint64_t s1,
                                                         uint64_t s2, uint64_t s3, uint64_t d, uint64_t total, double *__restrict__ out,
                                                         uint32_t ld, uint64_t seq_cols, int transpose) {
    const uint64_t sid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t e0 = sid * d;
    if (e0 >= total) return;
    uint64_t st[4] = {s0, s1, s2, s3};
    for (int k = 0; k < n_pow; k++) {
        if (!((sid >> k) & 1ull)) continue;
        const uint64_t *__restrict__ m = jpow + (size_t)k * 256 * 4;
        uint64_t nx[4] = {0, 0, 0, 0};
        for (int i = 0; i < 256; i++) {
            const uint64_t *r = m + i * 4;
            const uint64_t x = (r[0] & st[0]) ^ (r[1] & st[1]) ^ (r[2] & st[2]) ^ (r[3] & st[3]);
            nx[i >> 6] |= (uint64_t)(__popcll(x) & 1) << (i & 63);
        }
        st[0] = nx[0];
        st[1] = nx[1];
        st[2] = nx[2];
        st[3] = nx[3];
    }
    const uint64_t e1 = min(total, e0 + d);
    for (uint64_t e = e0; e < e1; e++) {
        const uint64_t result = xo_rotl(st[0] + st[3], 23) + st[0];
        const uint64_t t = st[1] << 17;
        st[2] ^= st[0];
        st[3] ^= st[1];
        st[1] ^= st[2];
        st[0] ^= st[3];
        st[2] ^= t;
        st[3] = xo_rotl(st[3], 45);
        const double v12 = __longlong_as_double((long long)((result >> 12) | 0x3FF0000000000000ull));
        const double v = (v12 - 1.0) * 2.0 + (-1.0);
        // sequential order is row-major over (seq_rows x seq_cols); the device panel is that matrix or its transpose
        const uint64_t i = e / seq_cols, j = e % seq_cols;
        if (transpose)
            out[j * ld + i] = v;
        else
            out[i * ld + j] = v;
    }
}

// dst[j, i] = src[i, j] for src (rows x cols, compact) -> dst (cols x rows, leading dimension ldd); LDS tile transpose
__global__ __launch_bounds__(256) void transpose_kernel(const double *__restrict__ src, uint64_t rows, uint64_t cols,
                                                        double *__restrict__ dst, uint32_t ldd) {
    __shared__ double tile[32][33];
    const uint64_t c0 = (uint64_t)blockIdx.x * 32u, r0 = (uint64_t)blockIdx.y * 32u;
    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5; // 32 x 8
    for (uint32_t k = ty; k < 32u; k += 8u)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = src[(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (uint32_t k = ty; k < 32u; k += 8u)
        if (c0 + k < cols && r0 + tx < rows) dst[(c0 + k) * ldd + r0 + tx] = tile[tx][k];
}
__global__ void fill_kernel(double *p, uint64_t n, double v) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) p[e] = v;
}

// Xc (optional): a compact copy of X's first l columns in rows of ldc, written from the same read (l even: the lanes move column pairs)
// C = X^T y for ONE vector y (rows x 1, stride ldy) and up to 128 columns of X: IRLBA's re-orthogonalisation dots (irlba.rs:19-22,
// 131-134, 10^6 x <= 70 against one Lanczos vector). The 32 x 32 MFMA tiles of gram_kernel spend 31 of 32 columns on padding there and
// load 16 lanes x 8 B per row (0.6-0.8 ms per call at 10^6 rows); here a lane owns columns lane and lane + 64, a wave walks rows
// r0 + wave, + 4, ... of its block's slice (a row of X = one coalesced read, y[r] one broadcast load), eight rows in flight; the four
// waves' sums meet in LDS in wave order, the blocks' partials are added in block order by gram_finish_kernel: deterministic.
__global__ __launch_bounds__(256) void gram_vec_kernel(const double *__restrict__ X, uint32_t ldx, uint32_t n, const double *__restrict__ y, uint32_t ldy,
                                                       uint64_t rows, uint64_t rows_per_block, double *__restrict__ slab, const int *__restrict__ skip) {
    if (skip && *skip) return;
    __shared__ double part[3][128];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    const bool a0 = lane < n, a1 = lane + 64u < n;
    double acc0 = 0.0, acc1 = 0.0;
    uint64_t i = r0 + wave;
    for (; i + 28u < r1; i += 32u) {
        double x0[8], x1[8], yv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const double *xr = X + (i + 4u * u) * ldx;
            x0[u] = a0 ? xr[lane] : 0.0;
            x1[u] = a1 ? xr[lane + 64u] : 0.0;
            yv[u] = y[(i + 4u * u) * ldy];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            acc0 = fma(x0[u], yv[u], acc0);
            acc1 = fma(x1[u], yv[u], acc1);
        }
    }
    for (; i < r1; i += 4u) {
        const double *xr = X + i * ldx;
        const double yv = y[i * ldy];
        acc0 = fma(a0 ? xr[lane] : 0.0, yv, acc0);
        acc1 = fma(a1 ? xr[lane + 64u] : 0.0, yv, acc1);
    }
    if (wave > 0) {
        part[wave - 1][lane] = acc0;
        part[wave - 1][lane + 64u] = acc1;
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 0; w < 3; w++) {
            acc0 += part[w][lane];
            acc1 += part[w][lane + 64u];
        }
        double *dst = slab + (size_t)blockIdx.x * n;
        if (a0) dst[lane] = acc0;
        if (a1) dst[lane + 64u] = acc1;
    }
}

void launch_weighted_colsum(Storage &st, const double *B, uint32_t rank, const double *X, uint32_t ldx, uint64_t n,
                            uint32_t l, double *w, uint32_t ldw, double *Xc, uint32_t ldc) {
    if (rank == 0 || l == 0) return;
    uint32_t nblocks = (uint32_t)std::min<uint64_t>(1024, (n + 255) / 256);
    if (nblocks == 0) nblocks = 1;
    const uint64_t rpb = (n + nblocks - 1) / nblocks;
    double *partial = st.scratch.get<double>("wcs_partial", (size_t)nblocks * rank * l);
    ProfScope ps(st, "weighted_colsum", (double)n * l * 8.0 + (double)n * rank * 8.0);
    hipLaunchKernelGGL(weighted_colsum_partial_kernel, dim3(nblocks), dim3(256), 0, st.stream, B, rank, X, ldx, n, l, rpb,
                       partial, Xc, ldc);
    hipLaunchKernelGGL(weighted_colsum_finish_kernel, grid1((uint64_t)rank * l, 64), dim3(256), 0, st.stream, partial,
                       nblocks, rank, l, w, ldw);
    SCANRS_HIP(hipGetLastError());
}

static bool on_side_stream(const Storage &st) {
    // work queued on a side stream runs beside the persistent tile kernel of a sparse pass, which holds all of every CU's LDS: a
    // kernel that needs LDS waits for the end of the pass; the register-only MFMA kernels fit the registers the tile kernel leaves
    return st.opt.dense_side_no_lds && ((st.aux_stream && st.stream == st.aux_stream) || (st.aux2_stream && st.stream == st.aux2_stream));
}

// one vector against a narrow panel: the streaming form (gram_vec_kernel)
static void launch_gram_vec(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint64_t rows, double *C) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, (rows + 255) / 256);
    const uint64_t rpb = (rows + blocks - 1) / blocks;
    double *slab = st.scratch.get<double>(st.skey("gram_slab"), (size_t)blocks * n);
    ProfScope ps(st, "gram_vec_f64", (double)rows * (n + 1) * 8.0);
    hipLaunchKernelGGL(gram_vec_kernel, dim3(blocks), dim3(256), 0, st.stream, X, ldx, n, Y, ldy, rows, rpb, slab, st.skip_flag);
    // (the blocks' partials in block order, four groups of 64 threads with eight loads in flight each: the plain ordered loop of
    // gram_finish_kernel walks 1 024 partials one load at a time)
    hipLaunchKernelGGL(weighted_colsum_finish_kernel, grid1((uint64_t)n, 64), dim3(256), 0, st.stream, slab, blocks, 1u, n, C, n);
    SCANRS_HIP(hipGetLastError());
}

// one wave per (32 x 32 tile of C, row slice)
static void launch_gram_wave(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint32_t m,
                             uint64_t rows, double *C) {
    const uint32_t tiles_n = (n + 31u) / 32u, tiles_m = (m + 31u) / 32u;
    const uint64_t tiles = (uint64_t)tiles_n * tiles_m;
    // aim for ~8k waves, at least 64 rows per slice
    uint64_t splits = std::max<uint64_t>(1, std::min<uint64_t>((rows + 63) / 64, (8192 + tiles - 1) / tiles));
    splits = std::min<uint64_t>(splits, 1024);
    uint64_t rps = (rows + splits - 1) / splits;
    rps = (rps + 7) & ~7ull;
    if (rps == 0) rps = 8;
    splits = std::max<uint64_t>(1, (rows + rps - 1) / rps);
    double *slab = st.scratch.get<double>(st.skey("gram_slab"), (size_t)splits * n * m);
    {
        ProfScope ps(st, "gram_mfma_f64", (double)rows * (n + (X == Y && n == m ? 0 : m)) * 8.0 + (double)n * m * 8.0);
        hipLaunchKernelGGL(gram_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(64), 0, st.stream, X, ldx, n, Y, ldy,
                           m, rows, rps, tiles_m, slab, st.skip_flag);
        hipLaunchKernelGGL(gram_finish_kernel, grid1((uint64_t)n * m, 256), dim3(256), 0, st.stream, slab,
                           (uint32_t)splits, (uint64_t)n * m, C, st.skip_flag);
    }
    SCANRS_HIP(hipGetLastError());
}

void launch_gram_route(Storage &st, int route, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint32_t m,
                       uint64_t rows, double *C) {
    if (n == 0 || m == 0) return;
    if (route == GRAM_AUTO) {
        route = gram_route(n, m, rows, ldx, ldy, on_side_stream(st), st.skip_flag != nullptr);
    } else if (route == GRAM_VEC) { // a forced kernel: its own preconditions, not the thresholds
        if (m != 1u || n > 128u || st.skip_flag) fail(SCANRS_ERR_ARGUMENT, "gram_vec: one vector, at most 128 panel columns, no skip flag");
    } else if (route == GRAM_TILED) {
        if ((ldx & 1u) || (ldy & 1u)) fail(SCANRS_ERR_ARGUMENT, "gram_tiled: ldx and ldy must be even");
    } else if (route != GRAM_WAVE) {
        fail(SCANRS_ERR_ARGUMENT, "unknown Gram route %d", route);
    }
    if (route == GRAM_VEC)
        launch_gram_vec(st, X, ldx, n, Y, ldy, rows, C);
    else if (route == GRAM_TILED)
        launch_gram_tiled(st, X, ldx, n, Y, ldy, m, rows, C);
    else
        launch_gram_wave(st, X, ldx, n, Y, ldy, m, rows, C);
}
void launch_gram(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *Y, uint32_t ldy, uint32_t m,
                 uint64_t rows, double *C) {
    launch_gram_route(st, GRAM_AUTO, X, ldx, n, Y, ldy, m, rows, C);
}

// one wave per 16 rows x 16 NJ columns
static void launch_gemm_wave(Storage &st, uint32_t nj, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                             uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo) {
    const uint64_t waves = (rows + 15) / 16;
    ProfScope ps(st, "gemm_nn_mfma_f64", (double)rows * (n + m) * 8.0 + (double)n * m * 8.0);
    const dim3 block(256);
    if (nj == 1u) {
        hipLaunchKernelGGL((gemm_nn_kernel<1>), dim3((unsigned)((waves + 3) / 4), (m + 15u) / 16u), block, 0, st.stream, X,
                           ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo, st.skip_flag);
    } else if (nj == 2u) {
        hipLaunchKernelGGL((gemm_nn_kernel<2>), dim3((unsigned)((waves + 3) / 4), (m + 31u) / 32u), block, 0, st.stream, X,
                           ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo, st.skip_flag);
    } else {
        hipLaunchKernelGGL((gemm_nn_kernel<4>), dim3((unsigned)((waves + 3) / 4), (m + 63u) / 64u), block, 0, st.stream, X,
                           ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo, st.skip_flag);
    }
    SCANRS_HIP(hipGetLastError());
}

void launch_gemm_route(Storage &st, int route, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                       uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out, uint32_t ldo) {
    if (rows == 0 || m == 0) return;
    if (ldx & 1u) fail(SCANRS_ERR_ARGUMENT, "gemm: ldx must be even");
    const bool aligned = (reinterpret_cast<uintptr_t>(X) & 15u) == 0;
    if (route == GEMM_AUTO) {
        route = gemm_route(aligned, ldx, n, m, rows, on_side_stream(st), st.opt.gemm_direct != 0).route;
    } else if (route == GEMM_DIRECT) { // a forced kernel: its own preconditions, not the dispatcher's choice
        if (!gemm_direct_ok(X, ldx, n, m, rows)) fail(SCANRS_ERR_ARGUMENT, "gemm_direct: needs X 16-byte aligned, n >= 16, rows >= 64, m <= 4096");
    } else if (route != GEMM_WAVE && route != GEMM_TILED && route != GEMM_SKINNY_LDS) {
        fail(SCANRS_ERR_ARGUMENT, "unknown GEMM route %d", route);
    }
    if (route == GEMM_DIRECT)
        launch_gemm_direct(st, X, ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo);
    else if (route == GEMM_TILED)
        launch_gemm_tiled(st, X, ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo);
    else if (route == GEMM_SKINNY_LDS)
        launch_gemm_skinny_lds(st, X, ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo);
    else
        launch_gemm_wave(st, gemm_wave_nj(m), X, ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo);
}
void launch_gemm_nn(Storage &st, const double *X, uint32_t ldx, uint32_t n, const double *W, uint32_t ldw, uint32_t m,
                    uint64_t rows, double alpha, double beta, const double *Cin, uint32_t ldc, double *Out,
                    uint32_t ldo) {
    launch_gemm_route(st, GEMM_AUTO, X, ldx, n, W, ldw, m, rows, alpha, beta, Cin, ldc, Out, ldo);
}

// one column with a scalar that arrives as a kernel argument (IRLBA's normalisations and three-term updates, irlba.rs:137-160: the
// scalar used to travel as a 1 x 1 matrix through a pageable upload and a synchronisation per call):
//   MODE 0: dst[r] = src[r] * alpha        MODE 1: dst[r] = src[r] * alpha + dst[r]  (product rounded, then the sum: what the GEMM form gave)
template <int MODE>
__global__ void col_scalar_kernel(double *dst, uint32_t ldd, const double *src, uint32_t lds, uint64_t rows, double alpha) { // (dst may be src)
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const double t = __dmul_rn(src[r * lds], alpha);
    dst[r * ldd] = MODE == 0 ? t : __dadd_rn(t, dst[r * ldd]);
}
// the same with the scalar taken from device memory as the SQUARE of a norm (a 1 x 1 Gram matrix left where the Gram kernel wrote it):
//   MODE 0: dst[r] = src[r] * invcheck(sqrt(*nsq))  (irlba.rs:25-33: 1 / x above 2 eps, else 0)    MODE 1: dst[r] = src[r] * (-sqrt(*nsq)) + dst[r]
template <int MODE>
__global__ void col_scalar_dev_kernel(double *dst, uint32_t ldd, const double *src, uint32_t lds, uint64_t rows, const double *__restrict__ nsq) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const double nrm = __dsqrt_rn(*nsq);
    const double alpha = MODE == 0 ? (nrm > 2.0 * 2.220446049250313e-16 ? __ddiv_rn(1.0, nrm) : 0.0) : -nrm;
    const double t = __dmul_rn(src[r * lds], alpha);
    dst[r * ldd] = MODE == 0 ? t : __dadd_rn(t, dst[r * ldd]);
}
void launch_col_scale_dev(Storage &st, double *dst, uint32_t ldd, const double *src, uint32_t lds, uint64_t rows, const double *nsq) {
    if (rows == 0) return;
    hipLaunchKernelGGL(col_scalar_dev_kernel<0>, grid1(rows, 256), dim3(256), 0, st.stream, dst, ldd, src, lds, rows, nsq);
    SCANRS_HIP(hipGetLastError());
}
void launch_col_axpy_dev(Storage &st, double *y, uint32_t ldy, const double *x, uint32_t ldx, uint64_t rows, const double *nsq) {
    if (rows == 0) return;
    hipLaunchKernelGGL(col_scalar_dev_kernel<1>, grid1(rows, 256), dim3(256), 0, st.stream, y, ldy, x, ldx, rows, nsq);
    SCANRS_HIP(hipGetLastError());
}
void launch_col_scale(Storage &st, double *dst, uint32_t ldd, const double *src, uint32_t lds, uint64_t rows, double alpha) {
    if (rows == 0) return;
    hipLaunchKernelGGL(col_scalar_kernel<0>, grid1(rows, 256), dim3(256), 0, st.stream, dst, ldd, src, lds, rows, alpha);
    SCANRS_HIP(hipGetLastError());
}
void launch_col_axpy(Storage &st, double *y, uint32_t ldy, const double *x, uint32_t ldx, uint64_t rows, double alpha) {
    if (rows == 0) return;
    hipLaunchKernelGGL(col_scalar_kernel<1>, grid1(rows, 256), dim3(256), 0, st.stream, y, ldy, x, ldx, rows, alpha);
    SCANRS_HIP(hipGetLastError());
}
void launch_copy_cols(Storage &st, const double *src, uint32_t lds, double *dst, uint32_t ldd, uint64_t rows,
                      uint32_t l) {
    if (rows == 0 || l == 0) return;
    hipLaunchKernelGGL(copy_cols_kernel, grid1(rows * l, 256), dim3(256), 0, st.stream, src, lds, dst, ldd, rows, l, st.skip_flag);
    SCANRS_HIP(hipGetLastError());
}
void launch_permute_cols(Storage &st, const double *src, uint32_t lds, double *dst, uint32_t ldd, uint64_t rows,
                         const uint32_t *d_idx, uint32_t n_idx, bool scatter) {
    if (rows == 0 || n_idx == 0) return;
    hipLaunchKernelGGL(permute_cols_kernel, grid1(rows * n_idx, 256), dim3(256), 0, st.stream, src, lds, dst, ldd, rows, d_idx,
                       n_idx, scatter ? 1 : 0);
    SCANRS_HIP(hipGetLastError());
}
void launch_omega_jump(Storage &st, const uint64_t *d_jpow, int n_pow, const uint64_t s[4], uint64_t d, uint64_t total, double *out,
                       uint32_t ld, uint64_t seq_cols, bool transpose) {
    const uint64_t streams = (total + d - 1) / d;
    hipLaunchKernelGGL(omega_jump_kernel, grid1(streams, 256), dim3(256), 0, st.stream, d_jpow, n_pow, s[0], s[1], s[2], s[3], d, total,
                       out, ld, seq_cols, transpose ? 1 : 0);
    SCANRS_HIP(hipGetLastError());
}
void launch_transpose(Storage &st, const double *src, uint64_t rows, uint64_t cols, double *dst, uint32_t ldd) {
    if (rows == 0 || cols == 0) return;
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, st.stream, src,
                       rows, cols, dst, ldd);
    SCANRS_HIP(hipGetLastError());
}
// columns [c0, c0 + nc) of a panel filled with a fixed pseudo-random function of (GLOBAL row, column): every rank of a sharded
// panel produces its own rows of the same matrix without talking to anybody (splitmix64 of the pair, mapped to (-1, 1))
__global__ void fill_hash_kernel(double *p, uint32_t ld, uint64_t rows, uint64_t row0, uint32_t c0, uint32_t nc, uint64_t seed) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * nc) return;
    const uint64_t r = e / nc;
    const uint32_t c = (uint32_t)(e - r * nc);
    uint64_t z = seed + (row0 + r) * 0x9E3779B97F4A7C15ull + (uint64_t)(c0 + c) * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    p[r * ld + c0 + c] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
void launch_fill_hash(Storage &st, double *p, uint32_t ld, uint64_t rows, uint64_t row0, uint32_t c0, uint32_t nc, uint64_t seed) {
    if (rows == 0 || nc == 0) return;
    hipLaunchKernelGGL(fill_hash_kernel, grid1(rows * nc, 256), dim3(256), 0, st.stream, p, ld, rows, row0, c0, nc, seed);
}
void launch_fill_f64(Storage &st, double *p, uint64_t n, double v) {
    if (n == 0) return;
    hipLaunchKernelGGL(fill_kernel, grid1(n, 256), dim3(256), 0, st.stream, p, n, v);
    SCANRS_HIP(hipGetLastError());
}

// scanrs_init(): loads this file's code object (library_warm_up, kernels.hip)
__global__ void warm_panel_ops_kernel() {}
void warm_panel_ops(hipStream_t s) { hipLaunchKernelGGL(warm_panel_ops_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
