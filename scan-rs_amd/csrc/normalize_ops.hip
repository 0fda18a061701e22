// The small kernels of normalize for gfx950 (MI355X) + their launchers: the fixed-point per-inner moments (col_moments_kernel,
// planned by col_moments_plan.hpp), the finishing step of scale_and_center, the count scale, the digit histogram of the median,
// the binomial residual vectors, a deterministic total, and to_dense.
#include "common.hpp"
#include "device_map.hpp"
#include "col_moments_plan.hpp"
#include "launch_util.hpp"

#include <algorithm>

namespace scanrs {

// scale_and_center finishing step, sqz/src/mat.rs:993-1000 + :966-981 + :946 (neg_means)
__global__ void finish_moments_kernel(const double *__restrict__ sum, const double *__restrict__ sumsq, uint64_t n,
                                      double m, int given_scale, const double *__restrict__ scale_in,
                                      double *__restrict__ neg_mean_over_scale, double *__restrict__ inv_scale,
                                      double *__restrict__ scale_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double mean = sum[i] / m;
    double sc;
    if (given_scale) {
        sc = scale_in[i];
    } else {
        const double d = sumsq[i] / m - mean * mean;
        sc = d <= 0.0 ? 1.0 : sqrt(d);
    }
    if (neg_mean_over_scale) neg_mean_over_scale[i] = -(mean / sc);
    if (inv_scale) inv_scale[i] = 1.0 / sc;
    if (scale_out) scale_out[i] = sc;
}
// col_scales = target / count  (scan-rs/src/normalization.rs:169)
__global__ void u32_to_scale_kernel(const uint32_t *__restrict__ counts, uint64_t n, double target,
                                    double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = target / (double)counts[i];
}
// 12-bit digit histogram of the values matching a prefix: the counting step of the radix select that
// stands in for median_mut's sort (scan-rs/src/stats.rs:13-38).
__global__ __launch_bounds__(256) void hist12_kernel(const uint32_t *__restrict__ v, uint64_t n, uint32_t shift,
                                                     uint32_t digit_mask, uint32_t prefix_mask, uint32_t prefix,
                                                     unsigned long long *__restrict__ hist) {
    __shared__ uint32_t h[4096];
    for (uint32_t i = threadIdx.x; i < 4096u; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = v[i];
        if ((x & prefix_mask) == prefix) atomicAdd(&h[(x >> shift) & digit_mask], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 4096u; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}
// to_dense (sqz/src/mat.rs:188-205): scatter mapped nonzeros into a zeroed rows_v x cols_v array.
__global__ __launch_bounds__(256) void densify_kernel(const uint32_t *__restrict__ indices,
                                                      const uint32_t *__restrict__ values,
                                                      const Item *__restrict__ items, uint32_t n_items, DevMap map,
                                                      int outer_is_view_row, uint64_t cols_v, double *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wid >= n_items) return;
    const Item it = items[wid];
    for (uint32_t p = lane; p < it.len; p += 64u) {
        const uint32_t in = indices[it.start + p];
        const double x = eval_map(map, values[it.start + p], it.row, in);
        const uint64_t r = outer_is_view_row ? it.row : in, c = outer_is_view_row ? in : it.row;
        out[r * cols_v + c] = x;
    }
}
// pi, u, v of binom_deviance_resid / binom_pearson_resid (scan-rs/src/normalization.rs:232-322)
__global__ void binom_rows_kernel(int kind, const double *__restrict__ rowsum, uint64_t nrows, double total,
                                  double *__restrict__ pi, double *__restrict__ u) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const double x = rowsum[i] / total;
    pi[i] = x;
    u[i] = kind == OP_BINOM_DEV ? sqrt(log(1.0 / (1.0 - x))) : sqrt(x / (1.0 - x));
}
__global__ void binom_cols_kernel(int kind, const double *__restrict__ n, uint64_t ncols, double *__restrict__ v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncols) return;
    v[i] = kind == OP_BINOM_DEV ? -sqrt(2.0 * n[i]) : -sqrt(n[i]);
}
__global__ void sum_f64_kernel(const double *__restrict__ x, uint64_t n, double *__restrict__ out) {
    // single block, fixed order: deterministic total (fit_multinomial_model, normalization.rs:224)
    __shared__ double sh[256];
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// ---- per-INNER-position sums of mapped values from the copy whose outer vectors are the summed-over axis ----------------------
// The moments of normalize() (sum and sum of squares of log(1 + x s_c) per gene over the cells) walk the gene-major copy and
// pay one f64 logarithm per nonzero (5.9 ms at 10^9 nonzeros: the pass is bound by that arithmetic, not by its 8 B per
// nonzero). On the CELL-major copy the logarithm's argument depends on the count and the outer vector only, and 99.9 % of
// the counts are at most 8: a wave evaluates a cell's eight values once and every nonzero is a lookup — but the sums belong
// to the inner positions, i.e. they are scattered. They are collected in LDS (a workgroup owns a range of 8192 inner positions
// and a block of cells; the nonzeros of a cell inside the range are a contiguous run: bounds table) as 64-bit FIXED-POINT
// numbers with integer atomics: integer addition is associative, so the result does not depend on the order in which the waves
// arrive (float atomics would make it depend on timing), and with the scale chosen per launch from a bound of the values
// (col_moments_plan.hpp) a workgroup's sums cannot overflow. Every term is rounded to that one quantum, an absolute error: the
// plan accepts a map only when the quantum is below 2^-40 of the SMALLEST nonzero term any slice can hold (2^-33 for the
// squares), so that every slice's sums are right to 4.6e-13 (5.9e-11) relative, not only those of the slices that hold large
// values; every other map takes the ordinary pass. The partial sums of the workgroups are added in double, in workgroup order.
constexpr uint32_t CM_RANGE_SHIFT = 13; // inner positions per range: 8192 x 2 x 8 B = 128 KB of LDS
constexpr uint32_t CM_TAB = 8;          // counts 1 .. 8 come from the per-cell table
constexpr uint32_t CM_NV = 4;           // cells per wave and trip (their bounds, their segments' loads side by side)
template <int MODE>
__global__ __launch_bounds__(1024) void col_moments_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                           const uint32_t *__restrict__ values, const uint32_t *__restrict__ bounds, uint32_t nb,
                                                           uint64_t n_outer, uint64_t cells_per_wg, uint32_t n_inner, DevMap map, double scale1,
                                                           double scale2, unsigned long long *__restrict__ slab) {
    extern __shared__ unsigned long long cm_acc[]; // [MODE][inner position of the range]: one array per moment (interleaved, the 16-byte stride put 64 lanes on 16 bank groups)
    const uint32_t range = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const uint32_t g0 = range << CM_RANGE_SHIFT, ng = min(1u << CM_RANGE_SHIFT, n_inner - g0);
    const uint32_t tiles_per_range = (1u << CM_RANGE_SHIFT) >> BT_SHIFT;
    const uint32_t b0 = range * tiles_per_range, b1 = min(nb, b0 + tiles_per_range);
    for (uint32_t i = tid; i < (MODE << CM_RANGE_SHIFT); i += blockDim.x) cm_acc[i] = 0ull;
    __syncthreads();
    const uint64_t c_begin = (uint64_t)wg * cells_per_wg, c_end = min(n_outer, c_begin + cells_per_wg);
    for (uint64_t c4 = c_begin + (uint64_t)wave * CM_NV; c4 < c_end; c4 += (uint64_t)n_waves * CM_NV) {
        uint32_t len_l = 0, blo = 0, bhi = 0;
        if (lane < CM_NV && c4 + lane < c_end) {
            const uint32_t *bd = bounds + (c4 + lane) * (nb + 1);
            const uint32_t o0 = bd[b0];
            len_l = bd[b1] - o0;
            const uint64_t base = indptr[c4 + lane] + o0;
            blo = (uint32_t)base;
            bhi = (uint32_t)(base >> 32);
        }
        // lanes 8 r .. 8 r + 7: the chain at counts 1 .. 8 of cell r of this trip
        double tab = 0.0;
        if (lane < CM_NV * CM_TAB && c4 + lane / CM_TAB < c_end) tab = eval_map(map, (lane % CM_TAB) + 1u, (uint32_t)(c4 + lane / CM_TAB), 0u);
        uint32_t start[CM_NV + 1];
        uint64_t base[CM_NV];
        start[0] = 0;
#pragma unroll
        for (uint32_t r = 0; r < CM_NV; r++) {
            start[r + 1] = start[r] + rdlane(len_l, r);
            base[r] = ((uint64_t)rdlane(bhi, r) << 32) | rdlane(blo, r);
        }
        const uint32_t total = start[CM_NV];
        // four strides of 64 nonzeros per trip: their index and count loads go out together (one stride per trip made the walk a
        // chain of load latencies: 3.9 ms per pass instead of 2.x)
        constexpr uint32_t CM_U = 8;
        for (uint32_t q0 = 0; q0 < total; q0 += 64u * CM_U) {
            uint32_t g[CM_U], cnt[CM_U], r[CM_U];
            bool on[CM_U];
#pragma unroll
            for (uint32_t u = 0; u < CM_U; u++) {
                const uint32_t p_raw = q0 + 64u * u + lane;
                on[u] = p_raw < total;
                // no branch around the loads (a lane past the end re-reads the trip's last nonzero and is masked below): behind a
                // branch every stride waited for its own index before the next stride's loads went out
                const uint32_t p = on[u] ? p_raw : total - 1u;
                r[u] = 0;
                uint64_t a = base[0] + p;
#pragma unroll
                for (uint32_t rr = 1; rr < CM_NV; rr++)
                    if (p >= start[rr]) {
                        r[u] = rr;
                        a = base[rr] + (p - start[rr]);
                    }
                g[u] = indices[a] - g0;
                cnt[u] = values[a];
            }
#pragma unroll
            for (uint32_t u = 0; u < CM_U; u++) {
                if (q0 + 64u * u >= total) break; // uniform
                double v = __shfl(tab, (int)(r[u] * CM_TAB + min(cnt[u], CM_TAB) - 1u)); // every lane takes part in the exchange
                if (on[u]) {
                    if (cnt[u] > CM_TAB) v = eval_map(map, cnt[u], (uint32_t)(c4 + r[u]), 0u);
                    // 0 <= t < 2^51 (col_moments_plan): t + 2^52 holds round-to-nearest(t) in its mantissa — two instructions
                    // instead of the ~15 of a general f64 -> i64 conversion, which made this loop VALU-bound
                    atomicAdd(&cm_acc[g[u]], (unsigned long long)__double_as_longlong(v * scale1 + 4503599627370496.0) & 0x000FFFFFFFFFFFFFull);
                    if (MODE == 2)
                        atomicAdd(&cm_acc[(1u << CM_RANGE_SHIFT) + g[u]],
                                  (unsigned long long)__double_as_longlong(v * v * scale2 + 4503599627370496.0) & 0x000FFFFFFFFFFFFFull);
                }
            }
        }
    }
    __syncthreads();
    unsigned long long *dst = slab + ((size_t)range * gridDim.x + wg) * ((size_t)MODE << CM_RANGE_SHIFT);
    for (uint32_t i = tid; i < (MODE << CM_RANGE_SHIFT); i += blockDim.x) dst[i] = cm_acc[i];
    (void)ng;
}
// the partial sums of the workgroups, added in double in workgroup order
template <int MODE>
__global__ void col_moments_finish_kernel(const unsigned long long *__restrict__ slab, uint32_t n_wg, uint32_t n_inner, double inv1, double inv2,
                                          double *__restrict__ out_sum, double *__restrict__ out_sumsq) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_inner) return;
    const uint32_t range = g >> CM_RANGE_SHIFT, gi = g & ((1u << CM_RANGE_SHIFT) - 1u);
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t w = 0; w < n_wg; w++) {
        const unsigned long long *src = slab + ((size_t)range * n_wg + w) * ((size_t)MODE << CM_RANGE_SHIFT) + gi;
        s1 += (double)(long long)src[0];
        if (MODE == 2) s2 += (double)(long long)src[1u << CM_RANGE_SHIFT];
    }
    out_sum[g] = s1 * inv1;
    if (MODE == 2 && out_sumsq) out_sumsq[g] = s2 * inv2;
}
__global__ void max_u32_kernel(const uint32_t *__restrict__ v, uint64_t n, uint32_t *__restrict__ out) {
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) m = max(m, v[i]);
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63u) == 0) atomicMax(out, m);
}
// [0] = smallest POSITIVE, [1] = largest value as order-preserving bit patterns of non-negative doubles (zeros take part in neither:
// [0] stays ~0 when no factor is positive, [1] stays +0.0 when all are zero); [2] != 0: a negative or non-finite value
__global__ void minmax_nonneg_kernel(const double *__restrict__ v, uint64_t n, unsigned long long *__restrict__ out) {
    unsigned long long lo = ~0ull, hi = 0ull;
    int bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double x = v[i];
        if (!(x >= 0.0) || !isfinite(x)) {
            bad = 1;
        } else if (x > 0.0) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(x);
            lo = b < lo ? b : lo;
            hi = b > hi ? b : hi;
        }
    }
    atomicMin(&out[0], lo);
    atomicMax(&out[1], hi);
    if (bad) atomicMax(&out[2], 1ull);
}

// Can the per-inner sums of `map` over `cp` (outer = the summed-over axis) take col_moments_kernel? Every link must be a
// ScaleAxis over the OUTER position with non-negative finite factors or a logarithm (then the value is non-negative and grows
// with the count and with the factors: its largest and its smallest possible value follow from the counts' and the factors'
// extremes). The device supplies those extremes; the decision and the exponents are col_moments_plan.hpp's.
// Returns the fixed-point scales in s1 / s2; false = use the ordinary pass.
static bool col_moments_plan(Storage &st, SparseCopy &cp, const DevMap &map, int mode, uint32_t n_wg, double &s1, double &s2) {
    bool has_log = false;
    for (int i = 0; i < map.n; i++) {
        const int k = map.ops[i].kind;
        if (k == OP_SCALE_AXIS) {
            if (!map.ops[i].a_outer) return false;
        } else if (k == OP_LN_1P || k == OP_LOG2_1P || k == OP_LOG10_1P) {
            has_log = true;
        } else {
            return false;
        }
    }
    if (!has_log || cp.n_outer == 0 || cp.n_inner == 0) return false;
    if (cp.max_value == 0) { // structure only: once per copy
        uint32_t *d = st.scratch.get<uint32_t>("cm_maxv", 1);
        SCANRS_HIP(hipMemsetAsync(d, 0, 4, st.stream));
        hipLaunchKernelGGL(max_u32_kernel, dim3(2048), dim3(256), 0, st.stream, cp.values.p, cp.nnz, d);
        const uint32_t h = SCANRS_D2H_VALUE(d, st.stream);
        cp.max_value = std::max(h, 1u);
    }
    std::vector<col_moments::Link> links((size_t)map.n);
    unsigned long long *d = st.scratch.get<unsigned long long>("cm_minmax", 3);
    for (int i = 0; i < map.n; i++) {
        col_moments::Link &l = links[(size_t)i];
        l.kind = map.ops[i].kind;
        l.on_summed_axis = 1;
        l.fmin_pos = l.fmax = 0.0;
        if (l.kind != OP_SCALE_AXIS) continue;
        const unsigned long long init[3] = {~0ull, 0ull, 0ull};
        SCANRS_HIP(hipMemcpyAsync(d, init, sizeof init, hipMemcpyHostToDevice, st.stream));
        hipLaunchKernelGGL(minmax_nonneg_kernel, dim3(512), dim3(256), 0, st.stream, map.ops[i].a, cp.n_outer, d);
        struct H3 {
            unsigned long long v[3];
        };
        const H3 h3 = SCANRS_D2H_VALUE(reinterpret_cast<const H3 *>(d), st.stream);
        const unsigned long long *h = h3.v;
        if (h[2]) return false;
        memcpy(&l.fmax, &h[1], 8);
        if (h[0] != ~0ull) memcpy(&l.fmin_pos, &h[0], 8);
    }
    const col_moments::Plan p = col_moments::plan(cp.max_value, links.data(), map.n, cp.n_outer, cp.n_inner, n_wg, mode);
    if (!p.ok) return false;
    s1 = std::ldexp(1.0, p.e1);
    s2 = std::ldexp(1.0, p.e2);
    return true;
}
// out_sum[i] (and out_sumsq[i]) over the outer vectors of cp, per INNER position i. false: not eligible (nothing was launched).
bool launch_col_moments(Storage &st, SparseCopy &cp, const DevMap &map, int mode, double *out_sum, double *out_sumsq) {
    if (mode != 1 && mode != 2) return false;
    int dev = 0, n_cu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    const uint32_t n_ranges = (uint32_t)((cp.n_inner + (1ull << CM_RANGE_SHIFT) - 1) >> CM_RANGE_SHIFT);
    if (cp.n_inner >= (1ull << 31) || n_ranges > 65535u) return false;
    // one workgroup per CU and range at a time; the cells dealt over as many workgroups as keep every CU busy for all ranges
    const uint32_t n_wg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_cu, (cp.n_outer + 63) / 64));
    double s1 = 0.0, s2 = 0.0;
    if (!col_moments_plan(st, cp, map, mode, n_wg, s1, s2)) return false;
    const uint32_t nb = ensure_bounds(st, cp);
    const uint64_t cells_per_wg = (cp.n_outer + n_wg - 1) / n_wg;
    unsigned long long *slab = st.scratch.get<unsigned long long>("cm_slab", (size_t)n_ranges * n_wg * ((size_t)mode << CM_RANGE_SHIFT));
    const size_t shmem = ((size_t)mode << CM_RANGE_SHIFT) * 8;
    ProfScope ps(st, mode == 2 ? "col_moments" : "col_sums", (double)cp.nnz * 8.0 + (double)cp.n_outer * (n_ranges + 1) * 4.0);
    if (mode == 2) {
        SCANRS_HIP(hipFuncSetAttribute((const void *)col_moments_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL((col_moments_kernel<2>), dim3(n_wg, n_ranges), dim3(1024), shmem, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, cp.bounds.p, nb,
                           cp.n_outer, cells_per_wg, (uint32_t)cp.n_inner, map, s1, s2, slab);
        hipLaunchKernelGGL((col_moments_finish_kernel<2>), dim3((unsigned)((cp.n_inner + 255) / 256)), dim3(256), 0, st.stream, slab, n_wg, (uint32_t)cp.n_inner,
                           1.0 / s1, 1.0 / s2, out_sum, out_sumsq);
    } else {
        SCANRS_HIP(hipFuncSetAttribute((const void *)col_moments_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL((col_moments_kernel<1>), dim3(n_wg, n_ranges), dim3(1024), shmem, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, cp.bounds.p, nb,
                           cp.n_outer, cells_per_wg, (uint32_t)cp.n_inner, map, s1, s2, slab);
        hipLaunchKernelGGL((col_moments_finish_kernel<1>), dim3((unsigned)((cp.n_inner + 255) / 256)), dim3(256), 0, st.stream, slab, n_wg, (uint32_t)cp.n_inner,
                           1.0 / s1, 1.0 / s2, out_sum, (double *)nullptr);
    }
    SCANRS_HIP(hipGetLastError());
    return true;
}

void launch_finish_moments(Storage &st, const double *sum, const double *sumsq, uint64_t n, double m, int given_scale,
                           const double *scale_in, double *neg_mean_over_scale, double *inv_scale, double *scale_out) {
    if (n == 0) return;
    hipLaunchKernelGGL(finish_moments_kernel, grid1(n, 256), dim3(256), 0, st.stream, sum, sumsq, n, m, given_scale,
                       scale_in, neg_mean_over_scale, inv_scale, scale_out);
    SCANRS_HIP(hipGetLastError());
}
void launch_u32_to_scale(Storage &st, const uint32_t *counts, uint64_t n, double target, double *out) {
    if (n == 0) return;
    hipLaunchKernelGGL(u32_to_scale_kernel, grid1(n, 256), dim3(256), 0, st.stream, counts, n, target, out);
    SCANRS_HIP(hipGetLastError());
}
void launch_hist12(Storage &st, const uint32_t *v, uint64_t n, uint32_t shift, uint32_t digit_mask, uint32_t prefix_mask,
                   uint32_t prefix, unsigned long long *hist) {
    SCANRS_HIP(hipMemsetAsync(hist, 0, 4096 * sizeof(unsigned long long), st.stream));
    if (n) {
        const unsigned blocks = (unsigned)std::min<uint64_t>(1024, (n + 255) / 256);
        hipLaunchKernelGGL(hist12_kernel, dim3(blocks), dim3(256), 0, st.stream, v, n, shift, digit_mask, prefix_mask, prefix, hist);
    }
    SCANRS_HIP(hipGetLastError());
}
void launch_densify(Storage &st, const SparseCopy &cp, const DevMap &map, bool outer_is_view_row, uint64_t cols_v,
                    double *out) {
    if (cp.n_items == 0) return;
    hipLaunchKernelGGL(densify_kernel, dim3((cp.n_items + 3u) / 4u), dim3(256), 0, st.stream, cp.indices.p, cp.values.p,
                       cp.items.p, cp.n_items, map, outer_is_view_row ? 1 : 0, cols_v, out);
    SCANRS_HIP(hipGetLastError());
}
void launch_binom_uv(Storage &st, int kind, const double *n, uint64_t ncols, const double *rowsum, uint64_t nrows,
                     double total, double *pi, double *u, double *v) {
    if (nrows) hipLaunchKernelGGL(binom_rows_kernel, grid1(nrows, 256), dim3(256), 0, st.stream, kind, rowsum, nrows, total, pi, u);
    if (ncols) hipLaunchKernelGGL(binom_cols_kernel, grid1(ncols, 256), dim3(256), 0, st.stream, kind, n, ncols, v);
    SCANRS_HIP(hipGetLastError());
}
void launch_sum_f64(Storage &st, const double *x, uint64_t n, double *out) {
    hipLaunchKernelGGL(sum_f64_kernel, dim3(1), dim3(256), 0, st.stream, x, n, out);
    SCANRS_HIP(hipGetLastError());
}

// scanrs_init(): loads this file's code object (library_warm_up, kernels.hip)
__global__ void warm_normalize_ops_kernel() {}
void warm_normalize_ops(hipStream_t s) { hipLaunchKernelGGL(warm_normalize_ops_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
