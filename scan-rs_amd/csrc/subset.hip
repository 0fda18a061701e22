// HIP kernels of the statistics over a list of columns: sum_rows, sum_cols, sum_rows_dual, mean_rows, mean_var_rows
// (sqz/src/mat.rs:279-282, 333-374, 414-583) + their launchers. Host logic and the entry points: subset_host.cpp.
//
// A list names positions of ONE axis of a compressed copy: either its inner positions or its outer vectors. Three forms:
//
//   subset_reduce_kernel<MODE, NSETS>   MASKED WALK, the result axis is the copy's outer dimension. A table of one byte per inner
//                                       position says which lists hold it (bit 0: list 1, bit 1: list 2; made by subset_code_kernel,
//                                       1 MB at 10^6 cells: resident in an XCD's L2). A wave walks a work item as row_reduce_kernel
//                                       does (SCAN_U strides of 64 nonzeros in flight, coalesced index and value loads), gathers the
//                                       byte of each nonzero's inner position and accumulates per list. One walk serves both lists of
//                                       the dual forms. MODE 0: u64 sums of the raw counts; 1: f64 sums of the mapped values; 2: sum
//                                       and sum of squares. Vectors cut into several items meet in a slab, added in slab order by
//                                       subset_finish_kernel (no floating-point atomics anywhere: f64 results are bit-reproducible).
//   subset_listed_kernel<MODE>          LISTED VECTORS, the listed positions are outer vectors and every one of them is a result:
//                                       a wave per listed vector over its whole length, the sum written at the vector's place in
//                                       the list. Work follows the listed nonzeros, not the matrix.
//   subset_listed_scatter_kernel        SCATTER, integer results from the copy of the OTHER orientation (so that no transposed copy
//   subset_inner_scatter_kernel         has to be built): the walk over the listed vectors adds every nonzero into out[inner], the
//                                       walk over all work items adds every nonzero at a listed inner position into out[its place
//                                       in the list], both with 64-bit integer atomics (exact in any order).
//   subset_reduce_fx_kernel<MODE, NSETS> FIXED POINT, the f64 sums of a sharded handle that cross its shards: the masked walk and the
//   subset_listed_fx_kernel             listed vectors with 128-bit integer accumulators in place of the f64 ones, so that the partial
//                                       sums of the shards add up exactly (further down, with the pre-pass that finds the quantum
//                                       and the limbs of the exchange).
#include "common.hpp"
#include "device_map.hpp"
#include "fixed128.hpp"
#include "launch_util.hpp"

namespace scanrs {

namespace {
constexpr uint32_t NOT_LISTED = 0xFFFFFFFFu;
inline dim3 wave_grid(uint64_t n_waves) { return dim3((unsigned)((n_waves + 3) / 4)); }

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
} // namespace

// ---- the tables made from a list ---------------------------------------------------------------------------------------------------
// code[list[i]] |= bit. The entries of a list are distinct, so no two threads of a launch touch the same byte; the second list's launch
// runs behind the first one's.
__global__ void subset_code_kernel(const uint32_t *__restrict__ list, uint64_t n, uint8_t bit, uint8_t *__restrict__ code) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) code[list[i]] |= bit;
}
// pos[list[i]] = i (the table starts out as NOT_LISTED)
__global__ void subset_pos_kernel(const uint32_t *__restrict__ list, uint64_t n, uint32_t *__restrict__ pos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[list[i]] = (uint32_t)i;
}

// ---- masked walk -------------------------------------------------------------------------------------------------------------------
// Results of an item that is a whole vector: out[k * stride + row], k = the list (MODE 0 / 1) or 0 = sum, 1 = sum of squares (MODE 2).
// Partial results of a cut vector: slab[2 * slab_row + k].
template <int MODE, int NSETS>
__global__ __launch_bounds__(256) void subset_reduce_kernel(const uint32_t *__restrict__ indices, const uint32_t *__restrict__ values,
                                                            const Item *__restrict__ items, uint32_t n_items, DevMap map,
                                                            const uint8_t *__restrict__ code, unsigned long long *__restrict__ out_u64,
                                                            double *__restrict__ out_f64, uint64_t stride,
                                                            unsigned long long *__restrict__ slab_u64, double *__restrict__ slab_f64) {
    static_assert(MODE != 2 || NSETS == 1, "the moments are made for one list");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wid >= n_items) return;
    const Item it = items[wid];
    const uint32_t *__restrict__ ind = indices + it.start;
    const uint32_t *__restrict__ val = values + it.start;
    if constexpr (MODE == 0) {
        unsigned long long s0 = 0, s1 = 0;
        for (uint32_t p0 = lane; p0 < it.len; p0 += 64u * SCAN_U) {
            uint32_t g[SCAN_U], vv[SCAN_U];
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) {
                const uint32_t p = p0 + 64u * u;
                const bool ok = p < it.len;
                const uint32_t q = ok ? p : it.len - 1u;
                g[u] = ind[q];
                vv[u] = ok ? val[q] : 0u; // a position past the end adds nothing
            }
            uint8_t c[SCAN_U];
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) c[u] = code[g[u]];
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) {
                s0 += (c[u] & 1u) ? vv[u] : 0u;
                if constexpr (NSETS == 2) s1 += (c[u] & 2u) ? vv[u] : 0u;
            }
        }
        s0 = wave_sum_u64(s0);
        if constexpr (NSETS == 2) s1 = wave_sum_u64(s1);
        if (lane == 0) {
            if (it.slab == NO_SLAB) {
                out_u64[it.row] = s0;
                if constexpr (NSETS == 2) out_u64[stride + it.row] = s1;
            } else {
                slab_u64[2 * (size_t)it.slab] = s0;
                if constexpr (NSETS == 2) slab_u64[2 * (size_t)it.slab + 1] = s1;
            }
        }
    } else {
        const RowMap rm = row_map(map, it.row);
        double s0 = 0.0, s1 = 0.0; // MODE 1: the two lists' sums; MODE 2: sum and sum of squares
        for (uint32_t p0 = lane; p0 < it.len; p0 += 64u * SCAN_U) {
            uint32_t g[SCAN_U], vv[SCAN_U];
            bool ok[SCAN_U];
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) {
                const uint32_t p = p0 + 64u * u;
                ok[u] = p < it.len;
                const uint32_t q = ok[u] ? p : it.len - 1u;
                g[u] = ind[q];
                vv[u] = val[q];
            }
            uint8_t c[SCAN_U];
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) c[u] = ok[u] ? code[g[u]] : (uint8_t)0;
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) {
                if (!c[u]) continue; // the map (its logarithm, its gathers) is evaluated for listed positions only
                const double x = eval_map(map, rm, vv[u], it.row, g[u]);
                if constexpr (MODE == 2) {
                    s0 += x;
                    s1 = fma(x, x, s1);
                } else {
                    s0 = (c[u] & 1u) ? s0 + x : s0;
                    if constexpr (NSETS == 2) s1 = (c[u] & 2u) ? s1 + x : s1;
                }
            }
        }
        constexpr bool TWO = MODE == 2 || NSETS == 2;
        s0 = wave_sum(s0);
        if constexpr (TWO) s1 = wave_sum(s1);
        if (lane == 0) {
            if (it.slab == NO_SLAB) {
                out_f64[it.row] = s0;
                if constexpr (TWO) out_f64[stride + it.row] = s1;
            } else {
                slab_f64[2 * (size_t)it.slab] = s0;
                if constexpr (TWO) slab_f64[2 * (size_t)it.slab + 1] = s1;
            }
        }
    }
}

// the partial results of the cut vectors, added in slab order; n_k: values per slab row in use (1 or 2)
template <typename T>
__global__ void subset_finish_kernel(const MultiRow *__restrict__ multi, uint32_t n_multi, const T *__restrict__ slab, int n_k,
                                     T *__restrict__ out, uint64_t stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_multi) return;
    const MultiRow mr = multi[i];
    for (int k = 0; k < n_k; k++) {
        T s = 0;
        for (uint32_t j = 0; j < mr.count; j++) s += slab[2 * (size_t)(mr.first_slab + j) + k];
        out[(uint64_t)k * stride + mr.row] = s;
    }
}

// the same walk with the result per listed INNER position: out[pos[inner]] += count (integer atomics)
__global__ __launch_bounds__(256) void subset_inner_scatter_kernel(const uint32_t *__restrict__ indices, const uint32_t *__restrict__ values,
                                                                   const Item *__restrict__ items, uint32_t n_items,
                                                                   const uint32_t *__restrict__ pos, unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wid >= n_items) return;
    const Item it = items[wid];
    const uint32_t *__restrict__ ind = indices + it.start;
    const uint32_t *__restrict__ val = values + it.start;
    for (uint32_t p0 = lane; p0 < it.len; p0 += 64u * SCAN_U) {
        uint32_t g[SCAN_U], vv[SCAN_U];
        bool ok[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; u++) {
            const uint32_t p = p0 + 64u * u;
            ok[u] = p < it.len;
            const uint32_t q = ok[u] ? p : it.len - 1u;
            g[u] = ind[q];
            vv[u] = val[q];
        }
        uint32_t at[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; u++) at[u] = ok[u] ? pos[g[u]] : NOT_LISTED;
#pragma unroll
        for (int u = 0; u < SCAN_U; u++)
            if (at[u] != NOT_LISTED) atomicAdd(out + at[u], (unsigned long long)vv[u]);
    }
}

// ---- listed vectors ----------------------------------------------------------------------------------------------------------------
template <int MODE> // 0: u64 sum of the raw counts, 1: f64 sum of the mapped values
__global__ __launch_bounds__(256) void subset_listed_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                            const uint32_t *__restrict__ values, const uint32_t *__restrict__ list,
                                                            uint64_t n_list, DevMap map, unsigned long long *__restrict__ out_u64,
                                                            double *__restrict__ out_f64) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_list) return;
    const uint32_t o = list[i];
    const uint64_t a = indptr[o];
    const uint32_t len = (uint32_t)(indptr[o + 1] - a); // (a vector is no longer than the inner dimension, which fits u32)
    const uint32_t *__restrict__ ind = indices + a;
    const uint32_t *__restrict__ val = values + a;
    if constexpr (MODE == 0) {
        unsigned long long s = 0;
        for (uint32_t p0 = lane; p0 < len; p0 += 64u * 8u) {
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t p = p0 + 64u * u;
                v[u] = p < len ? val[p] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) s += v[u];
        }
        s = wave_sum_u64(s);
        if (lane == 0) out_u64[i] = s;
    } else {
        const RowMap rm = row_map(map, o);
        double s = 0.0;
        for (uint32_t p0 = lane; p0 < len; p0 += 64u * SCAN_U) {
            uint32_t g[SCAN_U], vv[SCAN_U];
            bool ok[SCAN_U];
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) {
                const uint32_t p = p0 + 64u * u;
                ok[u] = p < len;
                const uint32_t q = ok[u] ? p : len - 1u;
                g[u] = ind[q];
                vv[u] = val[q];
            }
#pragma unroll
            for (int u = 0; u < SCAN_U; u++) {
                const double x = eval_map(map, rm, vv[u], o, g[u]);
                s = ok[u] ? s + x : s;
            }
        }
        s = wave_sum(s);
        if (lane == 0) out_f64[i] = s;
    }
}

// out[inner] += count over the listed vectors (integer atomics)
__global__ __launch_bounds__(256) void subset_listed_scatter_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                                    const uint32_t *__restrict__ values, const uint32_t *__restrict__ list,
                                                                    uint64_t n_list, unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_list) return;
    const uint32_t o = list[i];
    const uint64_t a = indptr[o];
    const uint32_t len = (uint32_t)(indptr[o + 1] - a);
    const uint32_t *__restrict__ ind = indices + a;
    const uint32_t *__restrict__ val = values + a;
    for (uint32_t p0 = lane; p0 < len; p0 += 64u * SCAN_U) {
        uint32_t g[SCAN_U], vv[SCAN_U];
        bool ok[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; u++) {
            const uint32_t p = p0 + 64u * u;
            ok[u] = p < len;
            const uint32_t q = ok[u] ? p : len - 1u;
            g[u] = ind[q];
            vv[u] = val[q];
        }
#pragma unroll
        for (int u = 0; u < SCAN_U; u++)
            if (ok[u]) atomicAdd(out + g[u], (unsigned long long)vv[u]);
    }
}

// ---- fixed-point forms: sums that cross the shards ---------------------------------------------------------------------
// The same two walks with every mapped value rounded ONCE to the call's quantum (1 / scale, the same on every rank) and summed as
// signed 128-bit integers (fixed128.hpp): per lane, across the wave with shfl_down128, across the slab for cut vectors, and across the
// shards as 32-bit limbs. No floating-point addition lies between a term and the host's final conversion, so the result depends
// neither on the cut into shards nor on the order in which anything arrives. A term that is not finite, or that the quantum cannot
// hold (its bound overflowed: the host then passes a NaN scale), sets the bit of its sum in the result's flag instead of being added.
namespace {
constexpr double FX_TERM_LIMIT = 0x1p125; // a term under the call's scale lies below 2^124 (subset_host.cpp: fx_scale)

__device__ __forceinline__ void fx_add(U128 &s, uint32_t &flags, uint32_t bit, double t, double scale) {
    if (!(fabs(t * scale) < FX_TERM_LIMIT)) { // (false for a NaN too)
        flags |= bit;
        return;
    }
    add128(s, to_fixed_signed(t, scale));
}
__device__ __forceinline__ void fx_wave_sum(U128 &s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) add128(s, shfl_down128(s, off));
}
__device__ __forceinline__ uint32_t fx_wave_or(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= (uint32_t)__shfl_down((int)v, off, 64);
    return v;
}
__device__ __forceinline__ double fx_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
// the largest finite magnitude so far (the bit patterns of non-negative doubles order as the numbers do)
__device__ __forceinline__ double fx_max_term(double mx, double x) {
    const double a = fabs(x);
    return a <= 1.7976931348623157e308 ? fmax(mx, a) : mx;
}
__device__ __forceinline__ void fx_publish_max(double mx, uint32_t lane, unsigned long long *out) {
    mx = fx_wave_max(mx);
    if (lane == 0 && mx > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(mx));
}

// f(code byte, mapped value) for the listed nonzeros of a work item, loaded as subset_reduce_kernel loads them
template <class F>
__device__ __forceinline__ void masked_terms(const uint32_t *__restrict__ ind, const uint32_t *__restrict__ val, uint32_t len, uint32_t lane,
                                             const uint8_t *__restrict__ code, const DevMap &map, const RowMap &rm, uint32_t row, F &&f) {
    for (uint32_t p0 = lane; p0 < len; p0 += 64u * SCAN_U) {
        uint32_t g[SCAN_U], vv[SCAN_U];
        bool ok[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; u++) {
            const uint32_t p = p0 + 64u * u;
            ok[u] = p < len;
            const uint32_t q = ok[u] ? p : len - 1u;
            g[u] = ind[q];
            vv[u] = val[q];
        }
        uint8_t c[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; u++) c[u] = ok[u] ? code[g[u]] : (uint8_t)0;
#pragma unroll
        for (int u = 0; u < SCAN_U; u++)
            if (c[u]) f(c[u], eval_map(map, rm, vv[u], row, g[u])); // the map is evaluated for listed positions only
    }
}
// f(mapped value) for every nonzero of a listed vector, as subset_listed_kernel walks it
template <class F>
__device__ __forceinline__ void listed_terms(const uint32_t *__restrict__ ind, const uint32_t *__restrict__ val, uint32_t len, uint32_t lane,
                                             const DevMap &map, const RowMap &rm, uint32_t o, F &&f) {
    for (uint32_t p0 = lane; p0 < len; p0 += 64u * SCAN_U) {
        uint32_t g[SCAN_U], vv[SCAN_U];
        bool ok[SCAN_U];
#pragma unroll
        for (int u = 0; u < SCAN_U; u++) {
            const uint32_t p = p0 + 64u * u;
            ok[u] = p < len;
            const uint32_t q = ok[u] ? p : len - 1u;
            g[u] = ind[q];
            vv[u] = val[q];
        }
#pragma unroll
        for (int u = 0; u < SCAN_U; u++)
            if (ok[u]) f(eval_map(map, rm, vv[u], o, g[u]));
    }
}
} // namespace

// Results of an item that is a whole vector: fx[4 * row ..] = lo, hi of the first sum, lo, hi of the second; bad[row] = the flags
// (bit 0: first sum, bit 1: second). Partial results of a cut vector: slab[5 * slab_row ..] = the four words and the flags.
// MODE 1: the sums of the one or two lists under scale1; MODE 2: sum under scale1 and sum of squares (x * x, rounded once) under scale2.
template <int MODE, int NSETS>
__global__ __launch_bounds__(256) void subset_reduce_fx_kernel(const uint32_t *__restrict__ indices, const uint32_t *__restrict__ values,
                                                               const Item *__restrict__ items, uint32_t n_items, DevMap map,
                                                               const uint8_t *__restrict__ code, double scale1, double scale2,
                                                               unsigned long long *__restrict__ fx, uint32_t *__restrict__ bad,
                                                               unsigned long long *__restrict__ slab) {
    static_assert(MODE == 1 || (MODE == 2 && NSETS == 1), "the moments are made for one list");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wid >= n_items) return;
    const Item it = items[wid];
    const RowMap rm = row_map(map, it.row);
    U128 s0{0, 0}, s1{0, 0};
    uint32_t flags = 0;
    masked_terms(indices + it.start, values + it.start, it.len, lane, code, map, rm, it.row, [&](uint8_t c, double x) {
        if constexpr (MODE == 2) {
            fx_add(s0, flags, 1u, x, scale1);
            fx_add(s1, flags, 2u, x * x, scale2);
        } else {
            if (c & 1u) fx_add(s0, flags, 1u, x, scale1);
            if constexpr (NSETS == 2)
                if (c & 2u) fx_add(s1, flags, 2u, x, scale1);
        }
    });
    fx_wave_sum(s0);
    if constexpr (MODE == 2 || NSETS == 2) fx_wave_sum(s1);
    flags = fx_wave_or(flags);
    if (lane == 0) {
        if (it.slab == NO_SLAB) {
            unsigned long long *o = fx + 4 * (size_t)it.row;
            o[0] = s0.lo, o[1] = s0.hi, o[2] = s1.lo, o[3] = s1.hi;
            bad[it.row] = flags;
        } else {
            unsigned long long *o = slab + 5 * (size_t)it.slab;
            o[0] = s0.lo, o[1] = s0.hi, o[2] = s1.lo, o[3] = s1.hi, o[4] = flags;
        }
    }
}

// the partial results of the cut vectors (integer sums: any order gives the same words)
__global__ void subset_finish_fx_kernel(const MultiRow *__restrict__ multi, uint32_t n_multi, const unsigned long long *__restrict__ slab,
                                        unsigned long long *__restrict__ fx, uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_multi) return;
    const MultiRow mr = multi[i];
    U128 s0{0, 0}, s1{0, 0};
    unsigned long long flags = 0;
    for (uint32_t j = 0; j < mr.count; j++) {
        const unsigned long long *p = slab + 5 * (size_t)(mr.first_slab + j);
        add128(s0, U128{p[0], p[1]});
        add128(s1, U128{p[2], p[3]});
        flags |= p[4];
    }
    unsigned long long *o = fx + 4 * (size_t)mr.row;
    o[0] = s0.lo, o[1] = s0.hi, o[2] = s1.lo, o[3] = s1.hi;
    bad[mr.row] = (uint32_t)flags;
}

__global__ __launch_bounds__(256) void subset_listed_fx_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                               const uint32_t *__restrict__ values, const uint32_t *__restrict__ list,
                                                               uint64_t n_list, DevMap map, double scale1, unsigned long long *__restrict__ fx,
                                                               uint32_t *__restrict__ bad) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_list) return;
    const uint32_t o = list[i];
    const uint64_t a = indptr[o];
    const uint32_t len = (uint32_t)(indptr[o + 1] - a);
    const RowMap rm = row_map(map, o);
    U128 s{0, 0};
    uint32_t flags = 0;
    listed_terms(indices + a, values + a, len, lane, map, rm, o, [&](double x) { fx_add(s, flags, 1u, x, scale1); });
    fx_wave_sum(s);
    flags = fx_wave_or(flags);
    if (lane == 0) {
        unsigned long long *p = fx + 4 * (size_t)i;
        p[0] = s.lo, p[1] = s.hi, p[2] = 0ull, p[3] = 0ull;
        bad[i] = flags;
    }
}

// the pre-pass of the quantum: the largest finite |mapped value| over the listed nonzeros, as its bit pattern (integer atomicMax)
__global__ __launch_bounds__(256) void subset_reduce_max_kernel(const uint32_t *__restrict__ indices, const uint32_t *__restrict__ values,
                                                                const Item *__restrict__ items, uint32_t n_items, DevMap map,
                                                                const uint8_t *__restrict__ code, unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wid >= n_items) return;
    const Item it = items[wid];
    const RowMap rm = row_map(map, it.row);
    double mx = 0.0;
    masked_terms(indices + it.start, values + it.start, it.len, lane, code, map, rm, it.row, [&](uint8_t, double x) { mx = fx_max_term(mx, x); });
    fx_publish_max(mx, lane, out);
}
__global__ __launch_bounds__(256) void subset_listed_max_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                                const uint32_t *__restrict__ values, const uint32_t *__restrict__ list,
                                                                uint64_t n_list, DevMap map, unsigned long long *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_list) return;
    const uint32_t o = list[i];
    const uint64_t a = indptr[o];
    const uint32_t len = (uint32_t)(indptr[o + 1] - a);
    const RowMap rm = row_map(map, o);
    double mx = 0.0;
    listed_terms(indices + a, values + a, len, lane, map, rm, o, [&](double x) { mx = fx_max_term(mx, x); });
    fx_publish_max(mx, lane, out);
}

// ---- the 128-bit sums across the shards ------------------------------------------------------------------------------------------------
// As sseq_mom_split_kernel / sseq_mom_join_kernel (sseq.hip), for n_sums sums per result: each sum's two words as four 32-bit limbs
// held in u64 and its flag, 5 u64 per sum. The limbs of up to 2^31 ranks add up without overflow and the join propagates the carries;
// a carry out of the top limb is dropped, which is what two's complement addition asks for.
__global__ void subset_fx_split_kernel(const unsigned long long *__restrict__ fx, const uint32_t *__restrict__ bad, uint64_t n, int n_sums,
                                       unsigned long long *__restrict__ limbs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int s = 0; s < n_sums; s++) {
        unsigned long long *out = limbs + (i * (uint64_t)n_sums + s) * 5u;
        const unsigned long long lo = fx[4 * i + 2 * s], hi = fx[4 * i + 2 * s + 1];
        out[0] = lo & 0xFFFFFFFFull;
        out[1] = lo >> 32;
        out[2] = hi & 0xFFFFFFFFull;
        out[3] = hi >> 32;
        out[4] = (bad[i] >> s) & 1u;
    }
}
__global__ void subset_fx_join_kernel(const unsigned long long *__restrict__ limbs, uint64_t n, int n_sums, unsigned long long *__restrict__ fx,
                                      uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t flags = 0;
    for (int s = 0; s < n_sums; s++) {
        const unsigned long long *in = limbs + (i * (uint64_t)n_sums + s) * 5u;
        unsigned long long c = 0, r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            c = (c >> 32) + in[k]; // carry < 2^32 and a limb sum < 2^63: no overflow
            r[k] = c & 0xFFFFFFFFull;
        }
        fx[4 * i + 2 * s] = r[0] | (r[1] << 32);
        fx[4 * i + 2 * s + 1] = r[2] | (r[3] << 32);
        if (in[4]) flags |= 1u << s;
    }
    bad[i] = flags;
}

// ---- launchers (all on st.stream) ----------------------------------------------------------------------------------------------------
void launch_subset_reduce_fx(Storage &st, const SparseCopy &cp, const DevMap &map, int mode, int n_sets, const uint8_t *d_code, double scale1,
                             double scale2, unsigned long long *d_fx, uint32_t *d_bad, unsigned long long *d_slab) {
    // (vectors without a work item keep zeros)
    SCANRS_HIP(hipMemsetAsync(d_fx, 0, std::max<uint64_t>(1, cp.n_outer) * 32, st.stream));
    SCANRS_HIP(hipMemsetAsync(d_bad, 0, std::max<uint64_t>(1, cp.n_outer) * 4, st.stream));
    if (cp.n_items == 0) return;
    const dim3 grid = wave_grid(cp.n_items), block(256);
    if (st.prof.on) st.prof.begin(st.stream, "subset_fx_walk", (double)cp.nnz * 8.0);
#define SUBSET_REDUCE_FX(M, N)                                                                                                              \
    hipLaunchKernelGGL((subset_reduce_fx_kernel<M, N>), grid, block, 0, st.stream, cp.indices.p, cp.values.p, cp.items.p, cp.n_items, map, \
                       d_code, scale1, scale2, d_fx, d_bad, d_slab)
    if (mode == 2)
        SUBSET_REDUCE_FX(2, 1);
    else if (n_sets == 1)
        SUBSET_REDUCE_FX(1, 1);
    else
        SUBSET_REDUCE_FX(1, 2);
#undef SUBSET_REDUCE_FX
    SCANRS_HIP(hipGetLastError());
    if (cp.n_multi)
        hipLaunchKernelGGL(subset_finish_fx_kernel, grid1(cp.n_multi, 256), dim3(256), 0, st.stream, cp.multi.p, cp.n_multi, d_slab, d_fx, d_bad);
    SCANRS_HIP(hipGetLastError());
    if (st.prof.on) st.prof.end(st.stream);
}
void launch_subset_listed_fx(Storage &st, const SparseCopy &cp, const DevMap &map, const uint32_t *d_list, uint64_t n, double scale1,
                             unsigned long long *d_fx, uint32_t *d_bad) {
    if (!n) return;
    if (st.prof.on) st.prof.begin(st.stream, "subset_fx_walk", 0.0);
    hipLaunchKernelGGL(subset_listed_fx_kernel, wave_grid(n), dim3(256), 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, d_list, n, map,
                       scale1, d_fx, d_bad);
    SCANRS_HIP(hipGetLastError());
    if (st.prof.on) st.prof.end(st.stream);
}
void launch_subset_reduce_max(Storage &st, const SparseCopy &cp, const DevMap &map, const uint8_t *d_code, unsigned long long *d_max) {
    if (cp.n_items == 0) return;
    if (st.prof.on) st.prof.begin(st.stream, "subset_fx_bound", (double)cp.nnz * 8.0);
    hipLaunchKernelGGL(subset_reduce_max_kernel, wave_grid(cp.n_items), dim3(256), 0, st.stream, cp.indices.p, cp.values.p, cp.items.p,
                       cp.n_items, map, d_code, d_max);
    SCANRS_HIP(hipGetLastError());
    if (st.prof.on) st.prof.end(st.stream);
}
void launch_subset_listed_max(Storage &st, const SparseCopy &cp, const DevMap &map, const uint32_t *d_list, uint64_t n, unsigned long long *d_max) {
    if (!n) return;
    if (st.prof.on) st.prof.begin(st.stream, "subset_fx_bound", 0.0);
    hipLaunchKernelGGL(subset_listed_max_kernel, wave_grid(n), dim3(256), 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, d_list, n, map,
                       d_max);
    SCANRS_HIP(hipGetLastError());
    if (st.prof.on) st.prof.end(st.stream);
}
void launch_subset_fx_split(Storage &st, const unsigned long long *d_fx, const uint32_t *d_bad, uint64_t n, int n_sums, unsigned long long *d_limbs) {
    if (!n) return;
    hipLaunchKernelGGL(subset_fx_split_kernel, grid1(n, 256), dim3(256), 0, st.stream, d_fx, d_bad, n, n_sums, d_limbs);
    SCANRS_HIP(hipGetLastError());
}
void launch_subset_fx_join(Storage &st, const unsigned long long *d_limbs, uint64_t n, int n_sums, unsigned long long *d_fx, uint32_t *d_bad) {
    if (!n) return;
    hipLaunchKernelGGL(subset_fx_join_kernel, grid1(n, 256), dim3(256), 0, st.stream, d_limbs, n, n_sums, d_fx, d_bad);
    SCANRS_HIP(hipGetLastError());
}

void launch_subset_code(Storage &st, const uint32_t *d_list, uint64_t n, uint8_t bit, uint8_t *d_code) {
    if (!n) return;
    hipLaunchKernelGGL(subset_code_kernel, grid1(n, 256), dim3(256), 0, st.stream, d_list, n, bit, d_code);
    SCANRS_HIP(hipGetLastError());
}
void launch_subset_pos(Storage &st, const uint32_t *d_list, uint64_t n, uint32_t *d_pos) {
    if (!n) return;
    hipLaunchKernelGGL(subset_pos_kernel, grid1(n, 256), dim3(256), 0, st.stream, d_list, n, d_pos);
    SCANRS_HIP(hipGetLastError());
}

void launch_subset_reduce(Storage &st, const SparseCopy &cp, const DevMap &map, int mode, int n_sets, const uint8_t *d_code, void *d_out,
                          uint64_t stride, void *d_slab) {
    if (cp.n_items == 0) return;
    const dim3 grid = wave_grid(cp.n_items), block(256);
    unsigned long long *ou = static_cast<unsigned long long *>(d_out), *su = static_cast<unsigned long long *>(d_slab);
    double *of = static_cast<double *>(d_out), *sf = static_cast<double *>(d_slab);
#define SUBSET_REDUCE(M, N)                                                                                                              \
    hipLaunchKernelGGL((subset_reduce_kernel<M, N>), grid, block, 0, st.stream, cp.indices.p, cp.values.p, cp.items.p, cp.n_items, map, \
                       d_code, ou, of, stride, su, sf)
    if (mode == 0 && n_sets == 1)
        SUBSET_REDUCE(0, 1);
    else if (mode == 0)
        SUBSET_REDUCE(0, 2);
    else if (mode == 1 && n_sets == 1)
        SUBSET_REDUCE(1, 1);
    else if (mode == 1)
        SUBSET_REDUCE(1, 2);
    else
        SUBSET_REDUCE(2, 1);
#undef SUBSET_REDUCE
    SCANRS_HIP(hipGetLastError());
}
void launch_subset_finish(Storage &st, const SparseCopy &cp, int mode, int n_k, const void *d_slab, void *d_out, uint64_t stride) {
    if (cp.n_multi == 0) return;
    const dim3 grid = grid1(cp.n_multi, 256), block(256);
    if (mode == 0)
        hipLaunchKernelGGL((subset_finish_kernel<unsigned long long>), grid, block, 0, st.stream, cp.multi.p, cp.n_multi,
                           static_cast<const unsigned long long *>(d_slab), n_k, static_cast<unsigned long long *>(d_out), stride);
    else
        hipLaunchKernelGGL((subset_finish_kernel<double>), grid, block, 0, st.stream, cp.multi.p, cp.n_multi, static_cast<const double *>(d_slab),
                           n_k, static_cast<double *>(d_out), stride);
    SCANRS_HIP(hipGetLastError());
}
void launch_subset_inner_scatter(Storage &st, const SparseCopy &cp, const uint32_t *d_pos, unsigned long long *d_out) {
    if (cp.n_items == 0) return;
    hipLaunchKernelGGL(subset_inner_scatter_kernel, wave_grid(cp.n_items), dim3(256), 0, st.stream, cp.indices.p, cp.values.p, cp.items.p,
                       cp.n_items, d_pos, d_out);
    SCANRS_HIP(hipGetLastError());
}
void launch_subset_listed(Storage &st, const SparseCopy &cp, const DevMap &map, int mode, const uint32_t *d_list, uint64_t n, void *d_out) {
    if (!n) return;
    const dim3 grid = wave_grid(n), block(256);
    if (mode == 0)
        hipLaunchKernelGGL((subset_listed_kernel<0>), grid, block, 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, d_list, n, map,
                           static_cast<unsigned long long *>(d_out), (double *)nullptr);
    else
        hipLaunchKernelGGL((subset_listed_kernel<1>), grid, block, 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, d_list, n, map,
                           (unsigned long long *)nullptr, static_cast<double *>(d_out));
    SCANRS_HIP(hipGetLastError());
}
void launch_subset_listed_scatter(Storage &st, const SparseCopy &cp, const uint32_t *d_list, uint64_t n, unsigned long long *d_out) {
    if (!n) return;
    hipLaunchKernelGGL(subset_listed_scatter_kernel, wave_grid(n), dim3(256), 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, d_list, n,
                       d_out);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs
